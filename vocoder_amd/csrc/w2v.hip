// wav2vec2 / HuBERT encoder (include/fishvoc.h fv_w2v_*): the reference's modules/encoders/hubert.py in eval mode, for the "stable layer
// norm" family of HF's HubertModel / Wav2Vec2Model (feat_extract_norm = "layer", do_stable_layer_norm, conv_bias, feat_proj_layer_norm).
// Activations are TIME MAJOR, (row, frame, channel), so a strided conv's window — taps x channels — is one contiguous run of the input and
// every matrix product of the network is the same implicit GEMM:
//   w2v_gemm   y[t][n] = epi(sum_k a[t][k] w[n][k] + bias[n])   a[t][k] = in[t stride - pad + k / Cg][group Cg + k % Cg], 0 outside the row
//              the conv layers (K = k C_in; layer 0: K = 10, a FIR), the projection, the grouped positional conv (K = k H / g per group),
//              q | k | v as one product, out_proj and the second FFN product (+ residual), the first (GELU), the three post convs (SiLU;
//              the last one stores channel major, the reference's layout)
//   w2v_ln     LayerNorm over a frame's channels, one wave per frame, the row in registers; optionally GELU after (the feature extractor)
//   w2v_attn   per (row, head, 128 queries): S' = K Q' / 8 on MFMA for 32 keys at a time, running maximum and sum per query, O' += V' P with
//              P straight from S's accumulator registers (the key order of that product is the accumulator's row order, a fixed
//              permutation); no frames x frames tensor exists
// The GEMM is exact fp32 on v_mfma_f32_32x32x2_f32, 128 frames x 128 channels per workgroup (64 x 64 per wave) where that fills the chip,
// 64 x 128 or 64 x 64 where it does not; K is staged through LDS 16 or 32 at a time with the next stage's loads in flight.  LayerNorm +
// GELU of the feature extractor is a separate in-place launch after the conv (profiles/LOG.md has its share); fusing it into the epilogue needs a workgroup that holds all 512 channels of its frames.
// Ragged rows: lengths travel by value (LaunchTable), as frame counts before and after the launch's layer.  A frame, key or sample at or
// past a row's count is never loaded; outputs and hidden states hold exact zeros there.  An element's sum is one accumulator chain over k
// ascending (zeros where the window leaves the row), then the bias: fixed by the layer's shape and the row's length alone, so a row has
// the same bits alone, in any batch and padded to any T.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>

#include "conv_mfma_impl.h"

namespace fv {
namespace {

constexpr int kW2vRows = 128;                       // rows per launch: their frame counts are a LaunchTable
constexpr int kW2vMaxLn = 1024;                     // widest LayerNorm row: 4 float4 per lane
constexpr int kW2vMaxWide = 8192, kW2vMaxLayers = 64, kW2vMaxConv = 8, kW2vHeadDim = 64;
constexpr long long kW2vMaxSamples = 1LL << 30;
constexpr float kW2vEps = 1e-5f;

struct W2vLen {
    int in, out;                                    // valid frames of the launch's input and output
};
using W2vRowBlock = LaunchTable<W2vLen, kW2vRows>;
using W2vSampleBlock = LaunchTable<int, kW2vRows>;

enum W2vEpi : int { W2V_BIAS = 0, W2V_GELU = 1, W2V_SILU = 2, W2V_RES = 3, W2V_GELU_RES = 4, W2V_BIAS_CM = 5 };

struct W2vGemmParams {
    const float* a;                 // input frames: element (b, f, c) at b * a_bstride + f * a_rstride + c
    long long a_bstride;
    int a_rstride;
    int Cg, stride, pad, K;         // K = taps * Cg; a[t][k] = in[t * stride - pad + k / Cg][group * Cg + k % Cg]
    const float* w;                 // (N, K)
    const float* bias;              // (N)
    int N, Ng;                      // output channels, and per group
    float* y;                       // (b, Fout, N); W2V_BIAS_CM: (b, N, Fout)
    const float* r;                 // residual, laid out as y
    int Fout, row0;
};


// Four waves, two along the frames by two along the channels, each with FT x CT accumulators of 32 frames x 32 channels: a workgroup covers
// 64 FT frames x 64 CT channels, and stages BK of K at a time (a small tile has few MFMAs per stage, so it takes a deeper stage to keep
// the loads covered).  The loads of stage s + 2 are issued when stage s begins.  VEC: 16-byte loads, four k at a time — every layer whose
// window is made of runs of a multiple of four channels, which is every one but the FIR on the wave.  Every load is unconditional on an
// address clamped INTO the row's valid frames (and the weight's rows), and the bounds test selects the loaded value or zero: a conditional
// load would make the compiler branch around each one and wait for it alone.  Nothing outside a row's own frames is read either way.
// An element's sum is over k ascending whatever the tile, so the launcher picks the tile by the grid alone.
template <int EPI, int FT, int CT, int BK, bool VEC>
__global__ __launch_bounds__(256) void w2v_gemm_kernel(const W2vGemmParams p, const W2vRowBlock rows) {
    constexpr int FB = 64 * FT, CB = 64 * CT, LD = BK + 1;
    constexpr int KV = VEC ? 4 : 1, KT = BK / KV, RP = 256 / KT, NA = FB / RP, NW = CB / RP;       // a thread stages KV columns of rows sr + RP i
    static_assert(NA >= 1 && NW >= 1, "a pass of the staging covers at most the tile");
    using vec_t = std::conditional_t<VEC, float4, float>;
    __shared__ float As[2][FB * LD];
    __shared__ float Ws[2][CB * LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wt = wave & 1, wc = wave >> 1;
    const int bl = blockIdx.z;
    const long long b = p.row0 + bl;
    const int len_in = rows.e[bl].in, len_out = rows.e[bl].out;
    const int t0 = blockIdx.x * FB;
    if (t0 >= p.Fout) return;
    const int tiles_per_group = (p.Ng + CB - 1) / CB;
    const int group = blockIdx.y / tiles_per_group;
    const int n0 = group * p.Ng + (blockIdx.y - group * tiles_per_group) * CB;
    const int nend = min((group + 1) * p.Ng, n0 + CB);

    f32x16 acc[CT][FT];       // [channel sub-tile][frame sub-tile]
#pragma unroll
    for (int ic = 0; ic < CT; ++ic)
#pragma unroll
        for (int it = 0; it < FT; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ic][it][r] = 0.f;

    if (t0 < len_out) {         // so the row holds at least one input frame: the clamped addresses below exist
        const float* __restrict__ ab = p.a + b * p.a_bstride + (long long)group * p.Cg;
        const int sk = (tid % KT) * KV, sr = tid / KT;
        vec_t pa[2][NA], pw[2][NW];
        auto stage_load = [&](auto slot_c, int k0) {
            constexpr int slot = decltype(slot_c)::value;
            const int k = k0 + sk;
            const bool kin = k < p.K;                       // VEC: K is a multiple of 4, so the four stand or fall together
            const int kc = min(k, p.K - KV);
            const int j = kc / p.Cg, c = kc - j * p.Cg;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int t = t0 + sr + RP * i, f = t * p.stride - p.pad + j;
                const bool ok = kin && t < len_out && f >= 0 && f < len_in;
                const vec_t v = *reinterpret_cast<const vec_t*>(ab + (long long)min(max(f, 0), len_in - 1) * p.a_rstride + c);
                pa[slot][i] = ok ? v : vec_t{};
            }
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int n = n0 + sr + RP * i;
                const vec_t u = *reinterpret_cast<const vec_t*>(p.w + (long long)min(n, nend - 1) * p.K + kc);
                pw[slot][i] = kin && n < nend ? u : vec_t{};
            }
        };
        auto lds_put = [&](float* dst, const vec_t& v) {
            if constexpr (VEC) dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
            else dst[0] = v;
        };
        const int nstage = (p.K + BK - 1) / BK;
        const int lrow = lane & 31, lh = lane >> 5;
        // stage s lives in register slot and LDS buffer s & 1: the buffer was last read in stage s - 2, and every wave has passed the
        // barrier of stage s - 1 since
        auto step = [&](auto slot_c, int s) {
            constexpr int slot = decltype(slot_c)::value;
#pragma unroll
            for (int i = 0; i < NA; ++i) lds_put(&As[slot][(sr + RP * i) * LD + sk], pa[slot][i]);
#pragma unroll
            for (int i = 0; i < NW; ++i) lds_put(&Ws[slot][(sr + RP * i) * LD + sk], pw[slot][i]);
            __syncthreads();
            if (s + 2 < nstage) stage_load(slot_c, (s + 2) * BK);
            const float* as = As[slot] + (wt * 32 * FT + lrow) * LD + lh;
            const float* ws = Ws[slot] + (wc * 32 * CT + lrow) * LD + lh;
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                float av[CT], bv[FT];
#pragma unroll
                for (int ic = 0; ic < CT; ++ic) av[ic] = ws[ic * 32 * LD + 2 * kk];
#pragma unroll
                for (int it = 0; it < FT; ++it) bv[it] = as[it * 32 * LD + 2 * kk];
#pragma unroll
                for (int ic = 0; ic < CT; ++ic)
#pragma unroll
                    for (int it = 0; it < FT; ++it) acc[ic][it] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ic], bv[it], acc[ic][it], 0, 0, 0);
            }
        };
        stage_load(std::integral_constant<int, 0>{}, 0);
        if (nstage > 1) stage_load(std::integral_constant<int, 1>{}, BK);
        for (int s = 0; s < nstage; s += 2) {
            step(std::integral_constant<int, 0>{}, s);
            if (s + 1 < nstage) step(std::integral_constant<int, 1>{}, s + 1);
        }
    }

    // register r of lane l: channel (r & 3) + 8 (r >> 2) + 4 (l >> 5), frame l & 31 of the sub-tile
#pragma unroll
    for (int it = 0; it < FT; ++it) {
        const int t = t0 + wt * 32 * FT + it * 32 + (lane & 31);
        if (t >= p.Fout) continue;
        const bool valid = t < len_out;
#pragma unroll
        for (int ic = 0; ic < CT; ++ic)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wc * 32 * CT + ic * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n >= nend) continue;
                const long long o = EPI == W2V_BIAS_CM ? (b * p.N + n) * p.Fout + t : (b * p.Fout + t) * p.N + n;
                float v = 0.f;
                if (valid) {
                    v = acc[ic][it][r] + p.bias[n];
                    if (EPI == W2V_GELU) v = gelu_fast(v);
                    else if (EPI == W2V_SILU) v = act_apply(v, FV_ACT_SILU, 0.f);
                    else if (EPI == W2V_RES) v = p.r[o] + v;
                    else if (EPI == W2V_GELU_RES) v = p.r[o] + gelu_fast(v);
                }
                p.y[o] = v;
            }
    }
}

// One wave per frame: the row (C <= 1024, a multiple of 4) in four float4 per lane; mean, then the variance about it, each a lane's sum
// in index order and a butterfly over the wave.  x == y is allowed.
template <bool GELU>
__global__ __launch_bounds__(256) void w2v_ln_kernel(const float* x, float* y, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     int C, int F, int row0, const W2vRowBlock rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave;
    if (t >= F) return;
    const int bl = blockIdx.z;
    const long long base = ((long long)(row0 + bl) * F + t) * C;
    const int nq = C >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= rows.e[bl].out) {
        for (int q = lane; q < nq; q += 64) reinterpret_cast<float4*>(y + base)[q] = zero4;
        return;
    }
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = lane + 64 * i;
        v[i] = q < nq ? reinterpret_cast<const float4*>(x + base)[q] : zero4;
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    const float mean = s / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (lane + 64 * i < nq) {
            v[i].x -= mean, v[i].y -= mean, v[i].z -= mean, v[i].w -= mean;
            ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
    const float rstd = 1.f / sqrtf(ss / (float)C + kW2vEps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = lane + 64 * i;
        if (q >= nq) continue;
        const float4 g = reinterpret_cast<const float4*>(gamma)[q], bt = reinterpret_cast<const float4*>(beta)[q];
        float4 o = make_float4(fmaf(v[i].x * rstd, g.x, bt.x), fmaf(v[i].y * rstd, g.y, bt.y), fmaf(v[i].z * rstd, g.z, bt.z), fmaf(v[i].w * rstd, g.w, bt.w));
        if (GELU) o = make_float4(gelu_fast(o.x), gelu_fast(o.y), gelu_fast(o.z), gelu_fast(o.w));
        reinterpret_cast<float4*>(y + base)[q] = o;
    }
}

// rows t >= the row's count of (b, F, C), zeroed (the hidden state that holds layer 0's input is written by the positional conv, which
// zeroes them itself; this serves the copies)
__global__ __launch_bounds__(256) void w2v_copy_kernel(const float* __restrict__ x, float* __restrict__ y, long long per_row, int C, int row0,
                                                       const W2vRowBlock rows) {
    const int bl = blockIdx.z;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= per_row) return;
    const long long o = (long long)(row0 + bl) * per_row + i;
    const bool valid = i / C < rows.e[bl].out;
    *reinterpret_cast<float4*>(y + o) = valid ? *reinterpret_cast<const float4*>(x + o) : make_float4(0.f, 0.f, 0.f, 0.f);
}

constexpr int kAttnKeys = 32, kAttnKLd = kW2vHeadDim + 4;

// qkv: (b, F, 3 H), q | k | v; o: (b, F, H).  A workgroup: one row, one head, 128 queries (32 per wave).
__global__ __launch_bounds__(256) void w2v_attn_kernel(const float* __restrict__ qkv, float* __restrict__ o, int H, int F, int row0,
                                                       const W2vRowBlock rows) {
    __shared__ __attribute__((aligned(16))) float Ks[kAttnKeys * kAttnKLd];
    __shared__ __attribute__((aligned(16))) float Vs[kAttnKeys * kW2vHeadDim];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bl = blockIdx.z, head = blockIdx.y;
    const int len = rows.e[bl].out;
    const int q0 = blockIdx.x * 128;
    if (q0 >= len) return;              // block-uniform: nothing past a row's frames is read downstream
    const long long rowbase = (long long)(row0 + bl) * F;
    const int ql = lane & 31, lh = lane >> 5;
    const int q = q0 + wave * 32 + ql;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // the contraction over d runs in the order (s, half): step s pairs d = s (lanes 0-31) with d = 32 + s (lanes 32-63)
    float qr[32];
    {
        const float4* src = reinterpret_cast<const float4*>(qkv + (rowbase + min(q, len - 1)) * 3 * H + head * kW2vHeadDim + lh * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 t4 = q < len ? src[i] : zero4;
            qr[4 * i] = t4.x, qr[4 * i + 1] = t4.y, qr[4 * i + 2] = t4.z, qr[4 * i + 3] = t4.w;
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) o0[r] = 0.f, o1[r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    float4 pk[2], pv[2];
    auto tile_load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, key = k0 + (idx >> 4), c4 = idx & 15;
            pk[i] = zero4, pv[i] = zero4;
            if (key < len) {            // keys at or past the row's count are never loaded
                const float* src = qkv + (rowbase + key) * 3 * H + H + head * kW2vHeadDim + c4 * 4;
                pk[i] = *reinterpret_cast<const float4*>(src);
                pv[i] = *reinterpret_cast<const float4*>(src + H);
            }
        }
    };
    tile_load(0);
    for (int k0 = 0; k0 < len; k0 += kAttnKeys) {
        __syncthreads();                // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, key = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<float4*>(&Ks[key * kAttnKLd + c4 * 4]) = pk[i];
            *reinterpret_cast<float4*>(&Vs[key * kW2vHeadDim + c4 * 4]) = pv[i];
        }
        __syncthreads();
        if (k0 + kAttnKeys < len) tile_load(k0 + kAttnKeys);

        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
        const float* kp = Ks + ql * kAttnKLd + lh * 32;        // this lane's key of the tile is ql
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * i);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qr[4 * i], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qr[4 * i + 1], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qr[4 * i + 2], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qr[4 * i + 3], sacc, 0, 0, 0);
        }
        // register r of lane l: key (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, query l & 31; the query's other 16 keys are in lane l ^ 32
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sacc[r] *= 0.125f;          // head_dim ** -0.5, exact
            if (k0 + (r & 3) + 8 * (r >> 2) + 4 * lh < len) mt = fmaxf(mt, sacc[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);       // finite: the tile holds at least one key of the row
        const float alpha = expf(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool kv = k0 + (r & 3) + 8 * (r >> 2) + 4 * lh < len;
            sacc[r] = kv ? expf(sacc[r] - m_new) : 0.f;
            psum += sacc[r];
        }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) o0[r] *= alpha, o1[r] *= alpha;
        // O' (d x queries) += V' (d x keys) P (keys x queries): step kk takes key (kk & 3) + 8 (kk >> 2) + 4 (l >> 5), which is where P's
        // register kk holds it
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float* vp = Vs + ((kk & 3) + 8 * (kk >> 2) + 4 * lh) * kW2vHeadDim + ql;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], sacc[kk], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32], sacc[kk], o1, 0, 0, 0);
        }
    }
    if (q >= len) return;
    const float inv = 1.f / l_run;
    float* dst = o + (rowbase + q) * H + head * kW2vHeadDim + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(dst + 8 * g) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
        *reinterpret_cast<float4*>(dst + 32 + 8 * g) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
}

// One product of the network on the host side
struct W2vLinear {
    int Cg = 0, taps = 1, stride = 1, pad = 0, N = 0, Ng = 0;
    std::vector<float> w, b;
    float* d_w = nullptr;
    float* d_b = nullptr;
};
struct W2vNorm {
    int C = 0;
    std::vector<float> g, b;
    float* d_g = nullptr;
    float* d_b = nullptr;
};

// torch (N, Cg, taps) -> (N, taps, Cg)
std::vector<float> tap_major(const std::vector<float>& w, int N, int Cg, int taps) {
    std::vector<float> out(w.size());
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < Cg; ++c)
            for (int j = 0; j < taps; ++j) out[((size_t)n * taps + j) * Cg + c] = w[((size_t)n * Cg + c) * taps + j];
    return out;
}

struct W2vTensor {
    std::vector<float> data;
};

std::string w2v_shape_str(const int64_t* shape, int ndim) {
    std::string s = "(";
    for (int i = 0; i < ndim; ++i) s += (i ? ", " : "") + std::to_string((long long)shape[i]);
    return s + ")";
}

long long conv_out_frames(long long len, int k, int s) { return len < k ? 0 : (len - k) / s + 1; }

const char* kPosG = "model.encoder.pos_conv_embed.conv.parametrizations.weight.original0";
const char* kPosV = "model.encoder.pos_conv_embed.conv.parametrizations.weight.original1";
const char* kPosGLegacy = "model.encoder.pos_conv_embed.conv.weight_g";
const char* kPosVLegacy = "model.encoder.pos_conv_embed.conv.weight_v";

}  // namespace
}  // namespace fv

using namespace fv;

struct fv_w2v {
    fv_w2v_config cfg{};
    std::map<std::string, std::vector<int64_t>> expect;
    std::vector<std::string> order;
    std::map<std::string, W2vTensor> loaded;
    bool finalized = false;
    std::vector<W2vLinear> conv;
    std::vector<W2vNorm> conv_ln;
    W2vNorm proj_ln, enc_ln;
    W2vLinear proj, pos;
    struct Layer {
        W2vNorm ln, final_ln;
        W2vLinear qkv, out, ff1, ff2;
    };
    std::vector<Layer> layers;
    W2vLinear post[3];
    std::vector<float*> owned;
    ~fv_w2v() {
        for (float* d : owned) (void)hipFree(d);
    }
};

namespace {

fv_status w2v_upload(fv_w2v* w, std::vector<float>& host, float** dev) {
    FV_HIP_CHECK(hipMalloc(dev, std::max<size_t>(host.size(), 4) * 4));
    w->owned.push_back(*dev);
    FV_HIP_CHECK(hipMemcpy(*dev, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    host = std::vector<float>();
    return FV_OK;
}
fv_status w2v_upload(fv_w2v* w, W2vLinear& l) {
    if (const fv_status st = w2v_upload(w, l.w, &l.d_w)) return st;
    return w2v_upload(w, l.b, &l.d_b);
}
fv_status w2v_upload(fv_w2v* w, W2vNorm& n) {
    if (const fv_status st = w2v_upload(w, n.g, &n.d_g)) return st;
    return w2v_upload(w, n.b, &n.d_b);
}

// frames of every stage for `samples` samples: f[l + 1] after conv layer l; the backbone's count is f[n_conv], post's f[n_conv + 1]
void w2v_stage_frames(const fv_w2v_config& c, long long samples, long long* f) {
    f[0] = samples;
    for (int l = 0; l < c.n_conv; ++l) f[l + 1] = conv_out_frames(f[l], c.conv_kernel[l], c.conv_stride[l]);
    const long long F = f[c.n_conv];
    f[c.n_conv + 1] = F > 0 ? (F - 1) / 2 + 1 : 0;
}

fv_status w2v_check_shape(const char* fn, const fv_w2v* w, int32_t batch, int64_t T) {
    if (!w) {
        set_error("%s: null encoder", fn);
        return FV_ERR_INVALID;
    }
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kW2vMaxSamples || (long long)batch * T > kW2vMaxSamples) {
        set_error("%s: T = %lld must be >= 0 and batch * T at most 2^30 samples", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// The workspace, in floats: two feature-extractor buffers, then h, the LayerNorm's output, q | k | v (the positional conv's output and
// the post stack's two intermediates live there too), the attention's output and the FFN's intermediate
struct W2vPlan {
    long long F[kW2vMaxConv + 2];
    size_t feat = 0, h = 0, qkv = 0, ffn = 0, total = 0;
};
W2vPlan w2v_plan(const fv_w2v_config& c, int batch, long long T) {
    W2vPlan pl{};
    w2v_stage_frames(c, T, pl.F);
    const size_t B = (size_t)batch, F = (size_t)pl.F[c.n_conv];
    for (int l = 0; l < c.n_conv; ++l) pl.feat = std::max(pl.feat, B * (size_t)pl.F[l + 1] * (size_t)c.conv_dim[l]);
    pl.h = B * F * (size_t)c.hidden;
    pl.qkv = std::max(3 * pl.h, 2 * B * F * (size_t)c.post_channels);
    pl.ffn = B * F * (size_t)c.intermediate;
    pl.total = 2 * pl.feat + 3 * pl.h + pl.qkv + pl.ffn;
    return pl;
}

template <int EPI>
void w2v_gemm(const W2vLinear& l, const float* a, long long a_bstride, int a_rstride, float* y, const float* r, int Fout, int row0, int nrows,
              const W2vRowBlock& rows, hipStream_t s) {
    W2vGemmParams p{};
    p.a = a, p.a_bstride = a_bstride, p.a_rstride = a_rstride;
    p.Cg = l.Cg, p.stride = l.stride, p.pad = l.pad, p.K = l.taps * l.Cg;
    p.w = l.d_w, p.bias = l.d_b, p.N = l.N, p.Ng = l.Ng;
    p.y = y, p.r = r, p.Fout = Fout, p.row0 = row0;
    const int groups = l.N / l.Ng;
    // the largest tile that still gives every compute unit a workgroup, else the smallest; the sums do not depend on it
    auto blocks = [&](int ft, int ct) { return (long long)((Fout + 64 * ft - 1) / (64 * ft)) * groups * ((l.Ng + 64 * ct - 1) / (64 * ct)) * nrows; };
    auto go = [&](auto kernel, int ft, int ct) {
        const dim3 grid((unsigned)((Fout + 64 * ft - 1) / (64 * ft)), (unsigned)(groups * ((l.Ng + 64 * ct - 1) / (64 * ct))), (unsigned)nrows);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p, rows);
    };
    const long long fill = num_cus();
    const int tile = blocks(2, 2) >= fill ? 0 : blocks(1, 2) >= fill ? 1 : 2;
    if (l.Cg % 4 == 0 && a_rstride % 4 == 0 && a_bstride % 4 == 0) {        // 16-byte loads: all but the FIR on the wave
        if (tile == 0) go(w2v_gemm_kernel<EPI, 2, 2, 16, true>, 2, 2);
        else if (tile == 1) go(w2v_gemm_kernel<EPI, 1, 2, 32, true>, 1, 2);
        else go(w2v_gemm_kernel<EPI, 1, 1, 32, true>, 1, 1);
    } else {
        if (tile == 0) go(w2v_gemm_kernel<EPI, 2, 2, 16, false>, 2, 2);
        else if (tile == 1) go(w2v_gemm_kernel<EPI, 1, 2, 32, false>, 1, 2);
        else go(w2v_gemm_kernel<EPI, 1, 1, 32, false>, 1, 1);
    }
}

template <bool GELU>
void w2v_ln(const W2vNorm& n, const float* x, float* y, int F, int row0, int nrows, const W2vRowBlock& rows, hipStream_t s) {
    hipLaunchKernelGGL(w2v_ln_kernel<GELU>, dim3((unsigned)((F + 3) / 4), 1, (unsigned)nrows), dim3(256), 0, s, x, y, n.d_g, n.d_b, n.C, F, row0, rows);
}

}  // namespace

extern "C" {

FV_API fv_status fv_w2v_create(const fv_w2v_config* cfg, fv_w2v** out) {
    const char* fn = "fv_w2v_create";
    if (!out || !cfg) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    auto range = [&](const std::string& name, int v, int lo, int hi) {
        if (v >= lo && v <= hi) return true;
        set_error("%s: %s = %d must lie in [%d, %d]", fn, name.c_str(), v, lo, hi);
        return false;
    };
    auto quad = [&](const std::string& name, int v) {
        if (v % 4 == 0) return true;
        set_error("%s: %s = %d must be a multiple of 4 (rows move as 16-byte quads)", fn, name.c_str(), v);
        return false;
    };
    if (!range("hidden", cfg->hidden, 1, kW2vMaxLn) || !quad("hidden", cfg->hidden) || !range("layers", cfg->layers, 1, kW2vMaxLayers) ||
        !range("heads", cfg->heads, 1, kW2vMaxLn) || !range("intermediate", cfg->intermediate, 1, kW2vMaxWide) ||
        !quad("intermediate", cfg->intermediate) || !range("n_conv", cfg->n_conv, 1, kW2vMaxConv))
        return FV_ERR_INVALID;
    if (cfg->hidden % cfg->heads) {
        set_error("%s: heads = %d must divide hidden = %d", fn, cfg->heads, cfg->hidden);
        return FV_ERR_INVALID;
    }
    if (cfg->hidden / cfg->heads != kW2vHeadDim) {
        set_error("%s: heads = %d gives a head size hidden / heads = %d; the attention kernel is built for %d only", fn, cfg->heads,
                  cfg->hidden / cfg->heads, kW2vHeadDim);
        return FV_ERR_UNSUPPORTED;
    }
    for (int l = 0; l < cfg->n_conv; ++l) {
        const std::string i = "[" + std::to_string(l) + "]";
        if (!range("conv_dim" + i, cfg->conv_dim[l], 1, kW2vMaxLn) || !quad("conv_dim" + i, cfg->conv_dim[l]) ||
            !range("conv_kernel" + i, cfg->conv_kernel[l], 1, l ? 64 : 32) || !range("conv_stride" + i, cfg->conv_stride[l], 1, 64))
            return FV_ERR_INVALID;
    }
    if (!range("pos_conv_kernel", cfg->pos_conv_kernel, 1, 256) || !range("pos_conv_groups", cfg->pos_conv_groups, 1, cfg->hidden)) return FV_ERR_INVALID;
    if (cfg->hidden % cfg->pos_conv_groups) {
        set_error("%s: pos_conv_groups = %d must divide hidden = %d", fn, cfg->pos_conv_groups, cfg->hidden);
        return FV_ERR_INVALID;
    }
    if (!range("post_channels", cfg->post_channels, 0, kW2vMaxWide) || !quad("post_channels", cfg->post_channels)) return FV_ERR_INVALID;

    std::unique_ptr<fv_w2v> w(new fv_w2v());
    w->cfg = *cfg;
    const int H = cfg->hidden, I = cfg->intermediate, O = cfg->post_channels;
    auto want = [&](const std::string& key, std::vector<int64_t> shape) {
        w->order.push_back(key);
        w->expect[key] = std::move(shape);
    };
    auto want_wb = [&](const std::string& pfx, std::vector<int64_t> wshape) {
        const int64_t rows = wshape[0];
        want(pfx + ".weight", std::move(wshape));
        want(pfx + ".bias", {rows});
    };
    for (int l = 0; l < cfg->n_conv; ++l) {
        const std::string pfx = "model.feature_extractor.conv_layers." + std::to_string(l);
        want_wb(pfx + ".conv", {cfg->conv_dim[l], l ? cfg->conv_dim[l - 1] : 1, cfg->conv_kernel[l]});
        want_wb(pfx + ".layer_norm", {cfg->conv_dim[l]});
    }
    const int Cl = cfg->conv_dim[cfg->n_conv - 1];
    want_wb("model.feature_projection.layer_norm", {Cl});
    want_wb("model.feature_projection.projection", {H, Cl});
    want("model.encoder.pos_conv_embed.conv.bias", {H});
    want(kPosG, {1, 1, cfg->pos_conv_kernel});
    want(kPosV, {H, H / cfg->pos_conv_groups, cfg->pos_conv_kernel});
    want_wb("model.encoder.layer_norm", {H});
    for (int i = 0; i < cfg->layers; ++i) {
        const std::string pfx = "model.encoder.layers." + std::to_string(i);
        for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) want_wb(pfx + ".attention." + n, {H, H});
        want_wb(pfx + ".layer_norm", {H});
        want_wb(pfx + ".feed_forward.intermediate_dense", {I, H});
        want_wb(pfx + ".feed_forward.output_dense", {H, I});
        want_wb(pfx + ".final_layer_norm", {H});
    }
    if (O) {
        want_wb("post.0", {O, H, 3});
        want_wb("post.2", {O, O, 3});
        want_wb("post.4", {O, O, 1});
    }
    *out = w.release();
    return FV_OK;
}

FV_API void fv_w2v_destroy(fv_w2v* w) { delete w; }

FV_API fv_status fv_w2v_load_weight(fv_w2v* w, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    const char* fn = "fv_w2v_load_weight";
    if (!w || !name || !host || ndim < 0 || (ndim > 0 && !shape)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (w->finalized) {
        set_error("%s: '%s' arrives after fv_w2v_finalize", fn, name);
        return FV_ERR_STATE;
    }
    if (!strcmp(name, "model.masked_spec_embed")) return FV_OK;        // SpecAugment's mask vector: no eval arithmetic
    const char* key = !strcmp(name, kPosGLegacy) ? kPosG : !strcmp(name, kPosVLegacy) ? kPosV : name;
    const auto it = w->expect.find(key);
    if (it == w->expect.end()) {
        set_error("%s: unknown key '%s'", fn, name);
        return FV_ERR_INVALID;
    }
    const std::vector<int64_t>& want = it->second;
    if ((size_t)ndim != want.size() || !std::equal(want.begin(), want.end(), shape)) {
        set_error("%s: '%s' has shape %s, expected %s", fn, name, w2v_shape_str(shape, ndim).c_str(), w2v_shape_str(want.data(), (int)want.size()).c_str());
        return FV_ERR_SHAPE;
    }
    size_t n = 1;
    for (int64_t v : want) n *= (size_t)v;
    w->loaded[key].data.assign(host, host + n);
    return FV_OK;
}

FV_API fv_status fv_w2v_finalize(fv_w2v* w) {
    const char* fn = "fv_w2v_finalize";
    if (!w) {
        set_error("%s: null encoder", fn);
        return FV_ERR_INVALID;
    }
    if (w->finalized) {
        set_error("%s: already finalized", fn);
        return FV_ERR_STATE;
    }
    for (const std::string& key : w->order)
        if (!w->loaded.count(key)) {
            set_error("%s: missing weight '%s'", fn, key.c_str());
            return FV_ERR_MISSING_WEIGHT;
        }
    const fv_w2v_config& c = w->cfg;
    const int H = c.hidden, I = c.intermediate, O = c.post_channels;
    auto data = [&](const std::string& key) -> const std::vector<float>& { return w->loaded[key].data; };
    auto linear = [&](W2vLinear& l, const std::string& pfx, int N, int Cg, int taps, int stride, int pad) {
        l.N = l.Ng = N, l.Cg = Cg, l.taps = taps, l.stride = stride, l.pad = pad;
        l.w = taps > 1 ? tap_major(data(pfx + ".weight"), N, Cg, taps) : data(pfx + ".weight");
        l.b = data(pfx + ".bias");
    };
    auto norm = [&](W2vNorm& n, const std::string& pfx, int C) { n.C = C, n.g = data(pfx + ".weight"), n.b = data(pfx + ".bias"); };
    w->conv.resize(c.n_conv), w->conv_ln.resize(c.n_conv);
    for (int l = 0; l < c.n_conv; ++l) {
        const std::string pfx = "model.feature_extractor.conv_layers." + std::to_string(l);
        linear(w->conv[l], pfx + ".conv", c.conv_dim[l], l ? c.conv_dim[l - 1] : 1, c.conv_kernel[l], c.conv_stride[l], 0);
        norm(w->conv_ln[l], pfx + ".layer_norm", c.conv_dim[l]);
    }
    const int Cl = c.conv_dim[c.n_conv - 1];
    norm(w->proj_ln, "model.feature_projection.layer_norm", Cl);
    linear(w->proj, "model.feature_projection.projection", H, Cl, 1, 1, 0);
    {
        // weight norm over dim 2: w[:, :, j] = g[j] v[:, :, j] / |v[:, :, j]|, in fp64, rounded once
        const int k = c.pos_conv_kernel, Cg = H / c.pos_conv_groups;
        const std::vector<float>&g = data(kPosG), &v = data(kPosV);
        std::vector<float> folded(v.size());
        for (int j = 0; j < k; ++j) {
            double ss = 0.0;
            for (size_t i = 0; i < (size_t)H * Cg; ++i) ss += (double)v[i * k + j] * (double)v[i * k + j];
            const double scale = (double)g[j] / std::sqrt(ss);
            for (size_t i = 0; i < (size_t)H * Cg; ++i) folded[i * k + j] = (float)((double)v[i * k + j] * scale);
        }
        W2vLinear& l = w->pos;
        l.N = H, l.Ng = Cg, l.Cg = Cg, l.taps = k, l.stride = 1, l.pad = k / 2;
        l.w = tap_major(folded, H, Cg, k);
        l.b = data("model.encoder.pos_conv_embed.conv.bias");
    }
    norm(w->enc_ln, "model.encoder.layer_norm", H);
    w->layers.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        const std::string pfx = "model.encoder.layers." + std::to_string(i);
        fv_w2v::Layer& L = w->layers[i];
        norm(L.ln, pfx + ".layer_norm", H);
        norm(L.final_ln, pfx + ".final_layer_norm", H);
        W2vLinear& q = L.qkv;
        q.N = q.Ng = 3 * H, q.Cg = H;
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
            const std::vector<float>&pw = data(pfx + ".attention." + n + ".weight"), &pb = data(pfx + ".attention." + n + ".bias");
            q.w.insert(q.w.end(), pw.begin(), pw.end());
            q.b.insert(q.b.end(), pb.begin(), pb.end());
        }
        linear(L.out, pfx + ".attention.out_proj", H, H, 1, 1, 0);
        linear(L.ff1, pfx + ".feed_forward.intermediate_dense", I, H, 1, 1, 0);
        linear(L.ff2, pfx + ".feed_forward.output_dense", H, I, 1, 1, 0);
    }
    if (O) {
        linear(w->post[0], "post.0", O, H, 3, 1, 1);
        linear(w->post[1], "post.2", O, O, 3, 2, 1);
        linear(w->post[2], "post.4", O, O, 1, 1, 0);
    }
    // everything is folded: upload
    fv_status st = FV_OK;
    for (int l = 0; l < c.n_conv && !st; ++l) {
        st = w2v_upload(w, w->conv[l]);
        if (!st) st = w2v_upload(w, w->conv_ln[l]);
    }
    if (!st) st = w2v_upload(w, w->proj_ln);
    if (!st) st = w2v_upload(w, w->proj);
    if (!st) st = w2v_upload(w, w->pos);
    if (!st) st = w2v_upload(w, w->enc_ln);
    for (int i = 0; i < c.layers && !st; ++i) {
        fv_w2v::Layer& L = w->layers[i];
        st = w2v_upload(w, L.ln);
        if (!st) st = w2v_upload(w, L.final_ln);
        if (!st) st = w2v_upload(w, L.qkv);
        if (!st) st = w2v_upload(w, L.out);
        if (!st) st = w2v_upload(w, L.ff1);
        if (!st) st = w2v_upload(w, L.ff2);
    }
    for (int i = 0; i < 3 && O && !st; ++i) st = w2v_upload(w, w->post[i]);
    if (st) return st;
    w->loaded.clear();
    w->finalized = true;
    return FV_OK;
}

FV_API int64_t fv_w2v_frames(const fv_w2v* w, int64_t samples, int32_t stage) {
    if (!w || samples < 0 || stage < 0 || stage > 1) return -1;
    long long f[kW2vMaxConv + 2];
    w2v_stage_frames(w->cfg, samples, f);
    return f[w->cfg.n_conv + stage];
}

FV_API size_t fv_w2v_workspace_bytes(const fv_w2v* w, int32_t batch, int64_t T) {
    if (w2v_check_shape("fv_w2v_workspace_bytes", w, batch, T)) return 0;
    const W2vPlan pl = w2v_plan(w->cfg, batch, T);
    if (!batch || !pl.F[w->cfg.n_conv]) return 0;
    return pl.total * sizeof(float);
}

FV_API fv_status fv_w2v_forward(fv_w2v* w, const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_out,
                                float* d_hidden_states, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fv_w2v_forward";
    if (const fv_status st = w2v_check_shape(fn, w, batch, T)) return st;
    if (!w->finalized) {
        set_error("%s: the encoder has not been finalized (fv_w2v_finalize)", fn);
        return FV_ERR_STATE;
    }
    const fv_w2v_config& c = w->cfg;
    const W2vPlan pl = w2v_plan(c, batch, T);
    const long long F = pl.F[c.n_conv], F2 = pl.F[c.n_conv + 1];
    if (batch == 0 || F == 0) return FV_OK;
    if (!d_x || !d_out) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : "d_out");
        return FV_ERR_INVALID;
    }
    const size_t need = pl.total * sizeof(float);
    if (workspace_bytes < need || !d_workspace) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_w2v_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, need, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (((uintptr_t)d_workspace | (uintptr_t)d_out | (uintptr_t)d_hidden_states) % 16) {
        set_error("%s: d_workspace, d_out and d_hidden_states must be 16-byte aligned (rows move as 16-byte quads)", fn);
        return FV_ERR_INVALID;
    }
    for (int b = 0; host_lengths && b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > T) {
            set_error("%s: host_lengths[%d] = %d lies outside [0, T = %lld]", fn, b, host_lengths[b], (long long)T);
            return FV_ERR_INVALID;
        }
    // everything is validated: enqueue

    const int H = c.hidden, O = c.post_channels, Fi = (int)F;
    float* feat0 = (float*)d_workspace;
    float* feat1 = feat0 + pl.feat;
    float* h = feat1 + pl.feat;
    float* xn = h + pl.h;
    float* at = xn + pl.h;
    float* qkv = at + pl.h;
    float* ffn = qkv + pl.qkv;
    hipStream_t s = (hipStream_t)stream;
    const size_t hs_plane = (size_t)batch * F * H;

    auto block = [&](const W2vSampleBlock& samples, int row0, int nrows) -> fv_status {
        // the rows' frame counts after every stage
        long long fr[kW2vRows][kW2vMaxConv + 2];
        for (int i = 0; i < nrows; ++i) w2v_stage_frames(c, samples.e[i], fr[i]);
        auto lens = [&](int in_stage, int out_stage) {
            W2vRowBlock t{};
            for (int i = 0; i < nrows; ++i) t.e[i].in = (int)fr[i][in_stage], t.e[i].out = (int)fr[i][out_stage];
            return t;
        };
        const int SF = c.n_conv, SP = c.n_conv + 1;
        // feature extractor: the wave is (b, T, 1)
        const float* cur = d_x;
        long long cur_bstride = T;
        float* bufs[2] = {feat0, feat1};
        for (int l = 0; l < c.n_conv; ++l) {
            const W2vRowBlock t = lens(l, l + 1);
            const int Fl = (int)pl.F[l + 1], Cin = l ? c.conv_dim[l - 1] : 1;
            float* y = bufs[l & 1];
            w2v_gemm<W2V_BIAS>(w->conv[l], cur, cur_bstride, Cin, y, nullptr, Fl, row0, nrows, t, s);
            w2v_ln<true>(w->conv_ln[l], y, y, Fl, row0, nrows, t, s);
            cur = y, cur_bstride = (long long)Fl * c.conv_dim[l];
        }
        const W2vRowBlock tf = lens(SF, SF);
        const int Cl = c.conv_dim[c.n_conv - 1];
        float* other = bufs[c.n_conv & 1];          // the feature buffer that `cur` is not
        w2v_ln<false>(w->proj_ln, cur, other, Fi, row0, nrows, tf, s);
        w2v_gemm<W2V_BIAS>(w->proj, other, (long long)Fi * Cl, Cl, xn, nullptr, Fi, row0, nrows, tf, s);
        // h = xn + GELU(pos_conv(xn)); with hidden states wanted it is written there first
        const long long hb = (long long)Fi * H;
        w2v_gemm<W2V_GELU_RES>(w->pos, xn, hb, H, h, xn, Fi, row0, nrows, tf, s);
        const dim3 cgrid((unsigned)((hb / 4 + 255) / 256), 1, (unsigned)nrows);
        if (d_hidden_states) hipLaunchKernelGGL(w2v_copy_kernel, cgrid, dim3(256), 0, s, h, d_hidden_states, hb, H, row0, tf);
        for (int i = 0; i < c.layers; ++i) {
            const fv_w2v::Layer& L = w->layers[i];
            w2v_ln<false>(L.ln, h, xn, Fi, row0, nrows, tf, s);
            w2v_gemm<W2V_BIAS>(L.qkv, xn, hb, H, qkv, nullptr, Fi, row0, nrows, tf, s);
            hipLaunchKernelGGL(w2v_attn_kernel, dim3((unsigned)((Fi + 127) / 128), (unsigned)c.heads, (unsigned)nrows), dim3(256), 0, s, qkv, at, H, Fi,
                               row0, tf);
            w2v_gemm<W2V_RES>(L.out, at, hb, H, h, h, Fi, row0, nrows, tf, s);
            w2v_ln<false>(L.final_ln, h, xn, Fi, row0, nrows, tf, s);
            w2v_gemm<W2V_GELU>(L.ff1, xn, hb, H, ffn, nullptr, Fi, row0, nrows, tf, s);
            w2v_gemm<W2V_RES>(L.ff2, ffn, (long long)Fi * c.intermediate, c.intermediate, h, h, Fi, row0, nrows, tf, s);
            if (d_hidden_states) hipLaunchKernelGGL(w2v_copy_kernel, cgrid, dim3(256), 0, s, h, d_hidden_states + (size_t)(i + 1) * hs_plane, hb, H, row0, tf);
        }
        if (!O) {
            w2v_ln<false>(w->enc_ln, h, d_out, Fi, row0, nrows, tf, s);
            return FV_OK;
        }
        w2v_ln<false>(w->enc_ln, h, xn, Fi, row0, nrows, tf, s);
        float* p0 = qkv;
        float* p1 = qkv + (size_t)batch * F * O;
        w2v_gemm<W2V_SILU>(w->post[0], xn, hb, H, p0, nullptr, Fi, row0, nrows, tf, s);
        w2v_gemm<W2V_SILU>(w->post[1], p0, (long long)Fi * O, O, p1, nullptr, (int)F2, row0, nrows, lens(SF, SP), s);
        w2v_gemm<W2V_BIAS_CM>(w->post[2], p1, F2 * O, O, d_out, nullptr, (int)F2, row0, nrows, lens(SP, SP), s);
        return FV_OK;
    };
    const fv_status st = for_each_launch_table<W2vSampleBlock>(batch, [&](int b) { return host_lengths ? host_lengths[b] : (int)T; }, block);
    if (st == FV_OK) set_last_kernel("w2v_gemm_kernel");
    return st;
}

}  // extern "C"
