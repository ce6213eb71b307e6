// The two critics of the reference's GAN (include/fishvoc.h fv_disc_*): modules/discriminators/mpd.py (MultiPeriodDiscriminator) and
// modules/discriminators/mrd.py (MultiResolutionDiscriminator), forward only, and the sums behind models/gan.py:149 / 155 / 204.
// Activations are CHANNEL LAST, (row, H, W, C): MPD's H is the folded time ceil(L / p) and W the period, MRD's H is the frequency bin and
// W the frame.  Every conv of both is one implicit GEMM:
//   disc_conv   y[h][w][n] = epi(sum_{kh, kw, c} in[h sh - ph + kh][w sw - pw + kw][c] wt[n][kh][kw][c] + bias[n]),  0 outside the row's (H, W)
//               M = the (h, w) positions of the batch's extent, flattened; K = KH KW C in the order (kh, kw, c).  The input is addressed as
//               h hs + w ws + c with free strides, which makes two more things the same product: MPD's fold (the wave read as (H, p, 1),
//               hs = p, ws = 1, zeros at and past the row's length) and MRD's DFT (frames x n_fft windows that overlap, hs = hop, C = n_fft).
//   disc_pad    mrd.py:53-60, the reflect padding at the row's own ends
//   disc_mag    mrd.py:70-71, sqrt(re^2 + im^2) with no epsilon, (frame, re | im) -> (bin, frame, 1)
//   disc_sums   gan.py:149 / 155 / 204: per row and feature map, sum |real - fake|, sum (1 - fake)^2, sum fake^2, sum (real - 1)^2 over the
//               row's own extent, fp64 partials per tile of 4096 elements in a fixed order, then a finish launch; no float atomics
// The GEMM is w2v_gemm_kernel's (w2v.hip) with a 2-D window: exact fp32 on v_mfma_f32_32x32x2_f32, K staged through LDS with the next
// stage's loads in flight, every load unconditional on an address clamped into the row, the tile chosen by the grid alone.  Layers of at
// most 32 output channels (all of MRD, every conv_post) put the four waves along M: 128 or 256 positions x 32 channels.
// Ragged rows: each layer's per-row (H, W) travel by value (LaunchTable).  Nothing at or past a row's extent is read; feature maps and
// scores hold exact zeros there.  An element's sum is one accumulator chain over k ascending, then the bias: fixed by the layer's shape and
// the row's own extent, so a row has the same bits alone, in any batch, in any order and padded to any T.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>

#include "conv_mfma_impl.h"

namespace fv {
namespace {

constexpr int kDiscRows = 64;                       // rows per launch: their extents are a LaunchTable
constexpr int kDiscMaxSub = 8, kDiscMaxChannels = 8, kDiscMaxLayers = kDiscMaxChannels;     // layers of a sub-discriminator, conv_post included
constexpr int kDiscMaxWidth = 1024, kDiscMaxPeriod = 4096, kDiscMaxFft = 4096, kDiscMaxKernel = 15, kDiscMaxStride = 16;
constexpr long long kDiscMaxSamples = 1LL << 26;
constexpr int kDiscSumTile = 4096, kDiscSumPer = kDiscSumTile / 256;

struct DiscExt {
    int hin, win, hout, wout;       // the row's own extents before and after the launch's layer
    int limit;                      // input offsets h hs + w ws + c at or past it read as zero (the fold's row length)
};
using DiscRowBlock = LaunchTable<DiscExt, kDiscRows>;
struct DiscHW {
    int h, w;
};
using DiscHWBlock = LaunchTable<DiscHW, kDiscRows>;
struct DiscLen {
    int len, frames;
};
using DiscLenBlock = LaunchTable<DiscLen, kDiscRows>;

enum DiscEpi : int { DISC_BIAS = 0, DISC_SILU = 1 };

struct DiscConvParams {
    const float* a;                 // input: element (b, h, w, c) at b * a_bstride + h * hs + w * ws + c
    long long a_bstride;
    int hs, ws;
    int Cin, KW, sh, sw, ph, pw, K; // K = KH * KW * Cin
    const float* w;                 // (N, KH, KW, Cin)
    const float* bias;              // (N)
    int N;
    float* y;                       // (b, Hout, Wout, N)
    int Hout, Wout, row0;           // the batch's extent
};

// Four waves, WC of them along the channels and 4 / WC along the positions, each with FT x CT accumulators of 32 positions x 32 channels.
// Staging, pipeline and clamped loads are w2v_gemm_kernel's; a position m = h Wout + w of the batch's extent is split once, before the
// K loop, and a k of the stage once per stage.  VEC: 16-byte loads, four k at a time, for layers whose channel count and strides are
// multiples of four: all but the single-input-channel first layers and a DFT whose hop is not one.
template <int EPI, int FT, int CT, int WC, int BK, bool VEC>
__global__ __launch_bounds__(256) void disc_conv_kernel(const DiscConvParams p, const DiscRowBlock rows) {
    constexpr int WM = 4 / WC, FB = 32 * FT * WM, CB = 32 * CT * WC, LD = BK + 1;
    constexpr int KV = VEC ? 4 : 1, KT = BK / KV, RP = 256 / KT, NA = FB / RP, NW = CB >= RP ? CB / RP : 1;
    static_assert(NA >= 1, "a pass of the staging covers at most the position tile");
    using vec_t = std::conditional_t<VEC, float4, float>;
    __shared__ float As[2][FB * LD];
    __shared__ float Ws[2][CB * LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wt = wave % WM, wc = wave / WM;
    const int bl = blockIdx.z;
    const long long b = p.row0 + bl;
    const DiscExt e = rows.e[bl];
    const long long M = (long long)p.Hout * p.Wout;
    const long long t0 = (long long)blockIdx.x * FB;
    if (t0 >= M) return;
    const int n0 = blockIdx.y * CB;
    const int nend = min(p.N, n0 + CB);

    f32x16 acc[CT][FT];       // [channel sub-tile][position sub-tile]
#pragma unroll
    for (int ic = 0; ic < CT; ++ic)
#pragma unroll
        for (int it = 0; it < FT; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ic][it][r] = 0.f;

    if (t0 / p.Wout < e.hout) {         // the tile holds a position of the row; the row holds at least one input element
        const float* __restrict__ ab = p.a + b * p.a_bstride;
        const int sk = (tid % KT) * KV, sr = tid / KT;
        int ih0[NA], iw0[NA];           // the window's origin; INT_MIN / 2 where the position lies outside the row's output
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const long long m = t0 + sr + RP * i;
            const int oh = (int)(m / p.Wout), ow = (int)(m - (long long)oh * p.Wout);
            const bool mv = oh < e.hout && ow < e.wout;
            ih0[i] = mv ? oh * p.sh - p.ph : INT_MIN / 2;
            iw0[i] = ow * p.sw - p.pw;
        }
        vec_t pa[2][NA], pw[2][NW];
        auto stage_load = [&](auto slot_c, int k0) {
            constexpr int slot = decltype(slot_c)::value;
            const int k = k0 + sk;
            const bool kin = k < p.K;                       // VEC: K is a multiple of 4, so the four stand or fall together
            const int kc = min(k, p.K - KV);
            const int j = kc / p.Cin, c = kc - j * p.Cin;
            const int kh = j / p.KW, kw = j - kh * p.KW;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int ih = ih0[i] + kh, iw = iw0[i] + kw;
                int off = min(max(ih, 0), e.hin - 1) * p.hs + min(max(iw, 0), e.win - 1) * p.ws + c;
                const bool ok = kin && ih >= 0 && ih < e.hin && iw >= 0 && iw < e.win && off < e.limit;
                if constexpr (!VEC) off = min(off, e.limit - 1);
                const vec_t v = *reinterpret_cast<const vec_t*>(ab + off);
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
            for (int i = 0; i < NW; ++i)
                if (CB >= RP || sr < CB) lds_put(&Ws[slot][(sr + RP * i) * LD + sk], pw[slot][i]);
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

    // register r of lane l: channel (r & 3) + 8 (r >> 2) + 4 (l >> 5), position l & 31 of the sub-tile
    const bool quads = (p.N & 3) == 0;      // then a group of four channels lies inside N or outside it, and its store is 16-byte aligned
#pragma unroll
    for (int it = 0; it < FT; ++it) {
        const long long m = t0 + wt * 32 * FT + it * 32 + (lane & 31);
        if (m >= M) continue;
        const int oh = (int)(m / p.Wout), ow = (int)(m - (long long)oh * p.Wout);
        const bool valid = oh < e.hout && ow < e.wout;
        float* yrow = p.y + (b * M + m) * p.N;
#pragma unroll
        for (int ic = 0; ic < CT; ++ic)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wc * 32 * CT + ic * 32 + 8 * g + 4 * (lane >> 5);
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = 0.f;
                    if (valid && n + q < nend) {
                        v[q] = acc[ic][it][4 * g + q] + p.bias[n + q];
                        if (EPI == DISC_SILU) v[q] = act_apply(v[q], FV_ACT_SILU, 0.f);
                    }
                }
                if (quads) {
                    if (n < nend) *reinterpret_cast<float4*>(yrow + n) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (n + q < nend) yrow[n + q] = v[q];
                }
            }
    }
}

// mrd.py:53-60: xp[i] = x[reflect(i - left)] for i < len + left + right, at the row's own ends (len > right >= left).  Nothing past the
// row's padded length is written: the DFT reads the row's own frames only.
__global__ __launch_bounds__(256) void disc_pad_kernel(const float* __restrict__ x, float* __restrict__ xp, long long T, long long Tp, int left,
                                                       int right, int row0, const DiscLenBlock rows) {
    const int bl = blockIdx.y;
    const int len = rows.e[bl].len;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)len + left + right) return;
    long long j = i - left;
    if (j < 0) j = -j;
    if (j >= len) j = 2LL * (len - 1) - j;
    xp[(row0 + bl) * Tp + i] = x[(row0 + bl) * T + j];
}

// mrd.py:70-71: (b, frame, re[nb] | im[nb]) -> (b, bin, frame) magnitudes, exact zeros at and past the row's frames
__global__ __launch_bounds__(256) void disc_mag_kernel(const float* __restrict__ ri, float* __restrict__ mag, int nb, int F, int row0,
                                                       const DiscLenBlock rows) {
    __shared__ float tile[32][33];
    const int bl = blockIdx.z;
    const int frames = rows.e[bl].frames;
    const long long b = row0 + bl;
    const int f0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + ty + 8 * i, k = k0 + tx;
        float v = 0.f;
        if (f < frames && k < nb) {
            const float* src = ri + (b * F + f) * 2 * nb + k;
            const float re = src[0], im = src[nb];
            v = sqrtf(re * re + im * im);
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, f = f0 + tx;
        if (k < nb && f < F) mag[(b * nb + k) * F + f] = tile[tx][ty + 8 * i];
    }
}

// One workgroup per (row, tile of 4096 elements of the row's OWN extent, in (h, w, c) order): a thread takes elements tid + 256 j of the
// tile in j order with one fp64 accumulator per sum, then a butterfly over the wave and the four waves in order through LDS.  Terms are
// fp32 with one rounding per operation, widened before they are added.
__global__ __launch_bounds__(256) void disc_sums_tile_kernel(const float* __restrict__ real, const float* __restrict__ fake,
                                                             double* __restrict__ partial, const DiscHWBlock rows, int Wmax, int C,
                                                             long long per_row, long long tiles, int row0) {
    __shared__ double red[4][4];
    const int bl = blockIdx.y;
    const DiscHW e = rows.e[bl];
    const long long count = (long long)e.h * e.w * C;
    const long long i0 = (long long)blockIdx.x * kDiscSumTile;
    if (i0 >= count) return;
    const long long b = row0 + bl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wc = e.w * C;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int j = 0; j < kDiscSumPer; ++j) {
        const long long i = i0 + j * 256 + threadIdx.x;
        if (i >= count) break;
        const long long h = i / wc;
        const long long o = b * per_row + h * Wmax * C + (i - h * wc);
        const float r = real[o], f = fake[o];
        const float d = r - f, a = 1.f - f, g = r - 1.f;
        const float aa = a * a, ff = f * f, gg = g * g;
        s[0] += (double)fabsf(d);
        s[1] += (double)aa;
        s[2] += (double)ff;
        s[3] += (double)gg;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += __shfl_xor(s[k], m, 64);
    if (lane == 0)
        for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) t += red[w][threadIdx.x];
        partial[(b * tiles + blockIdx.x) * 4 + threadIdx.x] = t;
    }
}

// One workgroup per row: thread t adds tiles t, t + 256, ... in order, then the same butterfly and wave order: a function of the row's tile
// count alone.  out[b][0..4) the sums, out[b][4] the element count.
__global__ __launch_bounds__(256) void disc_sums_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, long long out_stride,
                                                               const DiscHWBlock rows, int C, long long tiles, int row0) {
    __shared__ double red[4][4];
    const int bl = blockIdx.x;
    const DiscHW e = rows.e[bl];
    const long long count = (long long)e.h * e.w * C;
    const long long nt = (count + kDiscSumTile - 1) / kDiscSumTile;
    const long long b = row0 + bl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long t = threadIdx.x; t < nt; t += 256) {
        const double* p = partial + (b * tiles + t) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += p[k];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += __shfl_xor(s[k], m, 64);
    if (lane == 0)
        for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) t += red[w][threadIdx.x];
        out[b * out_stride + threadIdx.x] = t;
    }
    if (threadIdx.x == 4) out[b * out_stride + 4] = (double)count;
}

// One conv of a critic on the host side
struct DiscLayer {
    int Cin = 0, N = 0, KH = 1, KW = 1, sh = 1, sw = 1, ph = 0, pw = 0;
    bool silu = true;
    std::vector<float> w, b;
    float* d_w = nullptr;
    float* d_b = nullptr;
};

std::string disc_shape_str(const int64_t* shape, int ndim) {
    std::string s = "(";
    for (int i = 0; i < ndim; ++i) s += (i ? ", " : "") + std::to_string((long long)shape[i]);
    return s + ")";
}

long long conv_extent(long long n, int k, int s, int pad) { return n + 2 * pad < k ? 0 : (n + 2 * pad - k) / s + 1; }
size_t round4(size_t n) { return (n + 3) / 4 * 4; }

}  // namespace
}  // namespace fv

using namespace fv;

struct fv_disc {
    fv_disc_config cfg{};
    int n_layers = 0;                               // per sub-discriminator, conv_post included
    std::map<std::string, std::vector<int64_t>> expect;
    std::vector<std::string> order;
    std::map<std::string, std::vector<float>> loaded;
    bool finalized = false;
    std::vector<std::vector<DiscLayer>> sub;        // [sub][layer]
    std::vector<DiscLayer> dft;                     // resolution kind: the windowed DFT of every sub-discriminator, (2 nb, n_fft)
    std::vector<float*> owned;
    ~fv_disc() {
        for (float* d : owned) (void)hipFree(d);
    }
};

namespace {

bool disc_period(const fv_disc_config& c) { return c.kind == FV_DISC_PERIOD; }
int disc_pad_left(const fv_disc_config& c, int i) { return (c.n_fft[i] - c.hop_length[i]) / 2; }
int disc_pad_right(const fv_disc_config& c, int i) { return (c.n_fft[i] - c.hop_length[i] + 1) / 2; }
// the shortest row sub-discriminator i takes: one frame, and longer than the reflect padding
int disc_min_length(const fv_disc_config& c, int i) { return disc_period(c) ? 1 : std::max(c.hop_length[i], disc_pad_right(c, i) + 1); }

// (H, W) of the input map (index 0) and of every layer's output (index l + 1) of sub-discriminator i for a row of L samples
void disc_extents(const fv_disc* d, int i, long long L, long long* H, long long* W) {
    const fv_disc_config& c = d->cfg;
    if (disc_period(c)) H[0] = (L + c.period[i] - 1) / c.period[i], W[0] = L > 0 ? c.period[i] : 0;
    else H[0] = L > 0 ? c.n_fft[i] / 2 + 1 : 0, W[0] = L / c.hop_length[i];
    for (int l = 0; l < d->n_layers; ++l) {
        const DiscLayer& y = d->sub[i][l];
        H[l + 1] = H[l] > 0 ? conv_extent(H[l], y.KH, y.sh, y.ph) : 0;
        W[l + 1] = W[l] > 0 ? conv_extent(W[l], y.KW, y.sw, y.pw) : 0;
    }
}

struct DiscPlan {
    long long H[kDiscMaxSub][kDiscMaxLayers + 1], W[kDiscMaxSub][kDiscMaxLayers + 1];
    size_t offset[kDiscMaxSub][kDiscMaxLayers];
    size_t out_floats = 0;
    size_t xp = 0, ri = 0, mag = 0, ws_floats = 0;  // forward's workspace: the padded wave, the DFT and the magnitudes of one sub-discriminator
    long long Tp = 0;
    size_t sum_tiles = 0, sum_bytes = 0;            // the distance's partials
    bool too_big = false;
};
DiscPlan disc_plan(const fv_disc* d, int batch, long long T) {
    DiscPlan pl{};
    const fv_disc_config& c = d->cfg;
    const size_t B = (size_t)batch;
    for (int i = 0; i < c.n_sub; ++i) {
        disc_extents(d, i, T, pl.H[i], pl.W[i]);
        for (int l = 0; l < d->n_layers; ++l) {
            const unsigned long long per_row = (unsigned long long)pl.H[i][l + 1] * pl.W[i][l + 1] * d->sub[i][l].N;
            if (per_row > (unsigned long long)INT_MAX) pl.too_big = true;
            pl.offset[i][l] = pl.out_floats;
            pl.out_floats += round4(B * per_row);
            pl.sum_tiles = std::max<size_t>(pl.sum_tiles, (per_row + kDiscSumTile - 1) / kDiscSumTile);
        }
        if (!disc_period(c)) {
            const int N = c.n_fft[i], nb = N / 2 + 1;
            const long long Tp = (long long)round4((size_t)(T + N - c.hop_length[i]));
            const unsigned long long F = pl.W[i][0];
            if (F * 2 * nb > (unsigned long long)INT_MAX || (unsigned long long)Tp > (unsigned long long)INT_MAX) pl.too_big = true;
            pl.Tp = std::max(pl.Tp, Tp);
            pl.xp = std::max(pl.xp, round4(B * Tp));
            pl.ri = std::max(pl.ri, round4(B * F * 2 * nb));
            pl.mag = std::max(pl.mag, round4(B * F * nb));
        }
    }
    pl.ws_floats = pl.xp + pl.ri + pl.mag;
    pl.sum_bytes = B * pl.sum_tiles * 4 * sizeof(double);
    return pl;
}

fv_status disc_check_shape(const char* fn, const fv_disc* d, int32_t batch, int64_t T) {
    if (!d) {
        set_error("%s: null discriminator", fn);
        return FV_ERR_INVALID;
    }
    if (!d->finalized) {
        set_error("%s: the discriminator has not been finalized (fv_disc_finalize)", fn);
        return FV_ERR_STATE;
    }
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kDiscMaxSamples) {
        set_error("%s: T = %lld must lie in [0, 2^26]", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

fv_status disc_check_lengths(const char* fn, const fv_disc* d, int64_t T, const int32_t* host_lengths, int32_t batch) {
    const fv_disc_config& c = d->cfg;
    for (int b = 0; b < batch; ++b) {
        const long long n = host_lengths ? host_lengths[b] : T;
        const std::string what = host_lengths ? "host_lengths[" + std::to_string(b) + "]" : std::string("T");
        if (n < 0 || n > T) {
            set_error("%s: %s = %lld lies outside [0, T = %lld]", fn, what.c_str(), n, (long long)T);
            return FV_ERR_INVALID;
        }
        if (n == 0) {
            set_error("%s: %s = 0: a row of 0 samples has no feature map (row %d)", fn, what.c_str(), b);
            return FV_ERR_INVALID;
        }
        for (int i = 0; i < c.n_sub; ++i)
            if (n < disc_min_length(c, i)) {
                set_error("%s: %s = %lld is below the minimum length %d of discriminator %d (n_fft = %d, hop_length = %d: row %d must be "
                          "longer than the reflect padding %d and hold one frame)", fn, what.c_str(), n, disc_min_length(c, i), i, c.n_fft[i],
                          c.hop_length[i], b, disc_pad_right(c, i));
                return FV_ERR_INVALID;
            }
    }
    return FV_OK;
}

template <int EPI>
void disc_conv_launch(const DiscLayer& l, const float* a, long long a_bstride, int hs, int ws, float* y, int Hout, int Wout, int row0, int nrows,
                      const DiscRowBlock& rows, hipStream_t s) {
    DiscConvParams p{};
    p.a = a, p.a_bstride = a_bstride, p.hs = hs, p.ws = ws;
    p.Cin = l.Cin, p.KW = l.KW, p.sh = l.sh, p.sw = l.sw, p.ph = l.ph, p.pw = l.pw, p.K = l.KH * l.KW * l.Cin;
    p.w = l.d_w, p.bias = l.d_b, p.N = l.N, p.y = y, p.Hout = Hout, p.Wout = Wout, p.row0 = row0;
    const long long M = (long long)Hout * Wout;
    auto blocks = [&](int fb, int cb) { return (M + fb - 1) / fb * ((l.N + cb - 1) / cb) * nrows; };
    auto go = [&](auto kernel, int fb, int cb) {
        const dim3 grid((unsigned)((M + fb - 1) / fb), (unsigned)((l.N + cb - 1) / cb), (unsigned)nrows);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p, rows);
    };
    // the largest tile that still gives every compute unit a workgroup, else the smallest; the sums do not depend on it
    const long long fill = num_cus();
    const bool vec = l.Cin % 4 == 0 && hs % 4 == 0 && ws % 4 == 0 && a_bstride % 4 == 0;
    if (l.N <= 32) {            // the four waves along the positions
        const bool big = blocks(256, 32) >= fill;
        if (vec) {
            if (big) go(disc_conv_kernel<EPI, 2, 1, 1, 16, true>, 256, 32);
            else go(disc_conv_kernel<EPI, 1, 1, 1, 32, true>, 128, 32);
        } else {
            if (big) go(disc_conv_kernel<EPI, 2, 1, 1, 16, false>, 256, 32);
            else go(disc_conv_kernel<EPI, 1, 1, 1, 32, false>, 128, 32);
        }
        return;
    }
    const int tile = blocks(128, 128) >= fill ? 0 : blocks(64, 128) >= fill ? 1 : 2;
    if (vec) {
        if (tile == 0) go(disc_conv_kernel<EPI, 2, 2, 2, 16, true>, 128, 128);
        else if (tile == 1) go(disc_conv_kernel<EPI, 1, 2, 2, 32, true>, 64, 128);
        else go(disc_conv_kernel<EPI, 1, 1, 2, 32, true>, 64, 64);
    } else {
        if (tile == 0) go(disc_conv_kernel<EPI, 2, 2, 2, 16, false>, 128, 128);
        else if (tile == 1) go(disc_conv_kernel<EPI, 1, 2, 2, 32, false>, 64, 128);
        else go(disc_conv_kernel<EPI, 1, 1, 2, 32, false>, 64, 64);
    }
}

void disc_conv(const DiscLayer& l, const float* a, long long a_bstride, int hs, int ws, float* y, int Hout, int Wout, int row0, int nrows,
               const DiscRowBlock& rows, hipStream_t s) {
    if (l.silu) disc_conv_launch<DISC_SILU>(l, a, a_bstride, hs, ws, y, Hout, Wout, row0, nrows, rows, s);
    else disc_conv_launch<DISC_BIAS>(l, a, a_bstride, hs, ws, y, Hout, Wout, row0, nrows, rows, s);
}

fv_status disc_upload(fv_disc* d, DiscLayer& l) {
    for (auto pr : {std::make_pair(&l.w, &l.d_w), std::make_pair(&l.b, &l.d_b)}) {
        FV_HIP_CHECK(hipMalloc(pr.second, std::max<size_t>(pr.first->size(), 4) * 4));
        d->owned.push_back(*pr.second);
        FV_HIP_CHECK(hipMemcpy(*pr.second, pr.first->data(), pr.first->size() * 4, hipMemcpyHostToDevice));
        *pr.first = std::vector<float>();
    }
    return FV_OK;
}

std::string disc_conv_prefix(int i, int l, int n_layers) {
    const std::string pfx = "discriminators." + std::to_string(i) + ".";
    return l == n_layers - 1 ? pfx + "conv_post." : pfx + "convs." + std::to_string(l) + ".";
}
const char* kDiscG = "parametrizations.weight.original0";
const char* kDiscV = "parametrizations.weight.original1";

}  // namespace

extern "C" {

FV_API fv_status fv_disc_create(const fv_disc_config* cfg, fv_disc** out) {
    const char* fn = "fv_disc_create";
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
    if (!range("kind", cfg->kind, FV_DISC_PERIOD, FV_DISC_RESOLUTION) || !range("n_sub", cfg->n_sub, 1, kDiscMaxSub)) return FV_ERR_INVALID;
    std::unique_ptr<fv_disc> d(new fv_disc());
    d->cfg = *cfg;
    d->sub.resize(cfg->n_sub);
    if (cfg->kind == FV_DISC_PERIOD) {
        if (!range("n_channels", cfg->n_channels, 2, kDiscMaxChannels) || !range("kernel_size", cfg->kernel_size, 1, kDiscMaxKernel) ||
            !range("stride", cfg->stride, 1, kDiscMaxStride))
            return FV_ERR_INVALID;
        if (cfg->channels[0] != 1) {
            set_error("%s: channels[0] = %d must be 1 (the folded wave)", fn, cfg->channels[0]);
            return FV_ERR_INVALID;
        }
        for (int l = 1; l < cfg->n_channels; ++l) {
            const std::string name = "channels[" + std::to_string(l) + "]";
            if (!range(name, cfg->channels[l], 4, kDiscMaxWidth)) return FV_ERR_INVALID;
            if (cfg->channels[l] % 4) {
                set_error("%s: %s = %d must be a multiple of 4 (positions move as 16-byte quads)", fn, name.c_str(), cfg->channels[l]);
                return FV_ERR_INVALID;
            }
        }
        for (int i = 0; i < cfg->n_sub; ++i)
            if (!range("period[" + std::to_string(i) + "]", cfg->period[i], 1, kDiscMaxPeriod)) return FV_ERR_INVALID;
        d->n_layers = cfg->n_channels;          // n_channels - 1 convs and conv_post
        for (int i = 0; i < cfg->n_sub; ++i) {
            for (int l = 0; l + 1 < cfg->n_channels; ++l) {
                DiscLayer y;
                y.Cin = cfg->channels[l], y.N = cfg->channels[l + 1], y.KH = cfg->kernel_size, y.sh = cfg->stride, y.ph = cfg->kernel_size / 2;
                d->sub[i].push_back(y);
            }
            DiscLayer post;
            post.Cin = cfg->channels[cfg->n_channels - 1], post.N = 1, post.KH = 3, post.ph = 1, post.silu = false;
            d->sub[i].push_back(post);
        }
    } else {
        for (int i = 0; i < cfg->n_sub; ++i) {
            const std::string idx = "[" + std::to_string(i) + "]";
            if (!range("n_fft" + idx, cfg->n_fft[i], 4, kDiscMaxFft)) return FV_ERR_INVALID;
            if (cfg->n_fft[i] % 4) {
                set_error("%s: n_fft%s = %d must be a multiple of 4 (a frame moves as 16-byte quads)", fn, idx.c_str(), cfg->n_fft[i]);
                return FV_ERR_INVALID;
            }
            if (!range("hop_length" + idx, cfg->hop_length[i], 1, cfg->n_fft[i]) || !range("win_length" + idx, cfg->win_length[i], 1, cfg->n_fft[i]))
                return FV_ERR_INVALID;
        }
        d->n_layers = 6;
        for (int i = 0; i < cfg->n_sub; ++i)
            for (int l = 0; l < 6; ++l) {
                DiscLayer y;
                y.Cin = l ? 32 : 1, y.N = l < 5 ? 32 : 1, y.KH = 3, y.ph = 1;
                y.KW = l < 4 ? 9 : 3, y.pw = l < 4 ? 4 : 1, y.sw = l >= 1 && l <= 3 ? 2 : 1;
                y.silu = l < 5;
                d->sub[i].push_back(y);
            }
    }
    for (int i = 0; i < cfg->n_sub; ++i)
        for (int l = 0; l < d->n_layers; ++l) {
            const DiscLayer& y = d->sub[i][l];
            const std::string pfx = disc_conv_prefix(i, l, d->n_layers);
            for (const auto& kv : {std::make_pair(pfx + "bias", std::vector<int64_t>{y.N}), std::make_pair(pfx + kDiscG, std::vector<int64_t>{y.N, 1, 1, 1}),
                                   std::make_pair(pfx + kDiscV, std::vector<int64_t>{y.N, y.Cin, y.KH, y.KW})}) {
                d->order.push_back(kv.first);
                d->expect[kv.first] = kv.second;
            }
        }
    *out = d.release();
    return FV_OK;
}

FV_API void fv_disc_destroy(fv_disc* d) { delete d; }

FV_API fv_status fv_disc_load_weight(fv_disc* d, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    const char* fn = "fv_disc_load_weight";
    if (!d || !name || !host || ndim < 0 || (ndim > 0 && !shape)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (d->finalized) {
        set_error("%s: '%s' arrives after fv_disc_finalize", fn, name);
        return FV_ERR_STATE;
    }
    std::string key = name;
    for (const auto& legacy : {std::make_pair(".weight_g", kDiscG), std::make_pair(".weight_v", kDiscV)}) {
        const size_t n = strlen(legacy.first);
        if (key.size() > n && !key.compare(key.size() - n, n, legacy.first)) key = key.substr(0, key.size() - n + 1) + legacy.second;
    }
    const auto it = d->expect.find(key);
    if (it == d->expect.end()) {
        set_error("%s: unknown key '%s'", fn, name);
        return FV_ERR_INVALID;
    }
    const std::vector<int64_t>& want = it->second;
    if ((size_t)ndim != want.size() || !std::equal(want.begin(), want.end(), shape)) {
        set_error("%s: '%s' has shape %s, expected %s", fn, name, disc_shape_str(shape, ndim).c_str(), disc_shape_str(want.data(), (int)want.size()).c_str());
        return FV_ERR_SHAPE;
    }
    size_t n = 1;
    for (int64_t v : want) n *= (size_t)v;
    d->loaded[key].assign(host, host + n);
    return FV_OK;
}

FV_API fv_status fv_disc_finalize(fv_disc* d) {
    const char* fn = "fv_disc_finalize";
    if (!d) {
        set_error("%s: null discriminator", fn);
        return FV_ERR_INVALID;
    }
    if (d->finalized) {
        set_error("%s: already finalized", fn);
        return FV_ERR_STATE;
    }
    for (const std::string& key : d->order)
        if (!d->loaded.count(key)) {
            set_error("%s: missing weight '%s'", fn, key.c_str());
            return FV_ERR_MISSING_WEIGHT;
        }
    const fv_disc_config& c = d->cfg;
    for (int i = 0; i < c.n_sub; ++i)
        for (int l = 0; l < d->n_layers; ++l) {
            DiscLayer& y = d->sub[i][l];
            const std::string pfx = disc_conv_prefix(i, l, d->n_layers);
            const std::vector<float>&g = d->loaded[pfx + kDiscG], &v = d->loaded[pfx + kDiscV];
            // weight norm over dims 1-3 (weight_norm's dim = 0): w[n] = g[n] v[n] / |v[n]|, in fp64, rounded once; (N, C, KH, KW) -> (N, KH, KW, C)
            const size_t per = (size_t)y.Cin * y.KH * y.KW;
            y.w.resize((size_t)y.N * per);
            for (int n = 0; n < y.N; ++n) {
                double ss = 0.0;
                for (size_t e = 0; e < per; ++e) ss += (double)v[n * per + e] * (double)v[n * per + e];
                const double scale = (double)g[n] / std::sqrt(ss);
                for (int ci = 0; ci < y.Cin; ++ci)
                    for (int t = 0; t < y.KH * y.KW; ++t)
                        y.w[(n * (size_t)(y.KH * y.KW) + t) * y.Cin + ci] = (float)((double)v[n * per + (size_t)ci * y.KH * y.KW + t] * scale);
            }
            y.b = d->loaded[pfx + "bias"];
        }
    if (!disc_period(c)) {
        d->dft.resize(c.n_sub);
        for (int i = 0; i < c.n_sub; ++i) {
            // torch.stft(window = None): ones of win_length, centred in n_fft (mrd.py:62-69)
            const int N = c.n_fft[i], nb = N / 2 + 1, left = (N - c.win_length[i]) / 2;
            std::vector<float> win(N, 0.f);
            for (int n = 0; n < c.win_length[i]; ++n) win[left + n] = 1.f;
            DiscLayer& y = d->dft[i];
            y.Cin = N, y.N = 2 * nb, y.silu = false;
            y.w = stft_basis(win, N, N, 1);         // (2 nb, N): cos rows, then -sin rows
            y.b.assign(2 * nb, 0.f);
        }
    }
    for (int i = 0; i < c.n_sub; ++i) {
        for (DiscLayer& y : d->sub[i])
            if (const fv_status st = disc_upload(d, y)) return st;
        if (!disc_period(c))
            if (const fv_status st = disc_upload(d, d->dft[i])) return st;
    }
    d->loaded.clear();
    d->finalized = true;
    return FV_OK;
}

FV_API int64_t fv_disc_layout(const fv_disc* d, int32_t batch, int64_t T, fv_disc_map* maps, int32_t capacity, int32_t* n_maps) {
    const char* fn = "fv_disc_layout";
    if (!d || batch < 0 || batch > 65535 || T < 0 || T > kDiscMaxSamples) {
        set_error("%s: a null discriminator, batch = %d outside [0, 65535] or T = %lld outside [0, 2^26]", fn, batch, (long long)T);
        return -1;
    }
    const int n = d->cfg.n_sub * d->n_layers;
    if (n_maps) *n_maps = n;
    const DiscPlan pl = disc_plan(d, batch, T);
    if (pl.too_big) {
        set_error("%s: T = %lld gives a feature map of more than 2^31 - 1 elements per row", fn, (long long)T);
        return -1;
    }
    if (maps) {
        if (capacity < n) {
            set_error("%s: capacity = %d is below the %d maps of this discriminator", fn, capacity, n);
            return -1;
        }
        for (int i = 0; i < d->cfg.n_sub; ++i)
            for (int l = 0; l < d->n_layers; ++l) {
                fv_disc_map& m = maps[i * d->n_layers + l];
                m.offset = (int64_t)pl.offset[i][l];
                m.H = (int32_t)pl.H[i][l + 1], m.W = (int32_t)pl.W[i][l + 1], m.C = d->sub[i][l].N;
                m.sub = i, m.layer = l;
            }
    }
    return (int64_t)pl.out_floats;
}

FV_API size_t fv_disc_workspace_bytes(const fv_disc* d, int32_t batch, int64_t T) {
    if (!d || batch < 0 || batch > 65535 || T < 0 || T > kDiscMaxSamples) {
        set_error("fv_disc_workspace_bytes: a null discriminator, batch = %d outside [0, 65535] or T = %lld outside [0, 2^26]", batch, (long long)T);
        return 0;
    }
    const DiscPlan pl = disc_plan(d, batch, T);
    if (pl.too_big) return 0;
    return (std::max(pl.ws_floats * sizeof(float), pl.sum_bytes) + 255) / 256 * 256;
}

FV_API fv_status fv_disc_forward(fv_disc* d, const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_out,
                                 int64_t out_floats, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fv_disc_forward";
    if (const fv_status st = disc_check_shape(fn, d, batch, T)) return st;
    if (batch == 0) return FV_OK;
    if (!d_x || !d_out) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : "d_out");
        return FV_ERR_INVALID;
    }
    if (const fv_status st = disc_check_lengths(fn, d, T, host_lengths, batch)) return st;
    const fv_disc_config& c = d->cfg;
    const DiscPlan pl = disc_plan(d, batch, T);
    if (pl.too_big) {
        set_error("%s: T = %lld gives a feature map of more than 2^31 - 1 elements per row", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    if (out_floats < (int64_t)pl.out_floats) {
        set_error("%s: out_floats = %lld is below the %zu that fv_disc_layout(batch = %d, T = %lld) gives", fn, (long long)out_floats, pl.out_floats, batch,
                  (long long)T);
        return FV_ERR_INVALID;
    }
    const size_t need = pl.ws_floats * sizeof(float);
    if (need && (workspace_bytes < need || !d_workspace)) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_disc_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, need, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (((uintptr_t)d_workspace | (uintptr_t)d_out) % 16) {
        set_error("%s: d_workspace and d_out must be 16-byte aligned (positions move as 16-byte quads)", fn);
        return FV_ERR_INVALID;
    }
    // everything is validated: enqueue

    hipStream_t s = (hipStream_t)stream;
    float* xp = (float*)d_workspace;
    float* ri = xp + pl.xp;
    float* mag = ri + pl.ri;
    const int nl = d->n_layers;
    auto block = [&](const LaunchTable<int, kDiscRows>& lens, int row0, int nrows) -> fv_status {
        for (int i = 0; i < c.n_sub; ++i) {
            long long rh[kDiscRows][kDiscMaxLayers + 1], rw[kDiscRows][kDiscMaxLayers + 1];
            for (int r = 0; r < nrows; ++r) disc_extents(d, i, lens.e[r], rh[r], rw[r]);
            const float* cur;
            long long cur_bstride;
            int hs, ws;
            if (disc_period(c)) {       // the fold is the first conv's addressing (mpd.py:47-52)
                cur = d_x, cur_bstride = T, hs = c.period[i], ws = 1;
            } else {
                const int N = c.n_fft[i], nb = N / 2 + 1, hop = c.hop_length[i], left = disc_pad_left(c, i), right = disc_pad_right(c, i);
                const int F = (int)pl.W[i][0];
                const long long Tp = (long long)round4((size_t)(T + N - hop));
                DiscLenBlock lt{};
                DiscRowBlock ext{};
                for (int r = 0; r < nrows; ++r) {
                    lt.e[r].len = lens.e[r], lt.e[r].frames = (int)rw[r][0];
                    ext.e[r] = DiscExt{(int)rw[r][0], 1, (int)rw[r][0], 1, lens.e[r] + left + right};
                }
                hipLaunchKernelGGL(disc_pad_kernel, dim3((unsigned)((T + left + right + 255) / 256), (unsigned)nrows), dim3(256), 0, s, d_x, xp, (long long)T,
                                   Tp, left, right, row0, lt);
                disc_conv(d->dft[i], xp, Tp, hop, 0, ri, F, 1, row0, nrows, ext, s);
                hipLaunchKernelGGL(disc_mag_kernel, dim3((unsigned)((F + 31) / 32), (unsigned)((nb + 31) / 32), (unsigned)nrows), dim3(256), 0, s, ri, mag, nb, F,
                                   row0, lt);
                cur = mag, cur_bstride = (long long)nb * F, hs = F, ws = 1;
            }
            for (int l = 0; l < nl; ++l) {
                const DiscLayer& y = d->sub[i][l];
                DiscRowBlock ext{};
                for (int r = 0; r < nrows; ++r) {
                    const long long limit = l == 0 && disc_period(c) ? (long long)lens.e[r] : rh[r][l] * hs;
                    ext.e[r] = DiscExt{(int)rh[r][l], (int)rw[r][l], (int)rh[r][l + 1], (int)rw[r][l + 1], (int)limit};
                }
                const int Ho = (int)pl.H[i][l + 1], Wo = (int)pl.W[i][l + 1];
                float* out = d_out + pl.offset[i][l];
                disc_conv(y, cur, cur_bstride, hs, ws, out, Ho, Wo, row0, nrows, ext, s);
                cur = out, cur_bstride = (long long)Ho * Wo * y.N, hs = Wo * y.N, ws = y.N;
            }
        }
        return FV_OK;
    };
    const fv_status st = for_each_launch_table<LaunchTable<int, kDiscRows>>(batch, [&](int b) { return host_lengths ? host_lengths[b] : (int)T; }, block);
    if (st == FV_OK) set_last_kernel("disc_conv_kernel");
    return st;
}

FV_API fv_status fv_disc_distance(fv_disc* d, const float* d_real, const float* d_fake, int64_t T, const int32_t* host_lengths, int32_t batch,
                                  double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fv_disc_distance";
    if (const fv_status st = disc_check_shape(fn, d, batch, T)) return st;
    if (batch == 0) return FV_OK;
    if (!d_real || !d_fake || !d_sums) {
        set_error("%s: null %s", fn, !d_real ? "d_real" : !d_fake ? "d_fake" : "d_sums");
        return FV_ERR_INVALID;
    }
    if (const fv_status st = disc_check_lengths(fn, d, T, host_lengths, batch)) return st;
    const fv_disc_config& c = d->cfg;
    const DiscPlan pl = disc_plan(d, batch, T);
    if (pl.too_big) {
        set_error("%s: T = %lld gives a feature map of more than 2^31 - 1 elements per row", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    if (workspace_bytes < pl.sum_bytes || !d_workspace) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_disc_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, pl.sum_bytes, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)d_workspace;
    const int nl = d->n_layers;
    const long long out_stride = (long long)c.n_sub * nl * 5;
    auto block = [&](const LaunchTable<int, kDiscRows>& lens, int row0, int nrows) -> fv_status {
        for (int i = 0; i < c.n_sub; ++i) {
            long long rh[kDiscRows][kDiscMaxLayers + 1], rw[kDiscRows][kDiscMaxLayers + 1];
            for (int r = 0; r < nrows; ++r) disc_extents(d, i, lens.e[r], rh[r], rw[r]);
            for (int l = 0; l < nl; ++l) {
                const int C = d->sub[i][l].N, Wmax = (int)pl.W[i][l + 1];
                const long long per_row = pl.H[i][l + 1] * Wmax * C;
                DiscHWBlock hw{};
                long long most = 0;
                for (int r = 0; r < nrows; ++r) {
                    hw.e[r] = DiscHW{(int)rh[r][l + 1], (int)rw[r][l + 1]};
                    most = std::max(most, rh[r][l + 1] * rw[r][l + 1] * C);
                }
                const long long tiles = (long long)pl.sum_tiles;
                hipLaunchKernelGGL(disc_sums_tile_kernel, dim3((unsigned)((most + kDiscSumTile - 1) / kDiscSumTile), (unsigned)nrows), dim3(256), 0, s,
                                   d_real + pl.offset[i][l], d_fake + pl.offset[i][l], partial, hw, Wmax, C, per_row, tiles, row0);
                hipLaunchKernelGGL(disc_sums_finish_kernel, dim3((unsigned)nrows), dim3(256), 0, s, partial, d_sums + (size_t)(i * nl + l) * 5, out_stride, hw,
                                   C, tiles, row0);
            }
        }
        return FV_OK;
    };
    const fv_status st = for_each_launch_table<LaunchTable<int, kDiscRows>>(batch, [&](int b) { return host_lengths ? host_lengths[b] : (int)T; }, block);
    if (st == FV_OK) set_last_kernel("disc_sums_tile_kernel");
    return st;
}

}  // extern "C"
