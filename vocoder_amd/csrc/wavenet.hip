// Posterior encoder (include/fishvoc.h fv_posterior_*): the WaveNet encoder of VITS / RVC, the reference's
// modules/encoders/posterior_encoder.py:57-80,133-160 in eval mode.  2 n_layers + 2 launches per forward and block of kWnRows batch rows:
//   wn_pre       h = pre(x) m                                    1 x 1 GEMM in_channels -> C, x read through a row stride
//   wn_gate      g = tanh(a[:C]) sigmoid(a[C:]), a = in_i(h)     implicit-GEMM dilated conv C -> 2C; `a` never reaches memory
//   wn_res_skip  h = (h + r[:C]) m, out (+)= r[C:], r = rs_i(g)  1 x 1 GEMM C -> 2C (the last layer: C -> C, out only); the first layer WRITES out
//   wn_proj      y = proj(out m) m and the mode's tail           1 x 1 GEMM C -> out_channels (vqvae) or 2 out_channels (split, clamp, BatchNorm, z)
// One body (wn_body) serves all four: exact fp32 on v_mfma_f32_32x32x2_f32 with the activation window staged through LDS in chunks of 8
// channels, as conv_generic.hip does (conv_mfma_impl.h's structure with the tap offsets either folded at compile time — the default k = 5,
// d = 1 and the 1 x 1 GEMMs — or computed); several chunks share a barrier where the window is short, the next stage's loads and the next
// weight fragments are in flight while a stage's MFMAs run.  Every GEMM has two row HALVES (the gate: tanh | sigmoid; res_skip: res | skip; proj in the vae
// modes: mean | logvar; pre and the vqvae proj: one half) and a wave carries an accumulator PAIR, M-tile j of either half: register r of
// lane l holds channel 32 j + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of both halves at column l & 31, so the gate and the split are register-wise.
// The weights are packed with a pair's two fragments adjacent; where a half is no multiple of 32 rows its last tile is zero padded and the
// padded rows are never stored.
// Ragged rows: the rows' lengths travel by value (LaunchTable).  The staging applies both the conv's zero padding and the row's length — a
// frame at or past lengths[b], and the padding of x, is never loaded — so h, g and out are neither written nor read past a row's length.
// Summation order: an output element's sum is one accumulator chain over (8-channel chunk, tap, channel pair), from chunk 0, then one
// addition of the bias: an order fixed by the layer's shape alone.  It does not depend on the batch, the column's tile or place in it, the
// tile width (WN) or the other rows' lengths (masked frames and padded channels add exact zeros in the same places), so a row has the same
// bits alone, in any batch and padded to any T.
// The stream (fv_wnstream_*): the same body instantiated with STREAM — a column origin, input and output addresses through a WnSpan (a ring
// or a linear buffer) and the input's valid range [lo, frontier) — runs every layer over a push's new columns only, out of one ring per
// layer input.  Nothing above depends on where a column sits, so a stream has the whole row's bits under any chunking.
// The pool (fv_wnpool_*): the body once more, instantiated with WN_POOL — the stream's form with the column origin, the end and the frontier
// taken per table entry (blockIdx.z), rings addressed by the entry's slot — for sessions that advance independently: one launch serves
// every item of a step, and a session has the bits of its whole utterance whatever the other sessions do.
// The counters of the stream and the pool, the refusals of a push, flush or step and the emission rule are frame_pool.h's (FrameStream,
// FramePool); this file keeps the rings (WnRings), the tables, the launches and the vqvae mode's refusal.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>

#include "fv_internal.h"
#include "frame_pool.h"

namespace fv {
namespace {

typedef float wn_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWnRows = 256;                        // rows per launch: their lengths are a LaunchTable (fv_internal.h)
constexpr size_t kWnLdsBudget = 64 * 1024;          // two staged chunks of kChunk x (columns + (k - 1) d) floats, as launch_conv_generic checks
constexpr int kWnWideCols = 128;                    // columns of the wide tile (four waves side by side); the narrow one is 32 (four pairs)
constexpr int kWnNarrowMaxT = 64;                   // T up to here runs the narrow tile
constexpr int kWnMaxHidden = 1024, kWnMaxIo = 4096, kWnMaxKernel = 11, kWnMaxLayers = 64;
constexpr long long kWnMaxFrames = 1LL << 30;
constexpr double kBnEps = 1e-5;                     // nn.BatchNorm1d's default (posterior_encoder.py:129)

constexpr int kWnSlots = 32;                        // staged floats per thread and stage, held in registers while the previous stage computes
constexpr int kWnRing = 4;                          // weight fragments in flight per wave and half
constexpr int kWnMaxStageChunks = 8;

using WnRowBlock = LaunchTable<int, kWnRows>;

// The pool form's table (fv_wnpool_*): an entry is one item of a step in one launch — the slot whose ring rows it reads and writes, its first
// column, its end (what T is to the stream: no column at or past it is written) and its input's frontier (what `uniform` is to the stream)
struct WnPoolEntry {
    int slot, col0, end, front;
};
constexpr int kWnPoolBlock = 128;                   // entries per launch: 2 KiB, with WnParams well inside the 4 KiB kernel-argument segment
using WnPoolBlock = LaunchTable<WnPoolEntry, kWnPoolBlock>;

enum WnForm : int { WN_ROWS = 0, WN_STREAM = 1, WN_POOL = 2 };

enum WnMode : int { WN_GATE = 0, WN_RES_SKIP = 1, WN_PRE = 2, WN_PROJ = 3 };

// Frame t of channel row r is element r * stride + ((t - org) & mask): a ring of `stride` = mask + 1 frames (org 0), or a linear buffer
// whose first frame is org (mask -1)
struct WnSpan {
    long long stride;
    int org, mask;
    __host__ __device__ long long at(long long r, int t) const { return r * stride + ((t - org) & mask); }
};

struct WnParams {
    const float* x;                 // (., Cin, .): element (b, c, t) at b * x_bstride + c * x_cstride + t
    long long x_bstride, x_cstride;
    int Cin, nchunk;                // nchunk = ceil(Cin / kChunk)
    const float4* wp;               // fragments [((pair * nchunk + chunk) * ks + tap) * 2 + half][lane], component q = w[half][32 pair + (lane & 31)][8 chunk + 2 q + (lane >> 5)][tap]
    const float* bias;              // 32 npairs values of half 0, then of half 1, zero padded
    int M0, M1, npairs;             // rows of the two halves; npairs = ceil(max(M0, M1) / 32)
    int T, ks, dil;
    int row0, uniform;              // first batch row of the launch; >= 0: every row holds this many frames and the table is not read
    float* y0;                      // half 0: g (gate), h (pre; res_skip, in place), z (vqvae proj), mean or NULL (vae proj)
    float* y1;                      // half 1: out (res_skip), logvar or NULL (vae proj)
    float* z;                       // vae proj: mean m
    const float* bn_scale;          // bnvae: mean = v scale + shift, applied after the mask
    const float* bn_shift;
    int first;                      // res_skip: the first layer writes out
    int G;                          // chunks staged per barrier (wn_stage_chunks)
    // The stream instantiations only (fv_wnstream_*).  A launch covers the frames [col0, T) of every row; `uniform` is the input's frontier
    // (frames at or past it stage as zero, whatever a ring holds there) and `lo` its first frame in memory.  A WnSpan is where a frame lives.
    // The pool instantiations (fv_wnpool_*) take col0, T and the frontier from their entry; `lo` != 0 says the input begins at the entry's
    // col0 (else at frame 0).  A ring span is indexed by the entry's slot, a linear one by the item's row row0 + blockIdx.z, origin col0.
    int col0, lo;
    WnSpan xs, y0s, y1s, rs;        // of x, of y0 (and z), of y1, of res
    const float* res;               // res_skip: the residual input h_i (its own ring; y0 is the ring of h_{i + 1})
};

// WN waves side by side along time (32 columns each) x 4 / WN pairs; KS = 0: taps and dilation at run time
// WN_STREAM: the tile's columns are the frames col0 + ..., and every address goes through a WnSpan; the sums are the whole-row ones
// WN_POOL: the stream's form with col0, the end and the frontier per table entry (blockIdx.z): sessions that advance independently
template <int MODE, int WN, int KS, int DIL, int FORM = WN_ROWS, class Rows = WnRowBlock>
__device__ __forceinline__ void wn_body(const WnParams& p, const Rows& rows) {
    constexpr bool STREAM = FORM != WN_ROWS, POOL = FORM == WN_POOL;
    constexpr int WM = 4 / WN, N_BLK = 32 * WN;
    extern __shared__ __attribute__((aligned(16))) float wn_xs[];
    const int ks = KS ? KS : p.ks, dil = KS ? DIL : p.dil;
    const int W = N_BLK + (ks - 1) * dil;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WN, wm = wave / WN;
    const int bl = blockIdx.z;
    const long long b = p.row0 + bl;
    int len, cbase, Tend, lo, slot = 0;
    if constexpr (POOL) {
        const WnPoolEntry e = rows.e[bl];
        len = e.front, cbase = e.col0, Tend = e.end, lo = p.lo ? e.col0 : 0, slot = e.slot;
    } else {
        len = STREAM || p.uniform >= 0 ? p.uniform : rows.e[bl];
        cbase = STREAM ? p.col0 : 0, Tend = p.T, lo = p.lo;
    }
    const int n0 = cbase + blockIdx.x * N_BLK;
    if (POOL && n0 >= Tend) return;                             // the grid is the widest entry's: this one has no column here (block-uniform)
    if ((FORM == WN_STREAM || MODE != WN_PROJ) && n0 >= len) return;       // nothing of this tile is ever read (block-uniform); proj still writes its zeros
    // where frame t of row m of a span's tensor lives
    auto at = [&](const WnSpan& sp, int M, int m, int t) -> long long {
        if constexpr (POOL) return ((sp.mask < 0 ? b : (long long)slot) * M + m) * sp.stride + ((t - (sp.mask < 0 ? cbase : 0)) & sp.mask);
        else return sp.at(b * M + m, t);
    };
    const int pair = blockIdx.y * WM + wm;
    const bool do0 = pair < p.npairs && pair * 32 < p.M0, do1 = pair < p.npairs && pair * 32 < p.M1;      // wave-uniform

    wn_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = 0.f, acc1[r] = 0.f;

    if (n0 < len) {
        const float* __restrict__ xb = p.x + (POOL && p.xs.mask >= 0 ? (long long)slot : b) * p.x_bstride;
        const int xorg = POOL ? (p.xs.mask < 0 ? cbase : 0) : p.xs.org;
        const int tbase = n0 - (ks - 1) * dil / 2;
        const int G = p.G, total = G * kChunk * W;          // a stage: G chunks, G kChunk W <= 256 kWnSlots floats (wn_stage_chunks)
        const int nstage = (p.nchunk + G - 1) / G;
        const int b_lane = (lane >> 5) * W + wn * 32 + (lane & 31);
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        // Staging: element e = tid + 256 i of a stage is row e / W (channel kChunk G s + row), column e % W; a thread walks its elements
        // without dividing again.  The loads of stage s + 1 are issued when stage s begins and land in registers while its MFMAs run.
        const int r0 = tid / W, col0 = tid - r0 * W, rq = 256 / W, cq = 256 - rq * W;
        float pf[kWnSlots];
        auto stage_load = [&](int s) {
            int r = r0, col = col0;
            static_for<kWnSlots>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                float v = 0.f;
                if (tid + 256 * i < total) {
                    const int ci = s * G * kChunk + r, t = tbase + col;
                    if constexpr (STREAM) {
                        if (ci < p.Cin && t >= lo && t < len) v = xb[(long long)ci * p.x_cstride + ((t - xorg) & p.xs.mask)];
                    } else {
                        if (ci < p.Cin && t >= 0 && t < len) v = xb[(long long)ci * p.x_cstride + t];     // the conv's zero padding and the row's length
                    }
                }
                pf[i] = v;
                r += rq, col += cq;
                if (col >= W) col -= W, ++r;
            });
        };
        auto stage_store = [&](int s) {
            float* dst = wn_xs + (s & 1) * total + tid;
            static_for<kWnSlots>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if (tid + 256 * i < total) dst[256 * i] = pf[i];
            });
        };
        // Weights: the fragments of a pair are contiguous over (chunk, tap), so they come through a ring of kWnRing float4 pairs, that
        // many (chunk, tap) steps ahead of the MFMAs that use them
        const int nf = p.nchunk * ks;
        const float4* __restrict__ wf = p.wp + (long long)pair * nf * 128 + lane;
        float4 ra0[kWnRing], ra1[kWnRing];
        static_for<kWnRing>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            ra0[i] = do0 && i < nf ? wf[i * 128] : zero4;
            ra1[i] = do1 && i < nf ? wf[i * 128 + 64] : zero4;
        });
        stage_load(0);
        int s = 0, cs = 0, j = 0;            // flat step f = (chunk G s + cs, tap j)
        for (int f0 = 0; f0 < nf; f0 += kWnRing) {
            static_for<kWnRing>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const int f = f0 + i;
                if (f >= nf) return;
                if (cs == 0 && j == 0) {             // a stage begins (block-uniform): its values go into the buffer that stage s - 2 has left
                    stage_store(s);
                    __syncthreads();
                    if (s + 1 < nstage) stage_load(s + 1);
                }
                if (do0 || do1) {
                    const float* xsb = wn_xs + (s & 1) * total + cs * kChunk * W + b_lane + j * dil;
                    const float4 a0 = ra0[i], a1 = ra1[i];
                    float bv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) bv[q] = xsb[2 * q * W];
                    ra0[i] = do0 && f + kWnRing < nf ? wf[(f + kWnRing) * 128] : zero4;
                    ra1[i] = do1 && f + kWnRing < nf ? wf[(f + kWnRing) * 128 + 64] : zero4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float av0 = q == 0 ? a0.x : q == 1 ? a0.y : q == 2 ? a0.z : a0.w;
                        const float av1 = q == 0 ? a1.x : q == 1 ? a1.y : q == 2 ? a1.z : a1.w;
                        if (do0) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv[q], acc0, 0, 0, 0);
                        if (do1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv[q], acc1, 0, 0, 0);
                    }
                }
                if (++j == ks) {
                    j = 0;
                    if (++cs == G) cs = 0, ++s;
                }
            });
        }
    }

    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= Tend || pair >= p.npairs) return;
    const bool valid = n < len;
    const float* __restrict__ bias0 = p.bias;
    const float* __restrict__ bias1 = p.bias + 32 * p.npairs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = pair * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const long long o0 = STREAM ? at(p.y0s, p.M0, m, n) : (b * p.M0 + m) * p.T + n;
        const long long o1 = STREAM ? at(p.y1s, p.M1, m, n) : (b * p.M1 + m) * p.T + n;
        if (MODE == WN_GATE) {
            if (valid && m < p.M0) {
                const float t = tanhf(acc0[r] + bias0[m]);
                const float s = 1.f / (1.f + expf(-(acc1[r] + bias1[m])));
                p.y0[o0] = t * s;
            }
        } else if (MODE == WN_RES_SKIP) {
            if (!valid) continue;
            if constexpr (STREAM) {
                if (m < p.M0) p.y0[o0] = p.res[at(p.rs, p.M0, m, n)] + (acc0[r] + bias0[m]);     // h_{i + 1} = h_i + r, from ring to ring
            } else {
                if (m < p.M0) p.y0[o0] = p.y0[o0] + (acc0[r] + bias0[m]);           // the same lane reads and writes the element
            }
            if (m < p.M1) {
                const float v = acc1[r] + bias1[m];
                p.y1[o1] = p.first ? v : p.y1[o1] + v;
            }
        } else if (MODE == WN_PRE) {
            if (valid && m < p.M0) p.y0[o0] = acc0[r] + bias0[m];
        } else {
            if (m < p.M0) {
                const float v = valid ? acc0[r] + bias0[m] : 0.f;
                if (p.z) {
                    const float mean = p.bn_scale ? fmaf(v, p.bn_scale[m], p.bn_shift[m]) : v;     // after the mask: a padded frame holds shift
                    if (p.y0) p.y0[o0] = POOL && !valid ? 0.f : mean;      // a pool's rows hold exact zeros past an item's frames
                    p.z[o0] = valid ? mean : 0.f;
                } else {
                    p.y0[o0] = v;
                }
            }
            if (m < p.M1 && p.y1) {
                const float v = valid ? acc1[r] + bias1[m] : 0.f;
                p.y1[o1] = fminf(fmaxf(v, -30.f), 20.f);
            }
        }
    }
}

template <int WN, int KS, int DIL>
__global__ __launch_bounds__(256) void wn_gate_kernel(const WnParams p, const WnRowBlock rows) { wn_body<WN_GATE, WN, KS, DIL>(p, rows); }
template <int WN>
__global__ __launch_bounds__(256) void wn_res_skip_kernel(const WnParams p, const WnRowBlock rows) { wn_body<WN_RES_SKIP, WN, 1, 1>(p, rows); }
template <int WN>
__global__ __launch_bounds__(256) void wn_pre_kernel(const WnParams p, const WnRowBlock rows) { wn_body<WN_PRE, WN, 1, 1>(p, rows); }
template <int WN>
__global__ __launch_bounds__(256) void wn_proj_kernel(const WnParams p, const WnRowBlock rows) { wn_body<WN_PROJ, WN, 1, 1>(p, rows); }
// The stream forms take no row table: every row of a stream holds the same frames
template <int MODE, int WN, int KS, int DIL>
__global__ __launch_bounds__(256) void wn_stream_kernel(const WnParams p) { wn_body<MODE, WN, KS, DIL, WN_STREAM>(p, WnRowBlock{}); }
// The pool forms: one table entry per item of the step
template <int MODE, int WN, int KS, int DIL>
__global__ __launch_bounds__(256) void wn_pool_kernel(const WnParams p, const WnPoolBlock rows) { wn_body<MODE, WN, KS, DIL, WN_POOL>(p, rows); }

// Chunks per stage: as many as keep a stage inside the threads' kWnSlots registers, which is also half the LDS budget (two stages)
int wn_stage_chunks(int cols, int ks, int dil) {
    const int W = cols + (ks - 1) * dil;
    return std::max(1, std::min(kWnMaxStageChunks, 256 * kWnSlots / (kChunk * W)));
}
size_t wn_lds_bytes(int cols, int ks, int dil, int G) { return (size_t)2 * G * kChunk * (cols + (size_t)(ks - 1) * dil) * sizeof(float); }
static_assert((size_t)2 * 256 * kWnSlots * sizeof(float) <= kWnLdsBudget, "two stages of 256 kWnSlots floats are the LDS budget");

template <int MODE, int KS, int DIL>
void wn_launch(WnParams p, const WnRowBlock& rows, int nrows, hipStream_t s) {
    const bool narrow = p.T <= kWnNarrowMaxT;
    const int cols = narrow ? 32 : kWnWideCols, wm = narrow ? 4 : 1;
    const dim3 grid((unsigned)((p.T + cols - 1) / cols), (unsigned)((p.npairs + wm - 1) / wm), (unsigned)nrows);
    p.G = wn_stage_chunks(cols, p.ks, p.dil);
    const size_t lds = wn_lds_bytes(cols, p.ks, p.dil, p.G);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, p, rows); };
    if (MODE == WN_GATE) narrow ? go(wn_gate_kernel<1, KS, DIL>) : go(wn_gate_kernel<4, KS, DIL>);
    else if (MODE == WN_RES_SKIP) narrow ? go(wn_res_skip_kernel<1>) : go(wn_res_skip_kernel<4>);
    else if (MODE == WN_PRE) narrow ? go(wn_pre_kernel<1>) : go(wn_pre_kernel<4>);
    else narrow ? go(wn_proj_kernel<1>) : go(wn_proj_kernel<4>);
}

// The frames [p.col0, p.T) of `nrows` rows; the tile is chosen by their count as wn_launch chooses it by T
template <int MODE, int KS, int DIL>
void wn_stream_launch(WnParams p, int nrows, hipStream_t s) {
    const int ncols = p.T - p.col0;
    const bool narrow = ncols <= kWnNarrowMaxT;
    const int cols = narrow ? 32 : kWnWideCols, wm = narrow ? 4 : 1;
    const dim3 grid((unsigned)((ncols + cols - 1) / cols), (unsigned)((p.npairs + wm - 1) / wm), (unsigned)nrows);
    p.G = wn_stage_chunks(cols, p.ks, p.dil);
    const size_t lds = wn_lds_bytes(cols, p.ks, p.dil, p.G);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, p); };
    narrow ? go(wn_stream_kernel<MODE, 1, KS, DIL>) : go(wn_stream_kernel<MODE, 4, KS, DIL>);
}

// The entries' frames of `nz` items; the grid is the widest entry's and the tile is chosen by its `ncols` columns, as wn_stream_launch does.
// p.col0, p.T and p.uniform are not read: they are the entries'.
template <int MODE, int KS, int DIL>
void wn_pool_launch(WnParams p, const WnPoolBlock& rows, int nz, int ncols, hipStream_t s) {
    const bool narrow = ncols <= kWnNarrowMaxT;
    const int cols = narrow ? 32 : kWnWideCols, wm = narrow ? 4 : 1;
    const dim3 grid((unsigned)((ncols + cols - 1) / cols), (unsigned)((p.npairs + wm - 1) / wm), (unsigned)nz);
    p.G = wn_stage_chunks(cols, p.ks, p.dil);
    const size_t lds = wn_lds_bytes(cols, p.ks, p.dil, p.G);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, p, rows); };
    narrow ? go(wn_pool_kernel<MODE, 1, KS, DIL>) : go(wn_pool_kernel<MODE, 4, KS, DIL>);
}

// One GEMM of the stack on the host side: the folded rows of its two halves, packed
struct WnGemm {
    int Cin = 0, ks = 1, M0 = 0, M1 = 0, npairs = 0, nchunk = 0;
    std::vector<float> packed, bias;
    float4* d_wp = nullptr;
    float* d_bias = nullptr;
};

// w: (M0 + M1, Cin, ks) folded rows, half 1 after half 0; b: (M0 + M1)
void wn_pack(WnGemm& g, const std::vector<float>& w, const std::vector<float>& b, int Cin, int ks, int M0, int M1) {
    g.Cin = Cin, g.ks = ks, g.M0 = M0, g.M1 = M1;
    g.npairs = (std::max(M0, M1) + 31) / 32;
    g.nchunk = (Cin + kChunk - 1) / kChunk;
    g.packed.assign((size_t)g.npairs * g.nchunk * ks * 2 * 64 * 4, 0.f);
    g.bias.assign((size_t)64 * g.npairs, 0.f);
    for (int half = 0; half < 2; ++half) {
        const int M = half ? M1 : M0, base = half ? M0 : 0;
        for (int m = 0; m < M; ++m) g.bias[(size_t)half * 32 * g.npairs + m] = b[base + m];
        for (int pr = 0; pr < g.npairs; ++pr)
            for (int c = 0; c < g.nchunk; ++c)
                for (int j = 0; j < ks; ++j)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < 4; ++q) {
                            const int m = 32 * pr + (lane & 31), ci = kChunk * c + 2 * q + (lane >> 5);
                            if (m < M && ci < Cin)
                                g.packed[(((((size_t)pr * g.nchunk + c) * ks + j) * 2 + half) * 64 + lane) * 4 + q] = w[((size_t)(base + m) * Cin + ci) * ks + j];
                        }
    }
}

struct WnTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

std::string shape_str(const int64_t* shape, int ndim) {
    std::string s = "(";
    for (int i = 0; i < ndim; ++i) s += (i ? ", " : "") + std::to_string((long long)shape[i]);
    return s + ")";
}

}  // namespace
}  // namespace fv

using namespace fv;

struct fv_posterior {
    fv_posterior_config cfg{};
    int reach = 0;
    std::vector<int> dil;                                   // per layer
    std::map<std::string, std::vector<int64_t>> expect;     // key -> shape
    std::vector<std::string> order;                         // the reference's key order (the first missing one is named)
    std::map<std::string, WnTensor> loaded;
    bool finalized = false;
    WnGemm pre, proj;
    std::vector<WnGemm> in_layers, rs_layers;
    float* d_bn = nullptr;                                  // scale (out_channels), then shift
    ~fv_posterior() {
        auto drop = [](WnGemm& g) {
            if (g.d_wp) (void)hipFree(g.d_wp);
            if (g.d_bias) (void)hipFree(g.d_bias);
        };
        drop(pre), drop(proj);
        for (auto& g : in_layers) drop(g);
        for (auto& g : rs_layers) drop(g);
        if (d_bn) (void)hipFree(d_bn);
    }
};

// The encoder chunk by chunk (fv_wnstream_*).  With p_i = (k - 1) d_i / 2 and lam[i] = p_0 + ... + p_{i - 1} (lam[n_layers] = R), layer i's
// input h_i is known up to frame N - lam[i] after N frames have arrived, and a push computes only the new columns of every layer.  h_i lives
// in a ring of its own: its next outputs still read the last 2 p_i frames below the frontier, and one call adds max(max_chunk, R) at the
// most (R: a flush takes every layer up to N), so nothing is copied between pushes.  `out`, the running skip sum, is a ring of the R frames
// that wait for their later layers plus one call's; g is linear, one call's columns.  One allocation holds them for `rows` rows: a stream's
// batch rows, or a pool's slots (g: its items).
namespace {
struct WnRings {
    std::vector<int> lam;               // n_layers + 1
    std::vector<float*> h;              // ring of h_i, (rows, C, hW[i])
    std::vector<int> hW;
    float* out = nullptr;               // (rows, C, outW)
    float* g = nullptr;                 // (rows, C, gW)
    int outW = 0, gW = 0;
    float* slab = nullptr;
    ~WnRings() {
        if (slab) (void)hipFree(slab);
    }
    // step: the most frames one call adds to a frontier
    fv_status create(const fv_posterior* p, int rows, long long step) {
        const int nl = p->cfg.n_layers, k = p->cfg.kernel_size, R = p->reach;
        lam.assign(nl + 1, 0);
        size_t frames = 0;                                         // per (row, channel)
        for (int i = 0; i < nl; ++i) {
            const int pad = (k - 1) * p->dil[i] / 2;
            lam[i + 1] = lam[i] + pad;
            int w = 1;
            while (w < 2LL * pad + step) w <<= 1;
            hW.push_back(w);
            frames += (size_t)w;
        }
        outW = 1;
        while (outW < R + step) outW <<= 1;
        gW = (int)step;
        frames += (size_t)outW + (size_t)gW;
        const size_t plane = (size_t)rows * (size_t)p->cfg.hidden_channels;
        FV_HIP_CHECK(hipMalloc(&slab, plane * frames * sizeof(float)));
        float* at = slab;
        for (int i = 0; i < nl; ++i) h.push_back(at), at += plane * (size_t)hW[i];
        out = at, at += plane * (size_t)outW;
        g = at;
        return FV_OK;
    }
};
}  // namespace

struct fv_wnstream : WnRings {
    fv_posterior* enc = nullptr;
    int batch = 0;
    FrameStream count;                  // frame_pool.h
};

// The encoder for `S` sessions that advance independently (fv_wnpool_*): the stream's rings with one row per slot, addressed by the slot's
// own absolute frame numbers, so a slot's state is its row of each ring and its counters; g has one row per item of a step.  A step fills
// one WnPoolEntry per item and launch from the item's (N, N', E, flush) and the layer's lam, wn_stream_advance's arithmetic per item, and a
// launch serves every item of a block.  An item may flush together with its last frames, so a layer advances by up to max_chunk + R frames
// in one step, where a stream's advances by max(max_chunk, R): the rings and g are sized for that.
struct fv_wnpool : WnRings {
    fv_posterior* enc = nullptr;
    FramePool count;                    // frame_pool.h
};

namespace {

fv_status wn_upload(WnGemm& g) {
    FV_HIP_CHECK(hipMalloc(&g.d_wp, g.packed.size() * 4));
    FV_HIP_CHECK(hipMalloc(&g.d_bias, g.bias.size() * 4));
    FV_HIP_CHECK(hipMemcpy(g.d_wp, g.packed.data(), g.packed.size() * 4, hipMemcpyHostToDevice));
    FV_HIP_CHECK(hipMemcpy(g.d_bias, g.bias.data(), g.bias.size() * 4, hipMemcpyHostToDevice));
    g.packed = std::vector<float>();
    g.bias = std::vector<float>();
    return FV_OK;
}

// nn.utils.weight_norm(name="weight"), dim 0: w[m] = g[m] v[m] / |v[m]|, in fp64, rounded once
std::vector<float> wn_fold(const std::vector<float>& g, const std::vector<float>& v, int M, size_t per_row) {
    std::vector<float> w((size_t)M * per_row);
    for (int m = 0; m < M; ++m) {
        double ss = 0.0;
        for (size_t i = 0; i < per_row; ++i) ss += (double)v[m * per_row + i] * (double)v[m * per_row + i];
        const double scale = (double)g[m] / std::sqrt(ss);
        for (size_t i = 0; i < per_row; ++i) w[m * per_row + i] = (float)((double)v[m * per_row + i] * scale);
    }
    return w;
}

fv_status wn_check_shape(const char* fn, const fv_posterior* p, int32_t batch, int64_t T) {
    if (!p) {
        set_error("%s: null encoder", fn);
        return FV_ERR_INVALID;
    }
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kWnMaxFrames || (long long)batch * T > kWnMaxFrames) {
        set_error("%s: T = %lld must be >= 0 and batch * T at most 2^30 frames", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

WnParams wn_params(const WnGemm& g, const float* x, long long x_bstride, long long x_cstride, int T, int dil) {
    WnParams q{};
    q.x = x, q.x_bstride = x_bstride, q.x_cstride = x_cstride;
    q.Cin = g.Cin, q.nchunk = g.nchunk;
    q.wp = g.d_wp, q.bias = g.d_bias;
    q.M0 = g.M0, q.M1 = g.M1, q.npairs = g.npairs;
    q.T = T, q.ks = g.ks, q.dil = dil;
    return q;
}

}  // namespace

extern "C" {

FV_API fv_status fv_posterior_create(const fv_posterior_config* cfg, fv_posterior** out) {
    const char* fn = "fv_posterior_create";
    if (!out || !cfg) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    auto range = [&](const char* name, int v, int lo, int hi) {
        if (v >= lo && v <= hi) return true;
        set_error("%s: %s = %d must lie in [%d, %d]", fn, name, v, lo, hi);
        return false;
    };
    if (!range("in_channels", cfg->in_channels, 1, kWnMaxIo) || !range("out_channels", cfg->out_channels, 1, kWnMaxIo) ||
        !range("hidden_channels", cfg->hidden_channels, 1, kWnMaxHidden) || !range("kernel_size", cfg->kernel_size, 1, kWnMaxKernel) ||
        !range("n_layers", cfg->n_layers, 1, kWnMaxLayers) || !range("mode", cfg->mode, 0, 2))
        return FV_ERR_INVALID;
    if (cfg->kernel_size % 2 == 0) {
        set_error("%s: kernel_size = %d must be odd (posterior_encoder.py:23)", fn, cfg->kernel_size);
        return FV_ERR_INVALID;
    }
    if (cfg->dilation_rate < 1) {
        set_error("%s: dilation_rate = %d must be >= 1", fn, cfg->dilation_rate);
        return FV_ERR_INVALID;
    }
    if (cfg->dilation_cycle < 1) {
        set_error("%s: dilation_cycle = %d must be >= 1", fn, cfg->dilation_cycle);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_posterior> p(new fv_posterior());
    p->cfg = *cfg;
    const int C = cfg->hidden_channels, k = cfg->kernel_size, nl = cfg->n_layers;
    const long long max_span = (long long)(kWnLdsBudget / (2 * kChunk * sizeof(float))) - kWnWideCols;      // (k - 1) d of the widest staged window
    for (int i = 0; i < nl; ++i) {
        long long d = 1;
        for (int e = 0; e < i % cfg->dilation_cycle && (k - 1) * d <= max_span; ++e) d *= cfg->dilation_rate;
        if ((k - 1) * d > max_span) {
            set_error("%s: dilation_rate = %d with dilation_cycle = %d gives layer %d a window of (kernel_size - 1) * dilation > %lld frames, "
                      "more than the staged window's LDS budget holds", fn, cfg->dilation_rate, cfg->dilation_cycle, i, max_span);
            return FV_ERR_UNSUPPORTED;
        }
        p->dil.push_back((int)d);
        p->reach += (int)((k - 1) * d / 2);
    }
    auto want = [&](const std::string& key, std::vector<int64_t> shape) {
        p->order.push_back(key);
        p->expect[key] = std::move(shape);
    };
    want("pre.weight", {C, cfg->in_channels, 1});
    want("pre.bias", {C});
    for (int i = 0; i < nl; ++i) {
        const std::string pfx = "enc.in_layers." + std::to_string(i);
        want(pfx + ".bias", {2 * C});
        want(pfx + ".weight_g", {2 * C, 1, 1});
        want(pfx + ".weight_v", {2 * C, C, k});
    }
    for (int i = 0; i < nl; ++i) {
        const std::string pfx = "enc.res_skip_layers." + std::to_string(i);
        const int R = i < nl - 1 ? 2 * C : C;
        want(pfx + ".bias", {R});
        want(pfx + ".weight_g", {R, 1, 1});
        want(pfx + ".weight_v", {R, C, 1});
    }
    const int O = cfg->mode == 0 ? cfg->out_channels : 2 * cfg->out_channels;
    want("proj.weight", {O, C, 1});
    want("proj.bias", {O});
    if (cfg->mode == 2)
        for (const char* n : {"mu_bn.weight", "mu_bn.bias", "mu_bn.running_mean", "mu_bn.running_var"}) want(n, {cfg->out_channels});
    *out = p.release();
    return FV_OK;
}

FV_API void fv_posterior_destroy(fv_posterior* p) { delete p; }

FV_API fv_status fv_posterior_load_weight(fv_posterior* p, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    const char* fn = "fv_posterior_load_weight";
    if (!p || !name || !host || ndim < 0 || (ndim > 0 && !shape)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (p->finalized) {
        set_error("%s: '%s' arrives after fv_posterior_finalize", fn, name);
        return FV_ERR_STATE;
    }
    if (p->cfg.mode == 2 && !strcmp(name, "mu_bn.num_batches_tracked")) return FV_OK;     // no eval arithmetic
    const auto it = p->expect.find(name);
    if (it == p->expect.end()) {
        set_error("%s: unknown key '%s'", fn, name);
        return FV_ERR_INVALID;
    }
    const std::vector<int64_t>& want = it->second;
    if ((size_t)ndim != want.size() || !std::equal(want.begin(), want.end(), shape)) {
        set_error("%s: '%s' has shape %s, expected %s", fn, name, shape_str(shape, ndim).c_str(), shape_str(want.data(), (int)want.size()).c_str());
        return FV_ERR_SHAPE;
    }
    size_t n = 1;
    for (int64_t v : want) n *= (size_t)v;
    WnTensor& t = p->loaded[name];
    t.shape = want;
    t.data.assign(host, host + n);
    return FV_OK;
}

FV_API fv_status fv_posterior_finalize(fv_posterior* p) {
    const char* fn = "fv_posterior_finalize";
    if (!p) {
        set_error("%s: null encoder", fn);
        return FV_ERR_INVALID;
    }
    if (p->finalized) {
        set_error("%s: already finalized", fn);
        return FV_ERR_STATE;
    }
    for (const std::string& key : p->order)
        if (!p->loaded.count(key)) {
            set_error("%s: missing weight '%s'", fn, key.c_str());
            return FV_ERR_MISSING_WEIGHT;
        }
    const fv_posterior_config& c = p->cfg;
    const int C = c.hidden_channels, k = c.kernel_size, nl = c.n_layers;
    auto data = [&](const std::string& key) -> const std::vector<float>& { return p->loaded[key].data; };
    wn_pack(p->pre, data("pre.weight"), data("pre.bias"), c.in_channels, 1, C, 0);
    p->in_layers.resize(nl), p->rs_layers.resize(nl);
    for (int i = 0; i < nl; ++i) {
        const std::string a = "enc.in_layers." + std::to_string(i), r = "enc.res_skip_layers." + std::to_string(i);
        wn_pack(p->in_layers[i], wn_fold(data(a + ".weight_g"), data(a + ".weight_v"), 2 * C, (size_t)C * k), data(a + ".bias"), C, k, C, C);
        const bool last = i == nl - 1;
        // the last layer's C rows are all "skip" rows: half 0 is empty
        wn_pack(p->rs_layers[i], wn_fold(data(r + ".weight_g"), data(r + ".weight_v"), last ? C : 2 * C, (size_t)C), data(r + ".bias"), C, 1, last ? 0 : C, C);
    }
    wn_pack(p->proj, data("proj.weight"), data("proj.bias"), C, 1, c.out_channels, c.mode == 0 ? 0 : c.out_channels);
    std::vector<float> bn;
    if (c.mode == 2) {
        bn.resize((size_t)2 * c.out_channels);
        for (int m = 0; m < c.out_channels; ++m) {
            const double scale = (double)data("mu_bn.weight")[m] / std::sqrt((double)data("mu_bn.running_var")[m] + kBnEps);
            bn[m] = (float)scale;
            bn[c.out_channels + m] = (float)((double)data("mu_bn.bias")[m] - (double)data("mu_bn.running_mean")[m] * scale);
        }
    }
    if (const fv_status st = wn_upload(p->pre)) return st;
    for (int i = 0; i < nl; ++i) {
        if (const fv_status st = wn_upload(p->in_layers[i])) return st;
        if (const fv_status st = wn_upload(p->rs_layers[i])) return st;
    }
    if (const fv_status st = wn_upload(p->proj)) return st;
    if (!bn.empty()) {
        FV_HIP_CHECK(hipMalloc(&p->d_bn, bn.size() * 4));
        FV_HIP_CHECK(hipMemcpy(p->d_bn, bn.data(), bn.size() * 4, hipMemcpyHostToDevice));
    }
    p->loaded.clear();
    p->finalized = true;
    return FV_OK;
}

FV_API int32_t fv_posterior_reach_frames(const fv_posterior* p) { return p ? p->reach : -1; }

FV_API int32_t fv_posterior_output_channels(const fv_posterior* p) { return p ? p->cfg.out_channels : -1; }

FV_API size_t fv_posterior_workspace_bytes(const fv_posterior* p, int32_t batch, int64_t T) {
    if (wn_check_shape("fv_posterior_workspace_bytes", p, batch, T)) return 0;
    return (size_t)3 * (size_t)batch * (size_t)p->cfg.hidden_channels * (size_t)T * sizeof(float);
}

FV_API fv_status fv_posterior_forward(fv_posterior* p, const float* d_x, int64_t x_row_stride, const int32_t* host_lengths, float* d_z,
                                      float* d_mean, float* d_logvar, int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes,
                                      void* stream) {
    const char* fn = "fv_posterior_forward";
    if (const fv_status st = wn_check_shape(fn, p, batch, T)) return st;
    if (!p->finalized) {
        set_error("%s: the encoder has not been finalized (fv_posterior_finalize)", fn);
        return FV_ERR_STATE;
    }
    if (p->cfg.mode == 0 && (d_mean || d_logvar)) {
        set_error("%s: %s must be NULL in vqvae mode (posterior_encoder.py:159-160 returns one tensor)", fn, d_mean ? "d_mean" : "d_logvar");
        return FV_ERR_INVALID;
    }
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_x || !d_z) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : "d_z");
        return FV_ERR_INVALID;
    }
    if (x_row_stride < T) {
        set_error("%s: x_row_stride = %lld (the stride between channels) is shorter than a row of T = %lld frames", fn, (long long)x_row_stride,
                  (long long)T);
        return FV_ERR_INVALID;
    }
    const size_t need = fv_posterior_workspace_bytes(p, batch, T);
    if (workspace_bytes < need || !d_workspace) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_posterior_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, need, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    for (int b = 0; host_lengths && b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > T) {
            set_error("%s: host_lengths[%d] = %d lies outside [0, T = %lld]", fn, b, host_lengths[b], (long long)T);
            return FV_ERR_INVALID;
        }
    // everything is validated: enqueue

    const fv_posterior_config& c = p->cfg;
    const int C = c.hidden_channels, nl = c.n_layers, Ti = (int)T;
    const size_t plane = (size_t)batch * C * (size_t)T;
    float* h = (float*)d_workspace;
    float* g = h + plane;
    float* out = g + plane;
    hipStream_t s = (hipStream_t)stream;
    const long long cstride = (long long)C * T;
    const bool k5 = c.kernel_size == 5;

    auto block = [&](const WnRowBlock& rows, int row0, int nrows, int uniform) -> fv_status {
        auto with_rows = [&](WnParams q) {
            q.row0 = row0, q.uniform = uniform;
            return q;
        };
        {
            WnParams q = with_rows(wn_params(p->pre, d_x, (long long)c.in_channels * x_row_stride, x_row_stride, Ti, 1));
            q.y0 = h;
            wn_launch<WN_PRE, 1, 1>(q, rows, nrows, s);
        }
        for (int i = 0; i < nl; ++i) {
            WnParams q = with_rows(wn_params(p->in_layers[i], h, cstride, T, Ti, p->dil[i]));
            q.y0 = g;
            if (k5 && p->dil[i] == 1) wn_launch<WN_GATE, 5, 1>(q, rows, nrows, s);
            else wn_launch<WN_GATE, 0, 0>(q, rows, nrows, s);
            WnParams r = with_rows(wn_params(p->rs_layers[i], g, cstride, T, Ti, 1));
            r.y0 = h, r.y1 = out, r.first = i == 0;
            wn_launch<WN_RES_SKIP, 1, 1>(r, rows, nrows, s);
        }
        WnParams q = with_rows(wn_params(p->proj, out, cstride, T, Ti, 1));
        if (c.mode == 0) {
            q.y0 = d_z;
        } else {
            q.y0 = d_mean, q.y1 = d_logvar, q.z = d_z;
            if (c.mode == 2) q.bn_scale = p->d_bn, q.bn_shift = p->d_bn + c.out_channels;
        }
        wn_launch<WN_PROJ, 1, 1>(q, rows, nrows, s);
        return FV_OK;
    };
    fv_status st;
    if (host_lengths) {
        st = for_each_launch_table<WnRowBlock>(batch, host_lengths, [&](const WnRowBlock& rows, int row0, int nrows) { return block(rows, row0, nrows, -1); });
    } else {
        st = block(WnRowBlock{}, 0, batch, Ti);        // every row holds T frames: one block over all rows, the zeroed table is never read
        if (st == FV_OK) FV_HIP_CHECK(hipGetLastError());
    }
    if (st == FV_OK) set_last_kernel(Ti <= kWnNarrowMaxT ? "wn_gate_kernel<1>" : "wn_gate_kernel<4>");
    return st;
}

}  // extern "C"

namespace {

// One push (c frames of d_x) or the flush: validates, then enqueues at most 2 n_layers + 2 launches and moves the counters
fv_status wn_stream_advance(const char* fn, fv_wnstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c, bool flush,
                            float* d_z, float* d_mean, float* d_logvar, int64_t y_row_stride, int64_t* emitted, void* stream) {
    if (const fv_status rs = frame_stream_chunk(fn, "fv_wnstream_reset", s ? &s->count : nullptr, c)) return rs;
    const fv_posterior* p = s->enc;
    const fv_posterior_config& cfg = p->cfg;
    if (cfg.mode == 0 && (d_mean || d_logvar)) {
        set_error("%s: %s must be NULL in vqvae mode (posterior_encoder.py:159-160 returns one tensor)", fn, d_mean ? "d_mean" : "d_logvar");
        return FV_ERR_INVALID;
    }
    if (const fv_status rs = s->count.input(fn, d_x, x_batch_stride, x_row_stride, c)) return rs;
    long long N1, E1;
    if (const fv_status rs = s->count.output(fn, "d_z", c, flush, d_z != nullptr, y_row_stride, &N1, &E1)) return rs;
    const int nl = cfg.n_layers, C = cfg.hidden_channels, B = s->batch;
    const long long N0 = s->count.N, E0 = s->count.E, k = E1 - E0;
    // everything is validated: enqueue

    hipStream_t st = (hipStream_t)stream;
    const bool k5 = cfg.kernel_size == 5;
    auto ring = [](int W) { return WnSpan{W, 0, W - 1}; };
    auto linear = [](long long stride, long long org) { return WnSpan{stride, (int)org, -1}; };
    auto clamp0 = [](long long v) { return (int)std::max(0LL, v); };
    bool any = false;
    if (c > 0) {        // h_0 = pre(x) over the new frames
        WnParams q = wn_params(p->pre, d_x, x_batch_stride, x_row_stride, (int)N1, 1);
        q.col0 = q.lo = (int)N0, q.uniform = (int)N1, q.xs = linear(x_row_stride, N0);
        q.y0 = s->h[0], q.y0s = ring(s->hW[0]);
        wn_stream_launch<WN_PRE, 1, 1>(q, B, st);
        any = true;
    }
    for (int i = 0; i < nl; ++i) {
        // the new columns of h_{i + 1} and skip_i; the flush takes every layer up to N, reading zeros from there on
        const int n0 = clamp0(N0 - s->lam[i + 1]), n1 = flush ? (int)N1 : clamp0(N1 - s->lam[i + 1]);
        if (n1 <= n0) continue;
        const int front = flush ? (int)N1 : clamp0(N1 - s->lam[i]);         // h_i's frontier: a ring holds an earlier lap's frame past it
        WnParams q = wn_params(p->in_layers[i], s->h[i], (long long)C * s->hW[i], s->hW[i], n1, p->dil[i]);
        q.col0 = n0, q.lo = 0, q.uniform = front, q.xs = ring(s->hW[i]);
        q.y0 = s->g, q.y0s = linear(s->gW, n0);
        if (k5 && p->dil[i] == 1) wn_stream_launch<WN_GATE, 5, 1>(q, B, st);
        else wn_stream_launch<WN_GATE, 0, 0>(q, B, st);
        WnParams r = wn_params(p->rs_layers[i], s->g, (long long)C * s->gW, s->gW, n1, 1);
        r.col0 = r.lo = n0, r.uniform = n1, r.xs = linear(s->gW, n0);
        r.res = s->h[i], r.rs = ring(s->hW[i]);
        if (i + 1 < nl) r.y0 = s->h[i + 1], r.y0s = ring(s->hW[i + 1]);
        r.y1 = s->out, r.y1s = ring(s->outW), r.first = i == 0;
        wn_stream_launch<WN_RES_SKIP, 1, 1>(r, B, st);
        any = true;
    }
    if (k > 0) {
        WnParams q = wn_params(p->proj, s->out, (long long)C * s->outW, s->outW, (int)E1, 1);
        q.col0 = (int)E0, q.lo = 0, q.uniform = (int)E1, q.xs = ring(s->outW);
        q.y0s = q.y1s = linear(y_row_stride, E0);
        if (cfg.mode == 0) {
            q.y0 = d_z;
        } else {
            q.y0 = d_mean, q.y1 = d_logvar, q.z = d_z;
            if (cfg.mode == 2) q.bn_scale = p->d_bn, q.bn_shift = p->d_bn + cfg.out_channels;
        }
        wn_stream_launch<WN_PROJ, 1, 1>(q, B, st);
        any = true;
    }
    if (any) {
        FV_HIP_CHECK(hipGetLastError());
        set_last_kernel("wn_stream_kernel");
    }
    s->count.commit(N1, E1, flush, emitted);
    return FV_OK;
}

}  // namespace

extern "C" {

FV_API fv_status fv_wnstream_create(fv_posterior* p, int32_t batch, int32_t max_chunk, fv_wnstream** out) {
    const char* fn = "fv_wnstream_create";
    if (!out || !p) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!p->finalized) {
        set_error("%s: the encoder has not been finalized (fv_posterior_finalize)", fn);
        return FV_ERR_STATE;
    }
    if (batch < 1 || batch > 65535) {
        set_error("%s: batch = %d must lie in [1, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (max_chunk < 1 || max_chunk > (1 << 20)) {
        set_error("%s: max_chunk = %d must lie in [1, 2^20]", fn, max_chunk);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_wnstream> s(new fv_wnstream());
    s->enc = p, s->batch = batch;
    s->count.max_chunk = max_chunk, s->count.R = p->reach;
    if (const fv_status st = s->create(p, batch, std::max(max_chunk, p->reach))) return st;
    *out = s.release();
    return FV_OK;
}

FV_API fv_status fv_wnstream_push(fv_wnstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c, float* d_z,
                                  float* d_mean, float* d_logvar, int64_t y_row_stride, int64_t* emitted, void* stream) {
    return wn_stream_advance("fv_wnstream_push", s, d_x, x_batch_stride, x_row_stride, c, false, d_z, d_mean, d_logvar, y_row_stride, emitted, stream);
}

FV_API fv_status fv_wnstream_flush(fv_wnstream* s, float* d_z, float* d_mean, float* d_logvar, int64_t y_row_stride, int64_t* emitted,
                                   void* stream) {
    return wn_stream_advance("fv_wnstream_flush", s, nullptr, 0, 0, 0, true, d_z, d_mean, d_logvar, y_row_stride, emitted, stream);
}

FV_API fv_status fv_wnstream_reset(fv_wnstream* s) {
    return frame_stream_reset("fv_wnstream_reset", s ? &s->count : nullptr);
}

FV_API int64_t fv_wnstream_pending(const fv_wnstream* s) { return s ? s->count.pending() : -1; }

FV_API int32_t fv_wnstream_lookahead(const fv_wnstream* s) { return s ? s->count.R : -1; }

FV_API void fv_wnstream_destroy(fv_wnstream* s) { delete s; }

}  // extern "C"

extern "C" {

FV_API fv_status fv_wnpool_create(fv_posterior* p, int32_t sessions, int32_t max_chunk, fv_wnpool** out) {
    const char* fn = "fv_wnpool_create";
    if (!out || !p) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!p->finalized) {
        set_error("%s: the encoder has not been finalized (fv_posterior_finalize)", fn);
        return FV_ERR_STATE;
    }
    if (const fv_status st = FramePool::range(fn, sessions, max_chunk)) return st;
    std::unique_ptr<fv_wnpool> s(new fv_wnpool());
    s->enc = p;
    s->count.init(sessions, max_chunk, p->reach);
    // an item may flush with its last frames: its layers then advance by max_chunk + lam[i + 1] <= max_chunk + R frames in one step
    if (const fv_status st = s->create(p, sessions, (long long)max_chunk + p->reach)) return st;
    *out = s.release();
    return FV_OK;
}

FV_API int64_t fv_wnpool_plan(int32_t reach, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                              const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out) {
    return FramePool::plan("fv_wnpool_plan", "fv_wnpool_reset", reach, sessions, max_chunk, received, emitted, flushed, items, count, frames_out);
}

FV_API fv_status fv_wnpool_step(fv_wnpool* p, const fv_wavpool_item* items, int32_t count, const float* d_x, int64_t x_item_stride,
                                int64_t x_row_stride, float* d_z, float* d_mean, float* d_logvar, int32_t out_cols, int64_t* frames_out,
                                void* stream) {
    const char* fn = "fv_wnpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    const fv_posterior* enc = p->enc;
    const fv_posterior_config& cfg = enc->cfg;
    if (cfg.mode == 0 && (d_mean || d_logvar)) {
        set_error("%s: %s must be NULL in vqvae mode (posterior_encoder.py:159-160 returns one tensor)", fn, d_mean ? "d_mean" : "d_logvar");
        return FV_ERR_INVALID;
    }
    const FramePool& fc = p->count;
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status st = fc.admit(fn, "fv_wnpool_reset", items, count, d_x, x_row_stride, N2.data(), E2.data())) return st;
    if (const fv_status st = fc.output(fn, "d_z", items, count, d_x, x_item_stride, E2.data(), d_z != nullptr, out_cols)) return st;
    // everything is validated: enqueue

    hipStream_t st = (hipStream_t)stream;
    const int nl = cfg.n_layers, C = cfg.hidden_channels;
    const bool k5 = cfg.kernel_size == 5;
    auto ring = [](int W) { return WnSpan{W, 0, W - 1}; };
    auto linear = [](long long stride) { return WnSpan{stride, 0, -1}; };       // the origin is the entry's col0
    auto clamp0 = [](long long v) { return (int)std::max(0LL, v); };
    int launches = 0;
    const fv_status rs = for_each_launch_table<WnPoolBlock>(
        count, [&](int i) { return WnPoolEntry{items[i].session, 0, 0, 0}; }, [&](const WnPoolBlock& slots, int first, int nz) -> fv_status {
            WnPoolBlock t = slots;
            // the table of one launch: cols(item, N, N', flush) -> {col0, end, frontier}; returns the widest entry's columns
            auto table = [&](auto&& cols) {
                int widest = 0;
                for (int i = 0; i < nz; ++i) {
                    const int item = first + i;
                    const WnPoolEntry e = cols(item, (long long)fc.N[(size_t)items[item].session], N2[(size_t)item], items[item].flush != 0);
                    t.e[i].col0 = e.col0, t.e[i].end = e.end, t.e[i].front = e.front;
                    widest = std::max(widest, e.end - e.col0);
                }
                return widest;
            };
            auto rows = [&](WnParams q) {
                q.row0 = first;
                return q;
            };
            // h_0 = pre(x) over every item's new frames
            if (const int w = table([&](int, long long N0, long long N1, bool) { return WnPoolEntry{0, (int)N0, (int)N1, (int)N1}; })) {
                WnParams q = rows(wn_params(enc->pre, d_x, x_item_stride, x_row_stride, 0, 1));
                q.lo = 1, q.xs = linear(x_row_stride);
                q.y0 = p->h[0], q.y0s = ring(p->hW[0]);
                wn_pool_launch<WN_PRE, 1, 1>(q, t, nz, w, st);
                ++launches;
            }
            for (int i = 0; i < nl; ++i) {
                // the new columns of h_{i + 1} and skip_i per item; a flush takes every layer up to N', reading zeros from there on
                const int lam0 = p->lam[i], lam1 = p->lam[i + 1];
                const int w = table([&](int, long long N0, long long N1, bool flush) {
                    return WnPoolEntry{0, clamp0(N0 - lam1), flush ? (int)N1 : clamp0(N1 - lam1), flush ? (int)N1 : clamp0(N1 - lam0)};
                });
                if (w == 0) continue;
                WnParams q = rows(wn_params(enc->in_layers[i], p->h[i], (long long)C * p->hW[i], p->hW[i], 0, enc->dil[i]));
                q.lo = 0, q.xs = ring(p->hW[i]);
                q.y0 = p->g, q.y0s = linear(p->gW);
                if (k5 && enc->dil[i] == 1) wn_pool_launch<WN_GATE, 5, 1>(q, t, nz, w, st);
                else wn_pool_launch<WN_GATE, 0, 0>(q, t, nz, w, st);
                for (int e = 0; e < nz; ++e) t.e[e].front = t.e[e].end;         // g holds exactly the new columns
                WnParams r = rows(wn_params(enc->rs_layers[i], p->g, (long long)C * p->gW, p->gW, 0, 1));
                r.lo = 1, r.xs = linear(p->gW);
                r.res = p->h[i], r.rs = ring(p->hW[i]);
                if (i + 1 < nl) r.y0 = p->h[i + 1], r.y0s = ring(p->hW[i + 1]);
                r.y1 = p->out, r.y1s = ring(p->outW), r.first = i == 0;
                wn_pool_launch<WN_RES_SKIP, 1, 1>(r, t, nz, w, st);
                launches += 2;
            }
            if (out_cols > 0) {     // every row's out_cols columns: the item's frames [E, E'), then zeros
                table([&](int item, long long, long long, bool) {
                    const long long E0 = fc.E[(size_t)items[item].session];
                    return WnPoolEntry{0, (int)E0, (int)(E0 + out_cols), (int)E2[(size_t)item]};
                });
                WnParams q = rows(wn_params(enc->proj, p->out, (long long)C * p->outW, p->outW, 0, 1));
                q.lo = 0, q.xs = ring(p->outW);
                q.y0s = q.y1s = linear(out_cols);
                if (cfg.mode == 0) {
                    q.y0 = d_z;
                } else {
                    q.y0 = d_mean, q.y1 = d_logvar, q.z = d_z;
                    if (cfg.mode == 2) q.bn_scale = enc->d_bn, q.bn_shift = enc->d_bn + cfg.out_channels;
                }
                wn_pool_launch<WN_PROJ, 1, 1>(q, t, nz, out_cols, st);
                ++launches;
            }
            return FV_OK;
        });
    if (rs != FV_OK) return rs;
    if (launches) set_last_kernel("wn_pool_kernel");
    p->count.commit(items, count, N2.data(), E2.data(), frames_out, launches);
    return FV_OK;
}

FV_API fv_status fv_wnpool_reset(fv_wnpool* p, int32_t session) {
    return frame_pool_reset("fv_wnpool_reset", p ? &p->count : nullptr, session);
}

FV_API int64_t fv_wnpool_received(const fv_wnpool* p, int32_t session) { return p ? p->count.received(session) : -1; }

FV_API int64_t fv_wnpool_emitted(const fv_wnpool* p, int32_t session) { return p ? p->count.emitted(session) : -1; }

FV_API int64_t fv_wnpool_pending(const fv_wnpool* p, int32_t session) { return p ? p->count.pending(session) : -1; }

FV_API int32_t fv_wnpool_lookahead(const fv_wnpool* p) { return p ? p->count.R : -1; }

FV_API int64_t fv_wnpool_max_frames(const fv_wnpool* p) { return p ? p->count.max_frames() : -1; }

FV_API int32_t fv_wnpool_launches(const fv_wnpool* p) { return p ? p->count.launches : -1; }

FV_API void fv_wnpool_destroy(fv_wnpool* p) { delete p; }

}  // extern "C"
