// Vector quantiser / residual vector quantiser (include/fishvoc.h fv_vq_*): the stage between generator.encoder and generator.decoder of the
// reference's VQVAEModel (fish_vocoder/models/vae.py:66-87) and the `vq` slot of UnifyGenerator (unify.py:21-53).  Inference arithmetic of
// encodec's core_vq, restated:
//   search(x, embed):  argmax_j s_j,  s_j = x . e_j - h_j,  h_j = 0.5 |e_j|^2 (fp64 at load, rounded to fp32); lowest index on equal scores,
//                      a NaN score never wins, code 0 when every score is NaN
//   r_0 = x;  c_q = search(r_q, embed_q);  r_{q+1} = r_q - e_{c_q};  z = ((e_{c_0} + e_{c_1}) + ...)          all fp32, one rounding per op
//
// vq_search_kernel: fp32 MFMA (v_mfma_f32_32x32x2_f32) with the CODEBOOK on the A operand (rows = codes) and the FRAMES on the B operand
//   (B[k = d][j = t]: lanes run along contiguous t of the (B, D, T) activation).  The 32x32 accumulator keeps a column on the lane and rows
//   in its 16 registers, so a lane holds 16 codes of ONE frame: the running (best score, best index) lives in the lane across registers and
//   code tiles, and only the two lane halves and the four waves are merged at the end.  Grid = frame tiles x codebook slices; a workgroup
//   writes one (score, index) partial per frame and slice.
// Invariance: s_j of a (frame, code) pair is one MFMA accumulator chain over d = 0 .. D-1 in steps of 2 from 0, then one subtraction of h_j:
//   an order that depends on D alone (zero products of the padding add exact zeros), never on the frame count, the frame's column, the code's
//   tile or the slice.  (greater score, then lower index) is associative and commutative, so codes and z have the same bits for a frame
//   alone, in any batch, under any chunking along T and any slice count.
// vq_select_kernel: per frame reduces the slice partials, stores the code, writes r_{q+1} and adds e_code into z.
// vq_gather_kernel: codes (n_q, B, T) -> z (B, D, T), the same layer-ordered sum.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

#include "fv_internal.h"

namespace fv {
namespace {

typedef float vq_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kVqMaxDim = 4096, kVqMaxCodes = 65536, kVqMaxLayers = 32;
constexpr int kVqRows = 256;                 // rows per launch: their lengths are a LaunchTable (fv_internal.h)
constexpr int kVqMT = 2;                     // 32-code tiles per wave and pass
constexpr int kVqGroup = 4;                  // chunks of 8 channels a wave requests at once (vq_search_kernel)
constexpr int kVqUnit = 4 * kVqMT;           // code tiles one pass of a workgroup's four waves covers: the slicing granule
constexpr int kVqSelFrames = 32, kVqSelD = 64;
constexpr int kNoCode = 0x7fffffff;          // "no score won yet": every NaN-free score beats it, a frame left with it takes code 0
constexpr long long kVqMaxFrames = 1LL << 30;

using VqRowBlock = LaunchTable<int, kVqRows>;

// Where the frames of a launch live: element (b, d, t) at b * bstride + d * dstride + t; rows [row0, row0 + rows) of the batch
struct VqFrames {
    long long bstride, dstride;
    int T, row0, rows;
    int uniform;      // >= 0: every row holds this many frames and `len` is not read
};

__device__ __forceinline__ bool vq_better(float s, int j, float bs, int bj) { return s > bs || (s == bs && j < bj); }

// NT = 32-frame tiles per workgroup (2 where the launch has frames enough to fill the chip with them: vq_plan)
template <int NT>
__global__ __launch_bounds__(256) void vq_search_kernel(const float* __restrict__ x, VqFrames fr, VqRowBlock rows, const float4* __restrict__ packed,
                                                        const float* __restrict__ h, int D, int K, int nchunk, int ktiles, int units_per_slice,
                                                        float* __restrict__ part_s, int* __restrict__ part_i, long long n_first, long long n_pad) {
    constexpr int MT = kVqMT;
    __shared__ float sh_s[4][NT * 32];
    __shared__ int sh_i[4][NT * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const long long nloc0 = (long long)blockIdx.x * (NT * 32);       // first frame of the tile, counted inside this row block
    const long long count = (long long)fr.rows * fr.T;
    const int slice = blockIdx.y;

    long long off[NT];
    bool ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const long long n = nloc0 + j * 32 + col;
        ok[j] = false;
        off[j] = 0;
        if (n < count) {
            const int bl = (int)(n / fr.T), t = (int)(n - (long long)bl * fr.T);
            const int len = fr.uniform >= 0 ? fr.uniform : rows.e[bl];
            ok[j] = t < len;                                           // frames at or past the row's length are never loaded
            off[j] = (long long)(fr.row0 + bl) * fr.bstride + t + (long long)half * fr.dstride;
        }
    }
    float best_s[NT];
    int best_i[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) best_s[j] = -INFINITY, best_i[j] = kNoCode;

    const int ct_end = min(ktiles, (slice + 1) * units_per_slice * kVqUnit);
    for (int ct = slice * units_per_slice * kVqUnit + wave * MT; ct < ct_end; ct += kVqUnit) {
        vq_f32x16 acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        bool tile_ok[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) tile_ok[i] = ct + i < ktiles;    // wave-uniform
        // Operands come straight from L2 (one 16-byte A load per tile and four B dwords per frame tile feed a chunk of 8 channels, 4 MFMAs per
        // accumulator) in groups of G chunks, one group ahead of the MFMAs that use them: a wave alone on its SIMD has the MFMA time
        // of a whole group to cover the loads' latency.  (The packed codebook is zero padded to whole groups.)
        constexpr int G = kVqGroup;
        float4 a0[G][MT], a1[G][MT];
        float b0[G][4][NT], b1[G][4][NT];
        auto load_group = [&](int g, float4 (&a)[G][MT], float (&b)[G][4][NT]) {
#pragma unroll
            for (int cc = 0; cc < G; ++cc) {
                const int c = G * g + cc;
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    a[cc][i] = tile_ok[i] ? packed[((long long)(ct + i) * nchunk + c) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int d = 8 * c + 2 * p + half;
#pragma unroll
                    for (int j = 0; j < NT; ++j) b[cc][p][j] = (ok[j] && d < D) ? x[off[j] + (long long)(8 * c + 2 * p) * fr.dstride] : 0.f;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto mfma_group = [&](const float4 (&a)[G][MT], const float (&b)[G][4][NT]) {
#pragma unroll
            for (int cc = 0; cc < G; ++cc) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        const float av = p == 0 ? a[cc][i].x : (p == 1 ? a[cc][i].y : (p == 2 ? a[cc][i].z : a[cc][i].w));
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[cc][p][j], acc[i][j], 0, 0, 0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        const int ngroup = nchunk / G;      // host: nchunk is a multiple of kVqGroup
        load_group(0, a0, b0);
        for (int g = 0; g < ngroup; g += 2) {
            if (g + 1 < ngroup) load_group(g + 1, a1, b1);
            mfma_group(a0, b0);
            if (g + 1 < ngroup) {
                if (g + 2 < ngroup) load_group(g + 2, a0, b0);
                mfma_group(a1, b1);
            }
        }
        // accumulator register r of lane l: code row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, frame column l & 31
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int code = (ct + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const bool cok = code < K;
                const float hv = cok ? h[code] : 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float s = acc[i][j][r] - hv;
                    if (cok && vq_better(s, code, best_s[j], best_i[j])) best_s[j] = s, best_i[j] = code;
                }
            }
        }
    }
    // the two lane halves hold different codes of the same frame
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const float os = __shfl_xor(best_s[j], 32);
        const int oi = __shfl_xor(best_i[j], 32);
        if (vq_better(os, oi, best_s[j], best_i[j])) best_s[j] = os, best_i[j] = oi;
        if (half == 0) sh_s[wave][j * 32 + col] = best_s[j], sh_i[wave][j * 32 + col] = best_i[j];
    }
    __syncthreads();
    if (threadIdx.x < NT * 32) {
        float bs = sh_s[0][threadIdx.x];
        int bi = sh_i[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (vq_better(sh_s[w][threadIdx.x], sh_i[w][threadIdx.x], bs, bi)) bs = sh_s[w][threadIdx.x], bi = sh_i[w][threadIdx.x];
        const long long n = nloc0 + threadIdx.x;
        if (n < count) {
            part_s[(long long)slice * n_pad + n_first + n] = bs;
            part_i[(long long)slice * n_pad + n_first + n] = bi;
        }
    }
}

// 32 frames x 64 channels per workgroup (grid.y runs over the channel chunks; every chunk settles the codes again from the few partials, chunk 0
// stores them).  The rows e_code are read along d (8 lanes per frame) into LDS and used along t (lane = frame), the direction in which x, r
// and z are contiguous.
__global__ __launch_bounds__(256) void vq_select_kernel(const float* in, VqFrames fr, VqRowBlock rows, const float* __restrict__ embed,
                                                        int D, int K, int slices, const float* __restrict__ part_s, const int* __restrict__ part_i,
                                                        long long n_first, long long n_pad, int* __restrict__ codes, float* r_out,
                                                        float* z, int first_layer) {
    __shared__ float tile[kVqSelFrames][kVqSelD + 1];
    __shared__ int sh_code[kVqSelFrames];
    const long long count = (long long)fr.rows * fr.T;
    const long long nloc0 = (long long)blockIdx.x * kVqSelFrames;
    if (threadIdx.x < kVqSelFrames) {
        const long long n = nloc0 + threadIdx.x;
        int code = -2;                                                  // -2: no such frame; -1: past the row's length
        if (n < count) {
            const int bl = (int)(n / fr.T), t = (int)(n - (long long)bl * fr.T);
            const int len = fr.uniform >= 0 ? fr.uniform : rows.e[bl];
            if (t < len) {
                float bs = -INFINITY;
                int bi = kNoCode;
                for (int s = 0; s < slices; ++s) {
                    const float ps = part_s[(long long)s * n_pad + n_first + n];
                    const int pi = part_i[(long long)s * n_pad + n_first + n];
                    if (vq_better(ps, pi, bs, bi)) bs = ps, bi = pi;
                }
                code = bi == kNoCode ? 0 : bi;
            } else {
                code = -1;
            }
            if (blockIdx.y == 0) codes[n_first + n] = code;
        }
        sh_code[threadIdx.x] = code;
    }
    __syncthreads();
    const int f = threadIdx.x & 31, dsub = threadIdx.x >> 5;
    const long long n = nloc0 + f;
    const int my_code = sh_code[f];
    long long xoff = 0, coff = 0;           // offsets of (b, 0, t) in `in` and in the contiguous (B, D, T) tensors r_out / z
    if (my_code != -2) {
        const int bl = (int)(n / fr.T), t = (int)(n - (long long)bl * fr.T);
        xoff = (long long)(fr.row0 + bl) * fr.bstride + t;
        coff = (long long)(fr.row0 + bl) * D * fr.T + t;
    }
    const int lf = threadIdx.x >> 3, ld = threadIdx.x & 7;
    const int lcode = sh_code[lf];
    {
        const int d0 = blockIdx.y * kVqSelD;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int dd = ld + 8 * i;
            tile[lf][dd] = (lcode >= 0 && d0 + dd < D) ? embed[(long long)lcode * D + d0 + dd] : 0.f;
        }
        __syncthreads();
        if (my_code == -2) return;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int dd = dsub + 8 * i, d = d0 + dd;
            if (d >= D) break;
            const long long co = coff + (long long)d * fr.T;
            if (my_code < 0) {
                if (z) z[co] = 0.f;
                continue;
            }
            const float e = tile[f][dd];
            if (r_out) r_out[co] = in[xoff + (long long)d * fr.dstride] - e;
            if (z) z[co] = first_layer ? e : z[co] + e;
        }
    }
}

struct VqLayerPtrs {
    const float* embed[kVqMaxLayers];
};

__global__ __launch_bounds__(256) void vq_gather_kernel(const int* __restrict__ codes, VqLayerPtrs layers, int n_q, int D, int K, int T, int row0,
                                                        int nrows, int uniform, VqRowBlock rows, long long n_total, float* __restrict__ z) {
    __shared__ float tile[kVqSelFrames][kVqSelD + 1];
    const long long count = (long long)nrows * T;
    const long long nloc0 = (long long)blockIdx.x * kVqSelFrames;
    const long long n_first = (long long)row0 * T;
    const int f = threadIdx.x & 31, dsub = threadIdx.x >> 5;
    const int lf = threadIdx.x >> 3, ld = threadIdx.x & 7;
    auto frame_ok = [&](long long n) {
        if (n >= count) return false;
        const int bl = (int)(n / T), t = (int)(n - (long long)bl * T);
        return t < (uniform >= 0 ? uniform : rows.e[bl]);
    };
    const long long n = nloc0 + f;
    const bool exists = n < count;
    long long coff = 0;
    if (exists) {
        const int bl = (int)(n / T), t = (int)(n - (long long)bl * T);
        coff = (long long)(row0 + bl) * D * T + t;
    }
    const bool lvalid = frame_ok(nloc0 + lf), fvalid = frame_ok(n);
    for (int d0 = 0; d0 < D; d0 += kVqSelD) {
        float acc[8];
        bool has = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int q = 0; q < n_q; ++q) {
            __syncthreads();
            int lcode = lvalid ? codes[(long long)q * n_total + n_first + nloc0 + lf] : -1;
            if (lcode >= K) lcode = -1;         // (the Python face raises IndexError before it comes to this)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int dd = ld + 8 * i;
                tile[lf][dd] = (lcode >= 0 && d0 + dd < D) ? layers.embed[q][(long long)lcode * D + d0 + dd] : 0.f;
            }
            __syncthreads();
            int c = fvalid ? codes[(long long)q * n_total + n_first + n] : -1;
            if (c >= K) c = -1;
            if (c >= 0) {                        // a negative code contributes nothing
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = has ? acc[i] + tile[f][dsub + 8 * i] : tile[f][dsub + 8 * i];
                has = true;
            }
        }
        if (exists) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int d = d0 + dsub + 8 * i;
                if (d < D) z[coff + (long long)d * T] = acc[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Code rings (engine_windows.hip fv_stream_push_codes / fv_codepool_step): stream_window_kernel and pool_gather_kernel
// (window_kernels.hip) for a session that keeps the CODES of its last `cap` frames, (rows, n_q, cap) int32 with frame f at slot f mod cap,
// and forms the generator's input window by looking them up: win[row][d][j] = ((e_0[c_0][d] + e_1[c_1][d]) + ...) of the window's column j,
// vq_gather_kernel's sum (layer order, the first valid layer assigned, a code < 0 or >= K contributes nothing, no valid code: exact zeros).
// A workgroup owns kVqSelFrames window columns x kVqSelD channels (blockIdx.y: the channel slice).  The codes of its columns come from the
// chunk at or after the old F and from the ring before it; slice 0 alone files the chunk's codes in the ring.  W <= cap, so the slots read and
// the slots written are distinct and no launch reads a code it wrote.  Every layer's row e_q[c] is read along d (a wave reads 64 consecutive
// floats of one row) into the padded tile and summed along the columns (lane = column), the direction in which the window is contiguous.
// ---------------------------------------------------------------------------------------------
struct CodeTile {
    float tile[kVqSelFrames][kVqSelD + 1];
    int code[kVqMaxLayers][kVqSelFrames];     // -1: nothing to add (no such column, or a code outside [0, K))
};

// The sum of the tile's columns over the layers; sh.code is filled and a barrier has been passed.  out(dd, v): channel d0 + dd of column
// threadIdx.x & 31 is v.
template <class Out>
__device__ __forceinline__ void code_tile_sum(CodeTile& sh, const VqLayerPtrs& layers, int n_q, int D, int d0, Out&& out) {
    const int f = threadIdx.x & 31, dsub = threadIdx.x >> 5;
    const int lane = threadIdx.x & 63, lrow = threadIdx.x >> 6;
    float acc[8];
    bool has = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int q = 0; q < n_q; ++q) {
        if (q) __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int fr = lrow + 4 * i;
            const int c = sh.code[q][fr];
            sh.tile[fr][lane] = (c >= 0 && d0 + lane < D) ? layers.embed[q][(long long)c * D + d0 + lane] : 0.f;
        }
        __syncthreads();
        if (sh.code[q][f] >= 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = has ? acc[i] + sh.tile[f][dsub + 8 * i] : sh.tile[f][dsub + 8 * i];
            has = true;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out(dsub + 8 * i, acc[i]);
}

__device__ __forceinline__ int code_or_none(int c, int K) { return c >= 0 && c < K ? c : -1; }

// chunk (n_q, B, n): the columns [c0, c0 + n); win (B, D, W): the columns [w, w + W), W = c0 + n - w (NULL: the chunk goes into the ring only)
__global__ __launch_bounds__(256) void stream_window_codes_kernel(const int* __restrict__ chunk, int* __restrict__ ring, float* __restrict__ win,
                                                                  VqLayerPtrs layers, int n_q, int D, int K, int B, long long cap,
                                                                  long long c0, long long n, long long w, long long W, int b0) {
    __shared__ CodeTile sh;
    const int b = b0 + blockIdx.z;
    const long long j0 = (long long)blockIdx.x * kVqSelFrames;
    for (int idx = threadIdx.x; idx < n_q * kVqSelFrames; idx += 256) {
        const int q = idx >> 5, fr = idx & 31;
        const long long j = j0 + fr, f = w + j;
        int c = -1;
        if (j < W) {
            int* slot = ring + ((long long)b * n_q + q) * cap + f % cap;
            if (f >= c0) {
                c = chunk[((long long)q * B + b) * n + (f - c0)];
                if (blockIdx.y == 0) *slot = c;
            } else {
                c = *slot;
            }
        }
        sh.code[q][fr] = code_or_none(c, K);
    }
    if (!win) return;
    __syncthreads();
    const int d0 = blockIdx.y * kVqSelD;
    const long long j = j0 + (threadIdx.x & 31);
    code_tile_sum(sh, layers, n_q, D, d0, [&](int dd, float v) {
        if (j < W && d0 + dd < D) win[((long long)b * D + d0 + dd) * W + j] = v;
    });
}

// chunk (n_q, items, in_frames), row e.item of every layer; win (rows, D, Wg): entry e's window at [col0, col0 + W), 0.0f elsewhere; an entry
// without a row (row < 0) only files its chunk in the ring (pool_gather_kernel's rule, counted in frames: hop = 1)
__global__ __launch_bounds__(256) void pool_gather_codes_kernel(const int* __restrict__ chunk, int* __restrict__ ring, float* __restrict__ win,
                                                                const PoolGatherBlock tab, VqLayerPtrs layers, int n_q, int D, int K, int items,
                                                                long long cap, long long in_frames, long long Wg) {
    __shared__ CodeTile sh;
    const PoolGatherEntry e = tab.e[blockIdx.z];
    const long long j0 = (long long)blockIdx.x * kVqSelFrames;
    if (e.row < 0) {
        if (blockIdx.y != 0) return;
        for (int idx = threadIdx.x; idx < n_q * kVqSelFrames; idx += 256) {
            const int q = idx >> 5;
            const long long j = j0 + (idx & 31);
            if (j < e.n) ring[((long long)e.slot * n_q + q) * cap + (e.F + j) % cap] = chunk[((long long)q * items + e.item) * in_frames + j];
        }
        return;
    }
    if (j0 >= Wg) return;      // (a launch spans its longest chunk where that is longer than the group's tensor)
    for (int idx = threadIdx.x; idx < n_q * kVqSelFrames; idx += 256) {
        const int q = idx >> 5, fr = idx & 31;
        const long long jj = j0 + fr - e.col0, f = e.w + jj;
        int c = -1;
        if (jj >= 0 && jj < e.W) {
            int* slot = ring + ((long long)e.slot * n_q + q) * cap + f % cap;
            if (f >= e.F) {
                c = chunk[((long long)q * items + e.item) * in_frames + (f - e.F)];
                if (blockIdx.y == 0) *slot = c;
            } else {
                c = *slot;
            }
        }
        sh.code[q][fr] = code_or_none(c, K);
    }
    __syncthreads();
    const int d0 = blockIdx.y * kVqSelD;
    const long long j = j0 + (threadIdx.x & 31);
    code_tile_sum(sh, layers, n_q, D, d0, [&](int dd, float v) {
        if (j < Wg && d0 + dd < D) win[((long long)e.row * D + d0 + dd) * Wg + j] = v;      // outside the entry's window: no code, v = 0.0f
    });
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace
}  // namespace fv

using namespace fv;

struct fv_vq {
    fv_vq_config cfg{};
    int nchunk = 0, ktiles = 0, units = 0;
    int slices_knob = 0;                            // fv_vq_set_slices: 0 = by launch size
    float* d_embed[kVqMaxLayers] = {};              // (K, D)
    float* d_packed[kVqMaxLayers] = {};             // A fragments: float4 [(tile * nchunk + chunk) * 64 + lane], component p = e[32 tile + (lane & 31)][8 chunk + 2 p + (lane >> 5)]
    float* d_h[kVqMaxLayers] = {};                  // (K)
    bool loaded[kVqMaxLayers] = {};
    ~fv_vq() {
        for (int q = 0; q < kVqMaxLayers; ++q) {
            if (d_embed[q]) (void)hipFree(d_embed[q]);
            if (d_packed[q]) (void)hipFree(d_packed[q]);
            if (d_h[q]) (void)hipFree(d_h[q]);
        }
    }
};

namespace fv {

fv_status vq_describe(const char* fn, const fv_vq* vq, int* dim, int* n_q) {
    if (!vq) {
        set_error("%s: null vq (the quantiser whose codebooks the code ring is decoded with)", fn);
        return FV_ERR_INVALID;
    }
    for (int q = 0; q < vq->cfg.num_quantizers; ++q)
        if (!vq->loaded[q]) {
            set_error("%s: the codebook of layer %d of vq has not been loaded (fv_vq_load_codebook)", fn, q);
            return FV_ERR_STATE;
        }
    *dim = vq->cfg.dim;
    *n_q = vq->cfg.num_quantizers;
    return FV_OK;
}

static VqLayerPtrs vq_layer_ptrs(const fv_vq* vq) {
    VqLayerPtrs lp{};
    for (int q = 0; q < vq->cfg.num_quantizers; ++q) lp.embed[q] = vq->d_embed[q];
    return lp;
}

fv_status launch_stream_window_codes(const fv_vq* vq, const int* chunk, int* ring, float* win, int B, long long cap, long long c0, long long n,
                                     long long w, hipStream_t s) {
    const long long W = c0 + n - w;
    if (W <= 0) return FV_OK;
    const int D = vq->cfg.dim;
    const unsigned slices = win ? (unsigned)((D + kVqSelD - 1) / kVqSelD) : 1u;
    constexpr long long kMaxZ = 65535;
    for (long long b0 = 0; b0 < B; b0 += kMaxZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxZ, (long long)B - b0);
        hipLaunchKernelGGL(stream_window_codes_kernel, dim3((unsigned)((W + kVqSelFrames - 1) / kVqSelFrames), slices, nz), dim3(256), 0, s, chunk,
                           ring, win, vq_layer_ptrs(vq), vq->cfg.num_quantizers, D, vq->cfg.codebook_size, B, cap, c0, n, w, W, (int)b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

fv_status launch_pool_gather_codes(const fv_vq* vq, const int* chunk, int* ring, float* win, const PoolGatherEntry* tab, int count, int items,
                                   long long cap, long long in_frames, long long Wg, hipStream_t s) {
    const int D = vq->cfg.dim;
    const VqLayerPtrs lp = vq_layer_ptrs(vq);
    return for_each_launch_table<PoolGatherBlock>(count, tab, [&](const PoolGatherBlock& blk, int, int nz) {
        long long X = 0;   // columns this launch spans: the group's tensor for a row, the chunk for a ring-only entry
        bool rows = false;
        for (int i = 0; i < nz; ++i) {
            X = std::max(X, blk.e[i].row >= 0 ? Wg : (long long)blk.e[i].n);
            rows |= blk.e[i].row >= 0;
        }
        if (X > 0)
            hipLaunchKernelGGL(pool_gather_codes_kernel, dim3((unsigned)((X + kVqSelFrames - 1) / kVqSelFrames), rows ? (unsigned)((D + kVqSelD - 1) / kVqSelD) : 1u, nz),
                               dim3(256), 0, s, chunk, ring, win, blk, lp, vq->cfg.num_quantizers, D, vq->cfg.codebook_size, items, cap, in_frames, Wg);
        return FV_OK;
    });
}

}  // namespace fv

namespace {

struct VqPlan {
    long long N = 0, n_pad = 0;
    int nt = 1, slices = 1, units_per_slice = 1;
    size_t r_bytes = 0, part_bytes = 0, total = 0;
};

// The launch shape of an encode: a function of the handle and (batch, T) alone, so fv_vq_workspace_bytes and fv_vq_encode agree
VqPlan vq_plan(const fv_vq* p, int batch, long long T) {
    VqPlan pl;
    pl.N = (long long)batch * T;
    pl.n_pad = (pl.N + 63) / 64 * 64;
    const int cus = std::max(num_cus(), 1);
    // the codebook streams from L2 once per workgroup: two frame tiles where that still leaves two workgroups per compute unit
    pl.nt = (pl.N + 63) / 64 * p->units >= 2LL * cus ? 2 : 1;
    const long long ftiles = std::max<long long>((pl.N + 32 * pl.nt - 1) / (32 * pl.nt), 1);
    long long want = p->slices_knob > 0 ? p->slices_knob : (2LL * cus + ftiles - 1) / ftiles;
    want = std::min<long long>(std::max<long long>(want, 1), p->units);
    pl.units_per_slice = (int)((p->units + want - 1) / want);
    pl.slices = (p->units + pl.units_per_slice - 1) / pl.units_per_slice;
    pl.r_bytes = p->cfg.num_quantizers > 1 ? up256((size_t)pl.N * (size_t)p->cfg.dim * 4) : 0;
    pl.part_bytes = up256((size_t)pl.slices * (size_t)pl.n_pad * 4);
    pl.total = pl.r_bytes + 2 * pl.part_bytes;
    return pl;
}

fv_status vq_check_shape(const char* fn, const fv_vq* p, int32_t batch, int64_t T) {
    if (!p) {
        set_error("%s: null quantiser", fn);
        return FV_ERR_INVALID;
    }
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kVqMaxFrames || (long long)batch * T > kVqMaxFrames) {
        set_error("%s: T = %lld must be >= 0 and batch * T at most 2^30 frames", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

fv_status vq_check_frames(const char* fn, const int32_t* host_frames, int batch, int T) {
    for (int b = 0; host_frames && b < batch; ++b)
        if (host_frames[b] < 0 || host_frames[b] > T) {
            set_error("%s: host_frames[%d] = %d lies outside [0, T = %d]", fn, b, host_frames[b], T);
            return FV_ERR_INVALID;
        }
    return FV_OK;
}

// launch(rows, row0, nrows, uniform) over the batch: kVqRows rows per call with their lengths, or — host_frames == NULL, every row holds T
// frames — one call over all rows with uniform = T and a zeroed table that is never read
template <class Launch>
fv_status vq_for_rows(const int32_t* host_frames, int batch, int T, Launch&& launch) {
    if (host_frames)
        return for_each_launch_table<VqRowBlock>(batch, host_frames,
                                                 [&](const VqRowBlock& rows, int row0, int nrows) { return launch(rows, row0, nrows, -1); });
    if (const fv_status st = launch(VqRowBlock{}, 0, batch, T)) return st;
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

fv_status vq_check_loaded(const char* fn, const fv_vq* p) {
    for (int q = 0; q < p->cfg.num_quantizers; ++q)
        if (!p->loaded[q]) {
            set_error("%s: the codebook of layer %d has not been loaded (fv_vq_load_codebook)", fn, q);
            return FV_ERR_STATE;
        }
    return FV_OK;
}

}  // namespace

extern "C" {

FV_API fv_status fv_vq_create(const fv_vq_config* cfg, fv_vq** out) {
    const char* fn = "fv_vq_create";
    if (!out || !cfg) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (cfg->dim < 1 || cfg->dim > kVqMaxDim) {
        set_error("%s: dim = %d must lie in [1, %d]", fn, cfg->dim, kVqMaxDim);
        return FV_ERR_INVALID;
    }
    if (cfg->codebook_size < 1 || cfg->codebook_size > kVqMaxCodes) {
        set_error("%s: codebook_size = %d must lie in [1, %d]", fn, cfg->codebook_size, kVqMaxCodes);
        return FV_ERR_INVALID;
    }
    if (cfg->num_quantizers < 1 || cfg->num_quantizers > kVqMaxLayers) {
        set_error("%s: num_quantizers = %d must lie in [1, %d]", fn, cfg->num_quantizers, kVqMaxLayers);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_vq> p(new fv_vq());
    p->cfg = *cfg;
    p->nchunk = (cfg->dim + 8 * kVqGroup - 1) / (8 * kVqGroup) * kVqGroup;      // chunks of 8 channels, in whole groups
    p->ktiles = (cfg->codebook_size + 31) / 32;
    p->units = (p->ktiles + kVqUnit - 1) / kVqUnit;
    *out = p.release();
    return FV_OK;
}

FV_API void fv_vq_destroy(fv_vq* p) { delete p; }

FV_API fv_status fv_vq_set_slices(fv_vq* p, int32_t slices) {
    if (!p || slices < 0) {
        set_error("fv_vq_set_slices: %s", !p ? "null quantiser" : "slices must be >= 0 (0 = by launch size)");
        return FV_ERR_INVALID;
    }
    p->slices_knob = slices;
    return FV_OK;
}

FV_API fv_status fv_vq_load_codebook(fv_vq* p, int32_t layer, const float* host_embed) {
    const char* fn = "fv_vq_load_codebook";
    if (!p || !host_embed) {
        set_error("%s: null %s", fn, !p ? "quantiser" : "host_embed");
        return FV_ERR_INVALID;
    }
    if (layer < 0 || layer >= p->cfg.num_quantizers) {
        set_error("%s: layer = %d lies outside [0, num_quantizers = %d)", fn, layer, p->cfg.num_quantizers);
        return FV_ERR_INVALID;
    }
    const int D = p->cfg.dim, K = p->cfg.codebook_size;
    std::vector<float> h(K);
    for (int j = 0; j < K; ++j) {
        double acc = 0.0;
        for (int d = 0; d < D; ++d) acc += (double)host_embed[(size_t)j * D + d] * (double)host_embed[(size_t)j * D + d];
        h[j] = (float)(0.5 * acc);
    }
    const size_t packed_floats = (size_t)p->ktiles * p->nchunk * 256;
    std::vector<float> packed(packed_floats, 0.f);
    for (int ct = 0; ct < p->ktiles; ++ct)
        for (int c = 0; c < p->nchunk; ++c)
            for (int lane = 0; lane < 64; ++lane)
                for (int pp = 0; pp < 4; ++pp) {
                    const int code = 32 * ct + (lane & 31), d = 8 * c + 2 * pp + (lane >> 5);
                    if (code < K && d < D) packed[(((size_t)ct * p->nchunk + c) * 64 + lane) * 4 + pp] = host_embed[(size_t)code * D + d];
                }
    if (!p->d_embed[layer]) FV_HIP_CHECK(hipMalloc(&p->d_embed[layer], (size_t)K * D * 4));
    if (!p->d_packed[layer]) FV_HIP_CHECK(hipMalloc(&p->d_packed[layer], packed_floats * 4));
    if (!p->d_h[layer]) FV_HIP_CHECK(hipMalloc(&p->d_h[layer], (size_t)K * 4));
    FV_HIP_CHECK(hipMemcpy(p->d_embed[layer], host_embed, (size_t)K * D * 4, hipMemcpyHostToDevice));
    FV_HIP_CHECK(hipMemcpy(p->d_packed[layer], packed.data(), packed_floats * 4, hipMemcpyHostToDevice));
    FV_HIP_CHECK(hipMemcpy(p->d_h[layer], h.data(), (size_t)K * 4, hipMemcpyHostToDevice));
    p->loaded[layer] = true;
    return FV_OK;
}

FV_API size_t fv_vq_workspace_bytes(const fv_vq* p, int32_t batch, int64_t T) {
    if (vq_check_shape("fv_vq_workspace_bytes", p, batch, T)) return 0;
    if (batch == 0 || T == 0) return 0;
    return vq_plan(p, batch, T).total;
}

FV_API fv_status fv_vq_encode(fv_vq* p, const float* d_x, int64_t x_row_stride, const int32_t* host_frames, int32_t* d_codes, float* d_z,
                              int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fv_vq_encode";
    if (const fv_status st = vq_check_shape(fn, p, batch, T)) return st;
    if (const fv_status st = vq_check_loaded(fn, p)) return st;
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_x || !d_codes) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : "d_codes");
        return FV_ERR_INVALID;
    }
    if (x_row_stride < T) {
        set_error("%s: x_row_stride = %lld (the stride between channels) is shorter than a row of T = %lld frames", fn, (long long)x_row_stride,
                  (long long)T);
        return FV_ERR_INVALID;
    }
    const VqPlan pl = vq_plan(p, batch, T);
    if (workspace_bytes < pl.total || (pl.total && !d_workspace)) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_vq_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, pl.total, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = vq_check_frames(fn, host_frames, batch, (int)T)) return st;   // everything is validated before anything is enqueued

    const int D = p->cfg.dim, K = p->cfg.codebook_size, nq = p->cfg.num_quantizers;
    char* ws = (char*)d_workspace;
    float* r = pl.r_bytes ? (float*)ws : nullptr;
    float* part_s = (float*)(ws + pl.r_bytes);
    int* part_i = (int*)(ws + pl.r_bytes + pl.part_bytes);
    hipStream_t s = (hipStream_t)stream;
    for (int q = 0; q < nq; ++q) {
        const bool last = q == nq - 1;
        const float* in = q == 0 ? d_x : r;
        const fv_status st = vq_for_rows(host_frames, batch, (int)T, [&](const VqRowBlock& rb, int row0, int nrows, int uniform) -> fv_status {
            VqFrames fr;
            fr.T = (int)T;
            fr.row0 = row0;
            fr.rows = nrows;
            fr.uniform = uniform;
            fr.bstride = q == 0 ? (long long)D * x_row_stride : (long long)D * T;
            fr.dstride = q == 0 ? (long long)x_row_stride : (long long)T;
            const long long count = (long long)fr.rows * T, n_first = (long long)fr.row0 * T;
            const dim3 grid((unsigned)((count + 32 * pl.nt - 1) / (32 * pl.nt)), (unsigned)pl.slices);
            const auto kernel = pl.nt == 2 ? vq_search_kernel<2> : vq_search_kernel<1>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, in, fr, rb, (const float4*)p->d_packed[q], p->d_h[q], D, K, p->nchunk, p->ktiles,
                               pl.units_per_slice, part_s, part_i, n_first, pl.n_pad);
            FV_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(vq_select_kernel, dim3((unsigned)((count + kVqSelFrames - 1) / kVqSelFrames), (unsigned)((D + kVqSelD - 1) / kVqSelD)), dim3(256), 0, s, in, fr, rb,
                               p->d_embed[q], D, K, pl.slices, part_s, part_i, n_first, pl.n_pad, d_codes + (size_t)q * pl.N, last ? nullptr : r, d_z,
                               q == 0 ? 1 : 0);
            return FV_OK;
        });
        if (st) return st;
    }
    set_last_kernel(pl.nt == 2 ? "vq_search_kernel<2>" : "vq_search_kernel<1>");
    return FV_OK;
}

FV_API fv_status fv_vq_decode(fv_vq* p, const int32_t* d_codes, const int32_t* host_frames, float* d_z, int32_t batch, int64_t T, void* stream) {
    const char* fn = "fv_vq_decode";
    if (const fv_status st = vq_check_shape(fn, p, batch, T)) return st;
    if (const fv_status st = vq_check_loaded(fn, p)) return st;
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_codes || !d_z) {
        set_error("%s: null %s", fn, !d_codes ? "d_codes" : "d_z");
        return FV_ERR_INVALID;
    }
    if (const fv_status st = vq_check_frames(fn, host_frames, batch, (int)T)) return st;
    VqLayerPtrs lp{};
    for (int q = 0; q < p->cfg.num_quantizers; ++q) lp.embed[q] = p->d_embed[q];
    const fv_status st = vq_for_rows(host_frames, batch, (int)T, [&](const VqRowBlock& rb, int row0, int nrows, int uniform) {
        const long long count = (long long)nrows * T;
        hipLaunchKernelGGL(vq_gather_kernel, dim3((unsigned)((count + kVqSelFrames - 1) / kVqSelFrames)), dim3(256), 0, (hipStream_t)stream, d_codes,
                           lp, p->cfg.num_quantizers, p->cfg.dim, p->cfg.codebook_size, (int)T, row0, nrows, uniform, rb, (long long)batch * T,
                           d_z);
        return FV_OK;
    });
    if (st == FV_OK) set_last_kernel("vq_gather_kernel");
    return st;
}

}  // extern "C"
