// The device half of engine_windows.hip: the copy kernels between the caller's tensors, the rings and the window workspace of the time
// tiles, streams, ragged batches and session pools; and the carry copies of the sample streams (sample_stream.h) and of the sample pools
// (sample_pool.h).  HBM-bound: each lane moves
// one fp32, coalesced along T.
#include <algorithm>

#include "fv_internal.h"

namespace fv {

// ---------------------------------------------------------------------------------------------
// Long clips as a batch of time tiles (engine_windows.hip run_model): tile i of a clip covers frames [a_i, a_i + L), a_i = min(i * stride, T - L);
// `hop` scales frames to samples (1 for the mel input, the generator's hop for the pitch template and the waveform).
//   gather : tiles[(b * n + i)][c][l] = x[b][c][a_i * hop + l]
//   scatter: y[b][c][lo_i * hop ...) = tiles[(b * n + i)][c][(lo_i - a_i) * hop ...), the frames [lo_i, hi_i) tile i contributes
// ---------------------------------------------------------------------------------------------
static constexpr long long kMaxGridZ = 65535;
__global__ __launch_bounds__(256) void gather_tiles_kernel(const float* __restrict__ x, float* __restrict__ tiles, int C, long long T,
                                                           int n, long long L, int stride, int hop, long long Tf, int bi0) {
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int c = blockIdx.y, bi = bi0 + blockIdx.z, b = bi / n, i = bi % n;
    long long a = (long long)i * stride;
    if (a > Tf - L / hop) a = Tf - L / hop;
    tiles[((long long)bi * C + c) * L + l] = x[((long long)b * C + c) * T + a * hop + l];
}
fv_status launch_gather_tiles(const float* x, float* tiles, int B, int C, int T, int n, int L, int stride, int hop, hipStream_t s) {
    const long long Ls = (long long)L * hop;
    // gridDim.z is limited to 65 535: (clip, tile) items in chunks of that (a long clip with a short tile and a moderate batch)
    for (long long bi0 = 0; bi0 < (long long)B * n; bi0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, (long long)B * n - bi0);
        hipLaunchKernelGGL(gather_tiles_kernel, dim3((unsigned)((Ls + 255) / 256), C, nz), dim3(256), 0, s, x, tiles, C, (long long)T * hop, n,
                           Ls, stride, hop, (long long)T, (int)bi0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}
__global__ __launch_bounds__(256) void scatter_tiles_kernel(const float* __restrict__ tiles, float* __restrict__ y, int C, long long T,
                                                            int n, long long L, int stride, int halo, int hop, long long Tf, int bi0) {
    const int c = blockIdx.y, bi = bi0 + blockIdx.z, b = bi / n, i = bi % n;
    const long long Lf = L / hop;
    long long a = (long long)i * stride;
    if (a > Tf - Lf) a = Tf - Lf;
    const long long lo = i == 0 ? 0 : (long long)(i - 1) * stride + Lf - halo;
    const long long hi = i + 1 == n ? Tf : (long long)i * stride + Lf - halo;
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;   // sample within the tile's contribution
    if (j >= (hi - lo) * hop) return;
    y[((long long)b * C + c) * T + lo * hop + j] = tiles[((long long)bi * C + c) * L + (lo - a) * hop + j];
}
fv_status launch_scatter_tiles(const float* tiles, float* y, int B, int C, int T, int n, int L, int stride, int halo, int hop, hipStream_t s) {
    const long long Ls = (long long)L * hop;
    for (long long bi0 = 0; bi0 < (long long)B * n; bi0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, (long long)B * n - bi0);
        hipLaunchKernelGGL(scatter_tiles_kernel, dim3((unsigned)((Ls + 255) / 256), C, nz), dim3(256), 0, s, tiles, y, C, (long long)T * hop, n,
                           Ls, stride, halo, hop, (long long)T, (int)bi0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------
// Streaming synthesis (engine_windows.hip fv_stream_push).  A session keeps its last `cap` columns in a ring: column f at slot f mod cap.  Columns are
// frames x hop (hop = 1 for the mel, the generator's hop for the pitch template), counted from the start of the utterance.  The chunk holds
// the columns [c0, c0 + n), the window the columns [w, c0 + n), w <= c0.
//   stream_window: ring[b][c][f mod cap] = chunk[b][c][f - c0] for the chunk's columns, and win[b][c][f - w] = column f for the window's, from
//                  the chunk for f >= c0 and from the ring before it (win = NULL: the chunk goes into the ring only).  A window spans at most
//                  `cap` columns, so the slots it reads and the slots the chunk overwrites are distinct: one launch does both.
//   stream_crop  : out[b][c][j] = y[b][c][a + j], j < len — the emitted samples of the window's output.
// Window starts, chunk sizes and ring slots follow the caller's pushes, so rows are not 16-byte aligned in general: each lane moves one fp32,
// coalesced along the row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stream_window_kernel(const float* __restrict__ chunk, float* __restrict__ ring, float* __restrict__ win,
                                                            int C, long long cap, long long c0, long long n, long long w, long long W, int b0) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= W) return;
    const long long row = (long long)(b0 + blockIdx.z) * C + blockIdx.y;
    const long long f = w + j;
    float* slot = ring + row * cap + f % cap;
    float v;
    if (f >= c0) {
        v = chunk[row * n + (f - c0)];
        *slot = v;
    } else {
        v = *slot;
    }
    if (win) win[row * W + j] = v;
}
fv_status launch_stream_window(const float* chunk, float* ring, float* win, int B, int C, long long cap, long long c0, long long n, long long w,
                               hipStream_t s) {
    const long long W = c0 + n - w;
    if (W <= 0) return FV_OK;
    for (long long b0 = 0; b0 < B; b0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, (long long)B - b0);
        hipLaunchKernelGGL(stream_window_kernel, dim3((unsigned)((W + 255) / 256), C, nz), dim3(256), 0, s, chunk, ring, win, C, cap, c0, n, w, W,
                           (int)b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}
__global__ __launch_bounds__(256) void stream_crop_kernel(const float* __restrict__ y, float* __restrict__ out, int C, long long Ly, long long a,
                                                          long long len, int b0) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    const long long row = (long long)(b0 + blockIdx.z) * C + blockIdx.y;
    out[row * len + j] = y[row * Ly + a + j];
}
fv_status launch_stream_crop(const float* y, float* out, int B, int C, long long Ly, long long a, long long len, hipStream_t s) {
    if (len <= 0) return FV_OK;
    for (long long b0 = 0; b0 < B; b0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, (long long)B - b0);
        hipLaunchKernelGGL(stream_crop_kernel, dim3((unsigned)((len + 255) / 256), C, nz), dim3(256), 0, s, y, out, C, Ly, a, len, (int)b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------
// Ragged batches (engine_windows.hip fv_ragged_forward).  `tab` is the plan's window table on the device (fv_ragged_window: clip b, start a, frames n,
// keep [lo, hi)), `lens` the clips' lengths in frames; item i of a launch is window i0 + blockIdx.z of the table, stored as item
// (i0 - first + blockIdx.z) of its group's buffer.  Columns are frames x hop (hop = 1 for the mel, the generator's hop for the pitch template
// and the waveform); T = columns of a clip's row in the caller's tensor, L = columns of a window.
//   gather   : win[i][c][l] = a hop + l < len_b hop ? x[b][c][a hop + l] : 0.  The padding is never LOADED: the address is clamped to the
//              window's first column (a < len_b always) and the value selected, so a NaN the caller left there cannot enter through 0 * x.
//   scatter  : y[b][c][lo hop + j] = out[i][c][(lo - a) hop + j], j < (hi - lo) hop
//   zero_tail: y[b][c][len_b hop ...) = 0 up to the row's end
// Rows start at arbitrary sample offsets: each lane moves one fp32, coalesced along the row (as the stream kernels).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ragged_gather_kernel(const float* __restrict__ x, float* __restrict__ win,
                                                            const fv_ragged_window* __restrict__ tab, const int* __restrict__ lens, int C,
                                                            long long T, long long L, int hop, int first, int i0) {
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int c = blockIdx.y, i = i0 + blockIdx.z;
    const fv_ragged_window w = tab[i];
    const long long a = (long long)w.start * hop, len = (long long)lens[w.clip] * hop;
    const bool valid = a + l < len;
    const float v = x[((long long)w.clip * C + c) * T + (valid ? a + l : a)];
    win[((long long)(i - first) * C + c) * L + l] = valid ? v : 0.0f;
}
fv_status launch_ragged_gather(const float* x, float* win, const fv_ragged_window* tab, const int* lens, int first, int count, int C,
                               long long T, long long L, int hop, hipStream_t s) {
    if (count <= 0 || L <= 0) return FV_OK;
    for (long long i0 = 0; i0 < count; i0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, count - i0);
        hipLaunchKernelGGL(ragged_gather_kernel, dim3((unsigned)((L + 255) / 256), C, nz), dim3(256), 0, s, x, win, tab, lens, C, T, L, hop,
                           first, (int)(first + i0));
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}
__global__ __launch_bounds__(256) void ragged_scatter_kernel(const float* __restrict__ win, float* __restrict__ y,
                                                             const fv_ragged_window* __restrict__ tab, int C, long long T, long long L,
                                                             int hop, int first, int i0) {
    const int c = blockIdx.y, i = i0 + blockIdx.z;
    const fv_ragged_window w = tab[i];
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long long)(w.keep_hi - w.keep_lo) * hop) return;
    y[((long long)w.clip * C + c) * T + (long long)w.keep_lo * hop + j] =
        win[((long long)(i - first) * C + c) * L + (long long)(w.keep_lo - w.start) * hop + j];
}
fv_status launch_ragged_scatter(const float* win, float* y, const fv_ragged_window* tab, int first, int count, int C, long long T,
                                long long L, int hop, hipStream_t s) {
    if (count <= 0 || L <= 0) return FV_OK;
    for (long long i0 = 0; i0 < count; i0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, count - i0);
        hipLaunchKernelGGL(ragged_scatter_kernel, dim3((unsigned)((L + 255) / 256), C, nz), dim3(256), 0, s, win, y, tab, C, T, L, hop, first,
                           (int)(first + i0));
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}
__global__ __launch_bounds__(256) void ragged_zero_tail_kernel(float* __restrict__ y, const int* __restrict__ lens, int C, long long T, int hop,
                                                               int b0) {
    const int b = b0 + blockIdx.z;
    const long long j = (long long)lens[b] * hop + (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    y[((long long)b * C + blockIdx.y) * T + j] = 0.0f;
}
// span: columns of the longest tail, (t_max - min length) * hop
fv_status launch_ragged_zero_tail(float* y, const int* lens, int B, int C, long long T, long long span, int hop, hipStream_t s) {
    if (span <= 0) return FV_OK;
    for (long long b0 = 0; b0 < B; b0 += kMaxGridZ) {
        const unsigned nz = (unsigned)std::min<long long>(kMaxGridZ, (long long)B - b0);
        hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3((unsigned)((span + 255) / 256), C, nz), dim3(256), 0, s, y, lens, C, T, hop, (int)b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------
// Session pool (engine_windows.hip fv_pool_step).  Every session keeps a ring row as a stream does (column f at slot f mod cap); the rows of
// one group are windows of different lengths placed inside one (rows, C, Wg) tensor.  The entry tables arrive by value (PoolGatherBlock /
// PoolCropBlock, kPoolBlock entries per launch: blockIdx.z picks the entry); entries count in frames and `hop` scales them to columns.
//   pool_gather: entry with a row: win[row][c][j] = column w + (j - col0) of the session for j in [col0, col0 + W), 0.0f elsewhere; as in
//                stream_window a column comes from the chunk when it lies at or after the old F — and goes into the ring on the way — and from
//                the ring before it, so no value is written to the ring and read back in one launch (W <= cap: the slots read and the slots
//                written are distinct).  Entry without a row (row < 0): chunk -> ring only.  Chunk columns >= n are never addressed: a
//                window column f reads chunk[f - F] with f < F + n, and a ring-only entry clamps the address and selects, as ragged_gather.
//   pool_crop  : out[item][c][j] = j < len ? y[row][c][src + j] : 0.0f over the whole output row (row < 0: a row of zeros).
// Rows start at arbitrary columns: each lane moves one fp32, coalesced along the row (as the stream and ragged kernels).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pool_gather_kernel(const float* __restrict__ chunk, float* __restrict__ ring, float* __restrict__ win,
                                                          const PoolGatherBlock tab, int C, long long cap, long long in_cols, long long Wg,
                                                          int hop) {
    const PoolGatherEntry e = tab.e[blockIdx.z];
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const long long F = e.F * hop, n = (long long)e.n * hop;
    const float* src = chunk + ((long long)e.item * C + c) * in_cols;
    float* rg = ring + ((long long)e.slot * C + c) * cap;
    if (e.row < 0) {
        if (n <= 0 || j >= in_cols) return;
        const bool valid = j < n;
        const float v = src[valid ? j : 0];
        if (valid) rg[(F + j) % cap] = v;
        return;
    }
    if (j >= Wg) return;
    const long long jj = j - (long long)e.col0 * hop, f = e.w * hop + jj;
    float v = 0.0f;
    if (jj >= 0 && jj < (long long)e.W * hop) {
        float* slot = rg + f % cap;
        if (f >= F) {
            v = src[f - F];
            *slot = v;
        } else {
            v = *slot;
        }
    }
    win[((long long)e.row * C + c) * Wg + j] = v;
}
fv_status launch_pool_gather(const float* chunk, float* ring, float* win, const PoolGatherEntry* tab, int count, int C, long long cap,
                             long long in_frames, long long Wg, int hop, hipStream_t s) {
    return for_each_launch_table<PoolGatherBlock>(count, tab, [&](const PoolGatherBlock& blk, int, int nz) {
        long long X = 0;   // columns this launch spans: the group's tensor for a row, the chunk for a ring-only entry
        for (int i = 0; i < nz; ++i) X = std::max(X, blk.e[i].row >= 0 ? Wg * hop : (long long)blk.e[i].n * hop);
        if (X > 0)
            hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)((X + 255) / 256), C, nz), dim3(256), 0, s, chunk, ring, win, blk, C, cap * hop,
                               in_frames * hop, Wg * hop, hop);
        return FV_OK;
    });
}
__global__ __launch_bounds__(256) void pool_crop_kernel(const float* __restrict__ y, float* __restrict__ out, const PoolCropBlock tab, int C,
                                                        long long Ly, long long out_cols, int hop, long long out_stride) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= out_cols) return;
    const PoolCropEntry e = tab.e[blockIdx.z];
    const int c = blockIdx.y;
    float v = 0.0f;
    if (e.row >= 0 && j < e.len * hop) v = y[((long long)e.row * C + c) * Ly + e.src * hop + j];
    out[((long long)e.item * C + c) * out_stride + j] = v;
}
fv_status launch_pool_crop(const float* y, float* out, const PoolCropEntry* tab, int count, int C, long long Ly, long long out_frames, int hop,
                           hipStream_t s, long long out_stride) {
    if (out_frames <= 0) return FV_OK;
    if (out_stride <= 0) out_stride = out_frames * hop;
    return for_each_launch_table<PoolCropBlock>(count, tab, [&](const PoolCropBlock& blk, int, int nz) {
        hipLaunchKernelGGL(pool_crop_kernel, dim3((unsigned)((out_frames * hop + 255) / 256), C, nz), dim3(256), 0, s, y, out, blk, C, Ly * hop,
                           out_frames * hop, hop, out_stride);
        return FV_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// Sample streams (sample_stream.h: fv_resample_stream_*, fv_logmel_stream_*).  A stream carries the last samples of every row in two ping-pong
// buffers of row stride `stride`; `N` samples have arrived before this call and the chunk holds the samples [N, ...).
//   sample_carry: next[b][i] = sample idx = next_origin + i of row b, i < count: chunk[b][idx - N] for idx >= N, prev[b][idx - prev_origin] for
//                 0 <= idx < N, 0.0f for idx < 0 (samples before the utterance's start do not exist and are never loaded).  prev is only read
//                 and next only written: no launch does both to one buffer.
// Indices and row offsets are 64-bit; each lane moves one fp32, coalesced along the row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_carry_kernel(const float* __restrict__ prev, float* __restrict__ next,
                                                           const float* __restrict__ chunk, long long stride, long long chunk_stride,
                                                           long long N, long long next_origin, long long prev_origin, long long count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long long b = blockIdx.y, idx = next_origin + i;
    float v = 0.0f;
    if (idx >= N) v = chunk[b * chunk_stride + (idx - N)];
    else if (idx >= 0) v = prev[b * stride + (idx - prev_origin)];
    next[b * stride + i] = v;
}
fv_status launch_sample_carry(const float* prev, float* next, const float* chunk, long long stride, long long chunk_stride, int B, long long N,
                              long long next_origin, long long prev_origin, long long count, hipStream_t s) {
    if (B <= 0 || count <= 0) return FV_OK;
    hipLaunchKernelGGL(sample_carry_kernel, dim3((unsigned)((count + 255) / 256), B), dim3(256), 0, s, prev, next, chunk, stride, chunk_stride, N,
                       next_origin, prev_origin, count);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------
// Sample pools (sample_pool.h: fv_wavpool_*).  Every slot has its own counters and its own ping-pong bit; the entries of one step arrive by
// value (SamplePoolBlock: blockIdx.y picks the entry).
//   sample_pool_carry: sample_carry's rule per entry — buf[bit ^ 1][slot][i] = sample idx = avail - H + i of the slot: chunk[item][idx - N] for
//                      idx >= N (= chunk_origin), buf[bit][slot][idx - (N - H)] for 0 <= idx < N, 0.0f for idx < 0.  An entry reads buffer `bit`
//                      and writes buffer `bit ^ 1` of its own slot only: no launch reads and writes the same buffer of a slot, and the slots
//                      that take no part in the step keep their carry where their own bit says it is.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_pool_carry_kernel(float* buf0, float* buf1, const float* __restrict__ chunk,
                                                                const SamplePoolBlock tab, long long H, long long chunk_stride) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const SamplePoolEntry e = tab.e[blockIdx.y];
    const float* prev = (e.bit ? buf1 : buf0) + (long long)e.slot * H;
    float* next = (e.bit ? buf0 : buf1) + (long long)e.slot * H;
    const long long idx = e.avail - H + i;
    float v = 0.0f;
    if (idx >= e.chunk_origin) v = chunk[(long long)e.item * chunk_stride + (idx - e.chunk_origin)];
    else if (idx >= 0) v = prev[idx - e.carry_origin];
    next[i] = v;
}
fv_status launch_sample_pool_carry(float* buf0, float* buf1, long long H, const float* chunk, long long chunk_stride,
                                   const SamplePoolEntry* tab, int count, hipStream_t s) {
    if (count <= 0 || H <= 0) return FV_OK;
    for (int k = 0; k < count; ++k) {
        const SamplePoolEntry& e = tab[k];
        const long long c = e.avail - e.chunk_origin;
        if (c < 0 || e.chunk_origin - e.carry_origin != H || (c > 0 && (!chunk || c > chunk_stride))) {
            set_error("sample_pool_carry: internal: entry %d (session %d) does not fit its pieces", k, e.slot);
            return FV_ERR_INVALID;
        }
    }
    return for_each_launch_table<SamplePoolBlock>(count, tab, [&](const SamplePoolBlock& blk, int, int nz) {
        hipLaunchKernelGGL(sample_pool_carry_kernel, dim3((unsigned)((H + 255) / 256), nz), dim3(256), 0, s, buf0, buf1, chunk, blk, H,
                           chunk_stride);
        return FV_OK;
    });
}
}  // namespace fv
