// The frame-domain copies around the STFT / ISTFT convs, each stage with ONE body that its whole-row and its carry + chunk (stream, ragged)
// entry points instantiate — a stream's bits equal the whole row's because both run the same statements:
//   polyphase_tile        wave -> the polyphase signal Yp[row][r][tp] = sample((f0 + tp) hop + r - pad): a 32 x 33 LDS transpose around a sample rule
//     polyphase_reflect_kernel   one row, reflect edges (the log-mel front-end of fv_forward)
//     logmel_window_kernel       carry + chunk, reflect edges, per-row ends (fv_logmel_ragged_forward, fv_logmel_stream_*)
//     logmel_pool_window_kernel  carry + chunk per table entry: sessions that advance independently (fv_wavpool_step)
//     pv_frame_kernel            one row, zero edges (the whole-row pitch shift)
//     pv_frame_window_kernel     carry + chunk, zero edges (fv_pv_stream_*)
//     pv_frame_pool_window_kernel  carry + chunk per table entry, zero edges (fv_pvpool_step)
//   ola_tile              frames -> samples: overlap-add in ascending g, envelope, crop, around a frame fetch over the global frame index
//     istft_ola_kernel           one piece of T frames (the vocos head, the whole-row pitch shift)
//     istft_ola_window_kernel    the carried frames plus the new ones, an output window [Y, Y2) (fv_pv_stream_*)
//     istft_ola_pool_window_kernel  the same per table entry: the slot's carried frames, its own S, dS, Tend and [Y, Y2) (fv_pvpool_step)
//   pv_frame_carry        the last G synthesised frames, into the other buffer of the pair; per table entry in pv_frame_pool_carry_kernel
//   zero_columns          columns >= T_b of a (B, C, T) result set to 0.0f
// HBM-bound copies: each lane moves one fp32.
#include <algorithm>

#include "fv_internal.h"

namespace fv {

// ---------------------------------------------------------------------------------------------
// Where a sample comes from, and what stands at the edges.
// A slot that takes no sample (padding, an empty row) loads nothing; a slot that takes one clamps its address into the row or the piece it
// reads, so whatever the caller left outside (NaN included) never reaches a register.  No source is written by a kernel that reads it, so a
// push never writes the carry and reads it back in one launch (the session pool's rule).
// ---------------------------------------------------------------------------------------------
// reflect edges: idx < 0 reflects to -idx; with the end known (end >= 0) idx >= end reflects to 2 (end - 1) - idx
__device__ __forceinline__ long long reflect_index(long long idx, long long end) {
    if (idx < 0) idx = -idx;
    if (end >= 0 && idx >= end) idx = 2 * (end - 1) - idx;
    return idx;
}

// one row of L samples (a row shorter than its padding is refused on the host: the clamp only keeps the address inside)
__device__ __forceinline__ float row_sample(const float* __restrict__ row, long long idx, long long L) {
    idx = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
    return row[idx];
}

// Two pieces of one row: the chunk holds the samples [chunk_origin, limit), the carry [carry_origin, chunk_origin).  Zero edges: a sample before 0, before the carry or from `limit` on is an exact 0.
struct SamplePieces {
    const float *carry, *chunk;
    long long carry_origin, chunk_origin, limit;
};
__device__ __forceinline__ float piece_sample(const SamplePieces& p, long long idx) {
    if (idx < 0 || idx < p.carry_origin || idx >= p.limit) return 0.f;
    const bool in_chunk = idx >= p.chunk_origin;
    const float* piece = in_chunk ? p.chunk : p.carry;
    const long long first = in_chunk ? p.chunk_origin : p.carry_origin;        // the piece holds the samples [first, last]
    const long long last = (in_chunk ? p.limit : p.chunk_origin) - 1;
    idx = idx < first ? first : (idx > last ? last : idx);
    return piece[idx - first];
}

// ---------------------------------------------------------------------------------------------
// yb[r][tp] = sample(tp, r) for the 32 x 32 slots of block (x: tp, y: r).  The read side has consecutive lanes on consecutive samples r, the
// write side on consecutive slots tp: the 32 x 33 LDS transpose keeps both coalesced.
// ---------------------------------------------------------------------------------------------
template <class Sample>
__device__ __forceinline__ void polyphase_tile(float* __restrict__ yb, int hop, int TP, Sample sample) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {   // read: consecutive lanes = consecutive samples (r) of frame slot t0 + i
        const int tp = t0 + i, r = r0 + tx;
        tile[i][tx] = tp < TP && r < hop ? sample(tp, r) : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {   // write: consecutive lanes = consecutive frame slots
        const int r = r0 + i, tp = t0 + tx;
        if (r < hop && tp < TP) yb[(long long)r * TP + tp] = tile[tx][i];
    }
}

// Log-mel front-end (fish_vocoder/data/transforms/spectrogram.py:25-56): reflect padding, 0 past the padded length L + pad_l + pad_r
__global__ __launch_bounds__(256) void polyphase_reflect_kernel(const float* __restrict__ wave, float* __restrict__ yp,
                                                                int L, int hop, int TP, int pad_l, int pad_r) {
    const int b = blockIdx.z;
    const float* wb = wave + (long long)b * L;
    const long long lpad = (long long)L + pad_l + pad_r;
    polyphase_tile(yp + (long long)b * hop * TP, hop, TP, [&](int tp, int r) {
        const long long pos = (long long)tp * hop + r;
        return pos < lpad ? row_sample(wb, reflect_index(pos - pad_l, L), L) : 0.f;
    });
}

fv_status launch_polyphase_reflect(const float* wave, float* yp, int B, int L, int hop, int TP, int pad_l, int pad_r, hipStream_t s) {
    hipLaunchKernelGGL(polyphase_reflect_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, B), dim3(256), 0, s, wave, yp, L, hop, TP,
                       pad_l, pad_r);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// The same on rows of different lengths and on chunks of a stream (spectrogram.py pads whole, equal-length rows; test.py:64-71 feeds it one file
// at a time).  Slot (tp, r) of row b is wave index (f0 + tp) hop + r - pad_l of that row.  With the row's end L_b known (len[b] >= 0) it reflects
// at L_b and everything from position L_b + pad_l + pad_r of the padded row on is an exact 0; with the end unknown (len[b] < 0: a stream's push)
// samples at or after `avail` are an exact 0 — only taps of zero weight reach them (fv_logmel_frames_ready).  A ragged call: chunk_origin = 0 and
// no carry.  The launcher refuses a NULL piece that is not empty.  Row offsets are 64-bit.
__global__ __launch_bounds__(256) void logmel_window_kernel(const float* __restrict__ carry, const float* __restrict__ chunk,
                                                            float* __restrict__ yp, const LogmelRowBlock rows, long long carry_stride,
                                                            long long chunk_stride, long long carry_origin, long long chunk_origin,
                                                            long long avail, long long f0, int hop, int TP, int pad_l, int pad_r, int b0) {
    const int b = b0 + blockIdx.z;
    const long long end = rows.e[blockIdx.z];
    const long long lpad = end >= 0 ? end + pad_l + pad_r : 0;    // the padded row's extent (known end only)
    const SamplePieces p{carry + (long long)b * carry_stride, chunk + (long long)b * chunk_stride, carry_origin, chunk_origin,
                         end >= 0 ? end : avail};
    polyphase_tile(yp + (long long)b * hop * TP, hop, TP, [&](int tp, int r) {
        const long long pos = (f0 + tp) * hop + r;
        return end >= 0 && pos >= lpad ? 0.f : piece_sample(p, reflect_index(pos - pad_l, end));
    });
}

fv_status launch_logmel_window(const float* carry, long long carry_stride, long long carry_origin, const float* chunk, long long chunk_stride,
                               long long chunk_origin, const long long* row_len, long long avail, float* yp, int B, long long f0, int hop,
                               int TP, int pad_l, int pad_r, hipStream_t s) {
    if (B <= 0 || TP <= 0) return FV_OK;
    long long limit = row_len ? 0 : avail;   // the last sample any row can select, plus one
    for (int b = 0; row_len && b < B; ++b) limit = std::max(limit, row_len[b]);
    if ((!chunk && limit > chunk_origin) || (!carry && chunk_origin > std::max(carry_origin, 0LL))) {
        set_error("logmel_window: internal: a piece that holds samples is NULL (%s)", chunk ? "carry" : "chunk");
        return FV_ERR_INVALID;
    }
    return for_each_launch_table<LogmelRowBlock>(B, [&](int b) { return row_len ? row_len[b] : -1LL; },
                                                 [&](const LogmelRowBlock& blk, int b0, int nz) {
        hipLaunchKernelGGL(logmel_window_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, nz), dim3(256), 0, s, carry, chunk, yp, blk,
                           carry_stride, chunk_stride, carry_origin, chunk_origin, avail, f0, hop, TP, pad_l, pad_r, b0);
        return FV_OK;
    });
}

// The same for sessions that advance independently (fv_wavpool_step; spectrogram.py:25-56 per session): tensor row k0 + blockIdx.z is one table
// entry — its own chunk row, its slot's carry in buf[bit], its own origins, end and first frame.  A row emits `count` frames out of the
// launch's T: the slots its frames read, tp < count + taps - 1, follow logmel_window_kernel's rule; the others load nothing and are exact zeros.
__global__ __launch_bounds__(256) void logmel_pool_window_kernel(const float* __restrict__ buf0, const float* __restrict__ buf1,
                                                                 const float* __restrict__ chunk, float* __restrict__ yp,
                                                                 const SamplePoolBlock tab, long long H, long long chunk_stride, int hop, int TP,
                                                                 int taps, int pad_l, int pad_r, int k0) {
    const SamplePoolEntry e = tab.e[blockIdx.z];
    const long long lpad = e.end >= 0 ? e.end + pad_l + pad_r : 0;    // the padded row's extent (known end only)
    const int used = e.count > 0 ? e.count + taps - 1 : 0;
    const SamplePieces p{(e.bit ? buf1 : buf0) + (long long)e.slot * H, chunk + (long long)e.item * chunk_stride, e.carry_origin,
                         e.chunk_origin, e.end >= 0 ? e.end : e.avail};
    polyphase_tile(yp + (long long)(k0 + blockIdx.z) * hop * TP, hop, TP, [&](int tp, int r) {
        if (tp >= used) return 0.f;
        const long long pos = (e.first + tp) * hop + r;
        return e.end >= 0 && pos >= lpad ? 0.f : piece_sample(p, reflect_index(pos - pad_l, e.end));
    });
}

fv_status launch_logmel_pool_window(const float* buf0, const float* buf1, long long H, const float* chunk, long long chunk_stride,
                                    const SamplePoolEntry* tab, int rows, float* yp, int hop, int TP, int taps, int pad_l, int pad_r,
                                    hipStream_t s) {
    if (rows <= 0 || TP <= 0) return FV_OK;
    for (int k = 0; k < rows; ++k) {
        const SamplePoolEntry& e = tab[k];
        if (e.count > TP - taps + 1 || e.chunk_origin - e.carry_origin != H || e.avail < e.chunk_origin ||
            (!chunk && e.avail > e.chunk_origin) || (chunk && e.avail - e.chunk_origin > chunk_stride)) {
            set_error("logmel_pool_window: internal: entry %d (session %d) does not fit its pieces", k, e.slot);
            return FV_ERR_INVALID;
        }
    }
    return for_each_launch_table<SamplePoolBlock>(rows, tab, [&](const SamplePoolBlock& blk, int k0, int nz) {
        hipLaunchKernelGGL(logmel_pool_window_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, nz), dim3(256), 0, s, buf0, buf1, chunk, yp, blk, H,
                           chunk_stride, hop, TP, taps, pad_l, pad_r, k0);
        return FV_OK;
    });
}

// The pitch shift's centred frames (pitch_shift.hip), zero edges: yp[b][r][tp] = wave[b][tp hop + r - pad] inside [0, L), else 0
__global__ __launch_bounds__(256) void pv_frame_kernel(const float* __restrict__ wave, float* __restrict__ yp, long long x_stride, long long L,
                                                       int hop, int TP, int pad) {
    const int b = blockIdx.z;
    const float* wb = wave + (long long)b * x_stride;
    polyphase_tile(yp + (long long)b * hop * TP, hop, TP, [&](int tp, int r) {
        const long long idx = (long long)tp * hop + r - pad;
        return idx >= 0 && idx < L ? row_sample(wb, idx, L) : 0.f;
    });
}

fv_status launch_pv_frame(const float* wave, long long x_stride, float* yp, int B, long long L, int hop, int TP, int pad, hipStream_t s) {
    hipLaunchKernelGGL(pv_frame_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, B), dim3(256), 0, s, wave, yp, x_stride, L, hop, TP, pad);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// The stream's: slot (tp, r) is sample (f0 + tp) hop + r - pad of row b, zeros before sample 0 and from `end` on.  The carry holds the samples
// [N - H, N), the chunk [N, end) (a push: end = N + c, no frame of the launch reaches it; the flush: end = N).
__global__ __launch_bounds__(256) void pv_frame_window_kernel(const float* __restrict__ carry, const float* __restrict__ chunk,
                                                              float* __restrict__ yp, long long carry_stride, long long chunk_stride, long long N,
                                                              int H, long long end, long long f0, int hop, int TP, int pad) {
    const int b = blockIdx.z;
    const SamplePieces p{carry + (long long)b * carry_stride, chunk + (long long)b * chunk_stride, N - H, N, end};
    polyphase_tile(yp + (long long)b * hop * TP, hop, TP,
                   [&](int tp, int r) { return piece_sample(p, (f0 + tp) * hop + r - pad); });
}

fv_status launch_pv_frame_window(const float* carry, long long carry_stride, const float* chunk, long long chunk_stride, float* yp, int B,
                                 long long N, int H, long long end, long long f0, int hop, int TP, int pad, hipStream_t s) {
    hipLaunchKernelGGL(pv_frame_window_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, B), dim3(256), 0, s, carry, chunk, yp, carry_stride,
                       chunk_stride, N, H, end, f0, hop, TP, pad);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// The pool's (fv_pvpool_step): tensor row k0 + blockIdx.z is one table entry — its own chunk row, its slot's carry in buf[bit], first frame A
// (first) and dA frames (count) out of the launch's TP - taps + 1.  What logmel_pool_window_kernel is to logmel_window_kernel, without the
// reflection: zeros before sample 0 and from `avail` on; the slots past tp = count + taps - 1 load nothing and are exact zeros.
__global__ __launch_bounds__(256) void pv_frame_pool_window_kernel(const float* __restrict__ buf0, const float* __restrict__ buf1,
                                                                   const float* __restrict__ chunk, float* __restrict__ yp,
                                                                   const SamplePoolBlock tab, long long H, long long chunk_stride, int hop, int TP,
                                                                   int taps, int pad, int k0) {
    const SamplePoolEntry e = tab.e[blockIdx.z];
    const int used = e.count > 0 ? e.count + taps - 1 : 0;
    const SamplePieces p{(e.bit ? buf1 : buf0) + (long long)e.slot * H, chunk + (long long)e.item * chunk_stride, e.carry_origin,
                         e.chunk_origin, e.avail};
    polyphase_tile(yp + (long long)(k0 + blockIdx.z) * hop * TP, hop, TP, [&](int tp, int r) {
        if (tp >= used) return 0.f;
        return piece_sample(p, (e.first + tp) * hop + r - pad);
    });
}

fv_status launch_pv_frame_pool_window(const float* buf0, const float* buf1, long long H, const float* chunk, long long chunk_stride,
                                      const SamplePoolEntry* tab, int rows, float* yp, int hop, int TP, int taps, int pad, hipStream_t s) {
    if (rows <= 0 || TP <= 0) return FV_OK;
    for (int k = 0; k < rows; ++k) {
        const SamplePoolEntry& e = tab[k];
        if (e.count < 0 || e.count > TP - taps + 1 || e.chunk_origin - e.carry_origin != H || e.avail < e.chunk_origin ||
            (!chunk && e.avail > e.chunk_origin) || (chunk && e.avail - e.chunk_origin > chunk_stride)) {
            set_error("pv_frame_pool_window: internal: entry %d (session %d) does not fit its pieces", k, e.slot);
            return FV_ERR_INVALID;
        }
    }
    return for_each_launch_table<SamplePoolBlock>(rows, tab, [&](const SamplePoolBlock& blk, int k0, int nz) {
        hipLaunchKernelGGL(pv_frame_pool_window_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, nz), dim3(256), 0, s, buf0, buf1, chunk, yp, blk, H,
                           chunk_stride, hop, TP, taps, pad, k0);
        return FV_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// Overlap-add + crop + envelope normalisation of vocos ISTFT("same").  The frames are already multiplied by the hann window (folded into the
// inverse-DFT basis); win2 = window^2 (n_fft).  Sample tau hop + r - pad sums frame(g hop + r, tau - g) in ascending g over the frames
// [0, Tend) that exist, tau = tau0 + ti a GLOBAL hop-frame index of type Idx, and lands at yb[sample - Y] if it lies in [Y, Y2).  Block (rt, tt)
// does 32 x 32 of (r, ti < n_tau); reads are coalesced along tau, the write is transposed through LDS so it is coalesced along r.
// frame(f, t) -> element f of frame t, for t in [0, Tend) only.
// ---------------------------------------------------------------------------------------------
template <class Idx, class Frame>
__device__ __forceinline__ void ola_tile(const float* __restrict__ win2, float* __restrict__ yb, int n_fft, int hop, int pad, Idx tau0, int n_tau,
                                         Idx Tend, long long Y, long long Y2, int rt, int tt, Frame frame) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int rr = ty; rr < 32; rr += 8) {
        const int r = rt * 32 + rr, ti = tt * 32 + tx;
        float acc = 0.f, env = 0.f;
        if (r < hop && ti < n_tau) {
            const Idx tau = tau0 + ti;
            for (int g = 0; g * hop + r < n_fft; ++g) {
                const Idx t = tau - g;
                if (t >= 0 && t < Tend) {
                    acc += frame(g * hop + r, t);
                    env += win2[g * hop + r];
                }
            }
        }
        tile[rr][tx] = env > 0.f ? acc / env : 0.f;
    }
    __syncthreads();
    for (int cc = ty; cc < 32; cc += 8) {
        const int ti = tt * 32 + cc, r = rt * 32 + tx;
        if (r < hop && ti < n_tau) {
            const long long sidx = (long long)(tau0 + ti) * hop + r - pad;
            if (sidx >= Y && sidx < Y2) yb[sidx - Y] = tile[tx][cc];
        }
    }
}

// one piece: frames (B, n_fft, T), every sample of [0, out_len)
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win2,
                                                        float* __restrict__ y, int n_fft, int T, int hop, int pad,
                                                        long long out_len, int r_tiles, int tau_tiles) {
    const int tt = blockIdx.x % tau_tiles, rt = blockIdx.x / tau_tiles % r_tiles, b = blockIdx.x / tau_tiles / r_tiles;
    const float* fb = frames + (long long)b * n_fft * T;
    const int n_tau = T + (n_fft + hop - 1) / hop;  // hop-frames touched by any analysis frame
    ola_tile<int>(win2, y + (long long)b * out_len, n_fft, hop, pad, 0, n_tau, T, 0, out_len, rt, tt,
                  [&](int f, int t) { return fb[(long long)f * T + t]; });
}

fv_status launch_istft_ola(const float* frames, const float* win2, float* y, int B, int n_fft, int T, int hop, int pad,
                           long long out_len, hipStream_t s) {
    const int r_tiles = (hop + 31) / 32;
    const int n_tau = T + (n_fft + hop - 1) / hop;
    const int tau_tiles = (n_tau + 31) / 32;
    hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)((long long)B * r_tiles * tau_tiles)), dim3(256), 0, s, frames,
                       win2, y, n_fft, T, hop, pad, out_len, r_tiles, tau_tiles);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// Element f of frame t from two pieces: the frames [S, ...) in `fb` (n_fft, ld), the frames [S - G, S) in the carried `cb` (n_fft, G)
__device__ __forceinline__ float two_piece_frame(const float* __restrict__ fb, long long ld, const float* __restrict__ cb, int G, long long S,
                                                 int f, long long t) {
    float v = 0.f;   // (a frame below S - G is never reached: fv_pv_stream_create's note on G)
    if (t >= S) v = fb[(long long)f * ld + (t - S)];
    else if (t >= S - G) v = cb[(long long)f * G + (t - (S - G))];
    return v;
}

// Two pieces, the stretched samples [Y, Y2) of a stream: frames [S, S + dS) from `frames` (B, n_fft, dS), frames [S - G, S) from the carried `cfr`
// (B, n_fft, G); the frames [0, Tend) exist.  During pushes Tend = S + dS cannot bind (every frame that covers a sample below Y2 exists); at
// the flush it is T'.
__global__ __launch_bounds__(256) void istft_ola_window_kernel(const float* __restrict__ frames, const float* __restrict__ cfr,
                                                               const float* __restrict__ win2, float* __restrict__ y, int n_fft, int hop, int pad,
                                                               int G, long long S, int dS, long long Tend, long long Y, long long Y2,
                                                               long long y_stride, long long tau0, int n_tau, int r_tiles, int tau_tiles) {
    const int tt = blockIdx.x % tau_tiles, rt = blockIdx.x / tau_tiles % r_tiles, b = blockIdx.x / tau_tiles / r_tiles;
    const float* fb = frames + (long long)b * n_fft * dS;
    const float* cb = cfr + (long long)b * n_fft * G;
    ola_tile<long long>(win2, y + (long long)b * y_stride, n_fft, hop, pad, tau0, n_tau, Tend, Y, Y2, rt, tt,
                        [&](int f, long long t) { return two_piece_frame(fb, dS, cb, G, S, f, t); });
}

fv_status launch_istft_ola_window(const float* frames, const float* cfr, const float* win2, float* y, int B, int n_fft, int hop, int pad, int G,
                                  long long S, int dS, long long Tend, long long Y, long long Y2, hipStream_t s) {
    const long long tau0 = (Y + pad) / hop;
    const int n_tau = (int)((Y2 - 1 + pad) / hop - tau0 + 1);
    const int r_tiles = (hop + 31) / 32, tau_tiles = (n_tau + 31) / 32;
    hipLaunchKernelGGL(istft_ola_window_kernel, dim3((unsigned)((long long)B * r_tiles * tau_tiles)), dim3(256), 0, s, frames, cfr, win2, y, n_fft,
                       hop, pad, G, S, dS, Tend, Y, Y2, Y2 - Y, tau0, n_tau, r_tiles, tau_tiles);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// Element e = f G + i of one row's next carry, frame S + dS - G + i: from the new frames `fb` (n_fft, ld) at or after S, from the carried
// `cb` (n_fft, G) below it, 0 before frame 0
__device__ __forceinline__ float frame_carry_value(const float* __restrict__ fb, long long ld, const float* __restrict__ cb, int G, long long S,
                                                   int dS, long long e) {
    const int f = (int)(e / G), i = (int)(e - (long long)f * G);
    const long long t = S + dS - G + i;
    float v = 0.f;
    if (t >= S) v = fb[(long long)f * ld + (t - S)];
    else if (t >= 0) v = cb[(long long)f * G + (t - (S - G))];
    return v;
}

// nfr[b][f][i] = frame S + dS - G + i: from the new frames at or after S, from the carried ones below it, 0 before frame 0
__global__ __launch_bounds__(256) void pv_frame_carry_kernel(const float* __restrict__ frames, const float* __restrict__ cfr,
                                                             float* __restrict__ nfr, int n_fft, int G, long long S, int dS) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_fft * G) return;
    const long long b = blockIdx.y;
    nfr[b * n_fft * G + e] = frame_carry_value(frames + b * n_fft * dS, dS, cfr + b * n_fft * G, G, S, dS, e);
}

fv_status launch_pv_frame_carry(const float* frames, const float* cfr, float* nfr, int B, int n_fft, int G, long long S, int dS, hipStream_t s) {
    hipLaunchKernelGGL(pv_frame_carry_kernel, dim3((unsigned)(((long long)n_fft * G + 255) / 256), B), dim3(256), 0, s, frames, cfr, nfr, n_fft, G,
                       S, dS);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// The pool's two (fv_pvpool_step): tensor row k0 + blockIdx.z is one table entry with its own S, dS, Tend and window [Y, Y2); the new frames
// are (rows, n_fft, ld) with ld the step's largest dS, the carried ones fr[fbit][slot].  An entry's n_tau follows from its own window; the grid
// spans the launch's largest, and a block past its entry's tiles leaves whole.
__global__ __launch_bounds__(256) void istft_ola_pool_window_kernel(const float* __restrict__ frames, const float* __restrict__ fr0,
                                                                    const float* __restrict__ fr1, const float* __restrict__ win2,
                                                                    float* __restrict__ y, const PvOlaBlock tab, int n_fft, int hop, int pad,
                                                                    int G, int ld, long long y_stride, int tau_tiles, int k0) {
    const PvOlaEntry e = tab.e[blockIdx.z];
    if (e.Y2 <= e.Y) return;
    const long long tau0 = (e.Y + pad) / hop;
    const int n_tau = (int)((e.Y2 - 1 + pad) / hop - tau0 + 1);
    const int tt = blockIdx.x % tau_tiles, rt = blockIdx.x / tau_tiles;
    if (tt * 32 >= n_tau) return;
    const long long row = k0 + blockIdx.z;
    const float* fb = frames + row * n_fft * ld;
    const float* cb = (e.fbit ? fr1 : fr0) + (long long)e.slot * n_fft * G;
    ola_tile<long long>(win2, y + row * y_stride, n_fft, hop, pad, tau0, n_tau, e.Tend, e.Y, e.Y2, rt, tt,
                        [&](int f, long long t) { return two_piece_frame(fb, ld, cb, G, e.S, f, t); });
}

__global__ __launch_bounds__(256) void pv_frame_pool_carry_kernel(const float* __restrict__ frames, float* fr0, float* fr1, const PvOlaBlock tab,
                                                                  int n_fft, int G, int ld, int k0) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const PvOlaEntry e = tab.e[blockIdx.y];
    if (i >= (long long)n_fft * G || e.dS <= 0) return;   // (a slot that synthesised no frame keeps its half and its bit)
    const long long slot = (long long)e.slot * n_fft * G;
    (e.fbit ? fr0 : fr1)[slot + i] = frame_carry_value(frames + (long long)(k0 + blockIdx.y) * n_fft * ld, ld, (e.fbit ? fr1 : fr0) + slot, G, e.S,
                                                       e.dS, i);
}

fv_status launch_pv_pool_ola(const float* frames, float* fr0, float* fr1, const float* win2, float* y, const PvOlaEntry* tab, int rows, int n_fft,
                             int hop, int pad, int G, int ld, long long y_stride, hipStream_t s) {
    if (rows <= 0) return FV_OK;
    for (int k = 0; k < rows; ++k) {
        const PvOlaEntry& e = tab[k];
        if (e.dS < 0 || e.dS > ld || e.Y2 < e.Y || e.Y2 - e.Y > y_stride || e.Tend > e.S + e.dS) {
            set_error("pv_pool_ola: internal: entry %d (session %d) does not fit its pieces", k, e.slot);
            return FV_ERR_INVALID;
        }
    }
    const int r_tiles = (hop + 31) / 32;
    return for_each_launch_table<PvOlaBlock>(rows, tab, [&](const PvOlaBlock& blk, int k0, int nz) {
        long long span = 0;
        bool carry = false;
        for (int i = 0; i < nz; ++i) {
            const PvOlaEntry& e = blk.e[i];
            if (e.Y2 > e.Y) span = std::max(span, (e.Y2 - 1 + pad) / hop - (e.Y + pad) / hop + 1);
            carry = carry || e.dS > 0;
        }
        if (span > 0) {
            const int tau_tiles = (int)((span + 31) / 32);
            hipLaunchKernelGGL(istft_ola_pool_window_kernel, dim3((unsigned)(r_tiles * tau_tiles), 1, nz), dim3(256), 0, s, frames, fr0, fr1, win2, y,
                               blk, n_fft, hop, pad, G, ld, y_stride, tau_tiles, k0);
        }
        if (carry)   // after the overlap-add in stream order; it writes the halves that one does not read
            hipLaunchKernelGGL(pv_frame_pool_carry_kernel, dim3((unsigned)(((long long)n_fft * G + 255) / 256), nz), dim3(256), 0, s, frames, fr0,
                               fr1, blk, n_fft, G, ld, k0);
        return FV_OK;
    });
}

// y[b][c][T_b ...) = 0.0f up to the row's end; T_b travels by value (rows.e), `span` = columns of the longest tail
__global__ __launch_bounds__(256) void zero_columns_kernel(float* __restrict__ y, const LogmelRowBlock rows, int C, long long T, int b0) {
    const long long j = rows.e[blockIdx.z] + (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    y[((long long)(b0 + blockIdx.z) * C + blockIdx.y) * T + j] = 0.0f;
}

fv_status launch_zero_columns(float* y, const long long* row_cols, int B, int C, long long T, hipStream_t s) {
    return for_each_launch_table<LogmelRowBlock>(B, [&](int b) { return std::min(std::max(row_cols[b], 0LL), T); },
                                                 [&](const LogmelRowBlock& blk, int b0, int nz) {
        long long span = 0;
        for (int i = 0; i < nz; ++i) span = std::max(span, T - blk.e[i]);
        if (span > 0) hipLaunchKernelGGL(zero_columns_kernel, dim3((unsigned)((span + 255) / 256), C, nz), dim3(256), 0, s, y, blk, C, T, b0);
        return FV_OK;
    });
}

}  // namespace fv
