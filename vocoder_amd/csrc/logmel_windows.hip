// The device half of engine_logmel.hip: the log-mel front-end on rows of different lengths and on chunks of a stream
// (fish_vocoder/data/transforms/spectrogram.py:25-56 pads whole, equal-length rows; test.py:64-71 feeds it one file at a time).
//   logmel_window : the polyphase signal Yp[row][r][tp] of the frames [f0, f0 + n) of every row, with per-row edges
//   zero_columns  : columns >= T_b of a (B, C, T) result set to 0.0f
// HBM-bound copies: each lane moves one fp32.
#include <algorithm>

#include "fv_internal.h"

namespace fv {

// ---------------------------------------------------------------------------------------------
// Slot (tp, r) of row b is wave index idx = (f0 + tp) hop + r - pad_l of that row:
//   idx < 0 reflects to -idx; with the row's end L_b known (len[b] >= 0) idx >= L_b reflects to 2 (L_b - 1) - idx and everything from
//   position L_b + pad_l + pad_r of the padded row on is an exact 0; with the end unknown (len[b] < 0: a stream's push) samples at or after
//   `avail` are an exact 0 — only taps of zero weight reach them (fv_logmel_frames_ready).
// The sample comes from one of two pieces: the chunk holds the samples [chunk_origin, ...), the carry the samples [carry_origin, chunk_origin)
// (a ragged call: chunk_origin = 0 and no carry).  Neither piece is written here, so a push never writes the carry and reads it back in one
// launch (the session pool's rule).  A slot that takes no sample (zero padding, an empty row) loads nothing; a slot that takes one selects
// its piece and clamps the address into that piece, as polyphase_reflect_kernel clamps into its row, so whatever the caller left at or past
// L_b, or past the chunk (NaN included), never reaches a register.  The launcher refuses a NULL piece that is not empty.
// The read side has consecutive lanes on consecutive samples r, the write side on consecutive slots tp: the 32 x 33 LDS transpose of
// polyphase_reflect_kernel keeps both coalesced.  Row offsets are 64-bit.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void logmel_window_kernel(const float* __restrict__ carry, const float* __restrict__ chunk,
                                                            float* __restrict__ yp, const LogmelRowBlock rows, long long carry_stride,
                                                            long long chunk_stride, long long carry_origin, long long chunk_origin,
                                                            long long avail, long long f0, int hop, int TP, int pad_l, int pad_r, int b0) {
    __shared__ float tile[32][33];
    const int b = b0 + blockIdx.z;
    const int r0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long end = rows.len[blockIdx.z];
    const long long limit = end >= 0 ? end : avail;              // samples [lo, limit) of the row exist
    const long long lpad = end >= 0 ? end + pad_l + pad_r : 0;    // the padded row's extent (known end only)
    for (int i = ty; i < 32; i += 8) {   // read: consecutive lanes = consecutive samples (r) of frame slot t0 + i
        const int tp = t0 + i, r = r0 + tx;
        float v = 0.f;
        if (tp < TP && r < hop) {
            const long long pos = (f0 + tp) * hop + r;
            long long idx = pos - pad_l;
            if (idx < 0) idx = -idx;
            bool valid = true;
            if (end >= 0) {
                valid = pos < lpad;
                if (idx >= end) idx = 2 * (end - 1) - idx;
            }
            valid = valid && idx >= 0 && idx >= carry_origin && idx < limit;   // (a row shorter than its padding is refused on the host)
            if (valid) {
                const bool in_chunk = idx >= chunk_origin;
                const float* piece = in_chunk ? chunk + (long long)b * chunk_stride : carry + (long long)b * carry_stride;
                const long long first = in_chunk ? chunk_origin : carry_origin;        // the piece holds the samples [first, last]
                const long long last = (in_chunk ? limit : chunk_origin) - 1;
                idx = idx < first ? first : (idx > last ? last : idx);
                v = piece[idx - first];
            }
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    float* yb = yp + (long long)b * hop * TP;
    for (int i = ty; i < 32; i += 8) {   // write: consecutive lanes = consecutive frame slots
        const int r = r0 + i, tp = t0 + tx;
        if (r < hop && tp < TP) yb[(long long)r * TP + tp] = tile[tx][i];
    }
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
    for (int b0 = 0; b0 < B; b0 += kLogmelRows) {
        const int nz = std::min(kLogmelRows, B - b0);
        LogmelRowBlock blk{};
        for (int i = 0; i < nz; ++i) blk.len[i] = row_len ? row_len[b0 + i] : -1;
        hipLaunchKernelGGL(logmel_window_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, nz), dim3(256), 0, s, carry, chunk, yp, blk,
                           carry_stride, chunk_stride, carry_origin, chunk_origin, avail, f0, hop, TP, pad_l, pad_r, b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

// y[b][c][T_b ...) = 0.0f up to the row's end; T_b travels by value (rows.len), `span` = columns of the longest tail
__global__ __launch_bounds__(256) void zero_columns_kernel(float* __restrict__ y, const LogmelRowBlock rows, int C, long long T, int b0) {
    const long long j = rows.len[blockIdx.z] + (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    y[((long long)(b0 + blockIdx.z) * C + blockIdx.y) * T + j] = 0.0f;
}

fv_status launch_zero_columns(float* y, const long long* row_cols, int B, int C, long long T, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += kLogmelRows) {
        const int nz = std::min(kLogmelRows, B - b0);
        LogmelRowBlock blk{};
        long long span = 0;
        for (int i = 0; i < nz; ++i) {
            blk.len[i] = std::min(std::max(row_cols[b0 + i], 0LL), T);
            span = std::max(span, T - blk.len[i]);
        }
        if (span <= 0) continue;
        hipLaunchKernelGGL(zero_columns_kernel, dim3((unsigned)((span + 255) / 256), C, nz), dim3(256), 0, s, y, blk, C, T, b0);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

}  // namespace fv
