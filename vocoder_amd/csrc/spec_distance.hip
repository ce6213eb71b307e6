// Spectrogram distances for scoring generated audio (include/fishvoc.h fv_spec_distance*): four sums per row over two (B, C, T) fp32 tensors
//   S_l1 = sum |est - ref|   S_sq = sum (est - ref)^2   S_ref = sum ref^2   S_log = sum |log ref - log est|      c < C, t < frames[b]
// from which the callers form eval.py:29-33's spec_diff (S_l1 / count on log-mels) and the two formulas of the STFT loss as metrics
// (stft.py:55 sqrt(S_sq) / sqrt(S_ref), stft.py:74 S_log / count on magnitudes).
//
// The first kernel of the project that reduces a row to a scalar.  The result must not depend on the batch, on T, on the strides or on the run,
// so there is no float atomic and no ticket: a fixed-order reduction in two launches (the launch boundary is the grid-wide barrier).
//   tile kernel   : one workgroup per (row, tile of kSdTile columns) -> four partial doubles in the workspace
//   finish kernel : per row, the partials added in tile order -> d_out[b][0..4)
// Order inside a tile: a lane is a column and a wave a channel, so the four waves of a workgroup take four channels per step; a thread walks
// its channels upwards with one fp64 accumulator per sum, then a butterfly over the 64 lanes of the wave (x + y is commutative: every lane
// ends with the same bits) and the four waves in order through LDS.  Columns past the row's end add an exact +0.0 and are never loaded, so the
// order is a function of C and of the tile's column count alone.
// Arithmetic: every term is formed in fp32 with one rounding per operation (the fp32 product is converted before it is added, so nothing
// contracts into an fma), widened, and accumulated in fp64.
// Loads: one fp32 per lane, 256 contiguous bytes per wave instruction, eight channels of both operands in flight per thread.  Nothing is
// assumed about alignment: the common spectrogram has an odd T (861 frames for 10 s), where 16-byte loads would serve only the first channel,
// and a second, wider path would need a second order of summation.  Memory-bound: each operand is read once.  All offsets are 64-bit.
#include <algorithm>
#include <cstdint>

#include "fv_internal.h"

namespace fv {

constexpr int kSdTile = 64;                          // columns per tile (fv_spec_distance_tile): one wave's lanes
constexpr int kSdThreads = 256;
constexpr int kSdWaves = kSdThreads / 64;            // channels per step
constexpr int kSdRows = 64;                          // rows per launch: their frame counts are a LaunchTable (fv_internal.h)
static_assert(kSdTile == 64, "a lane is a column");
static_assert(kSdRows * 4 == kSdThreads, "the finish kernel gives a row four threads, one per sum");

using SdRowBlock = LaunchTable<int, kSdRows>;

template <bool LOG>
__global__ __launch_bounds__(kSdThreads) void spec_distance_tile_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                        double* __restrict__ partial, const SdRowBlock rows,
                                                                        long long row_stride, long long ld, int C, long long tiles, int b0) {
    __shared__ double red[kSdWaves][4];
    const int frames = rows.e[blockIdx.y];
    const long long col0 = (long long)blockIdx.x * kSdTile;
    if (col0 >= frames) return;                                  // (the whole workgroup: nothing of this tile is loaded or written)
    const long long b = b0 + (long long)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s_l1 = 0.0, s_sq = 0.0, s_ref = 0.0, s_log = 0.0;
    if (col0 + lane < frames) {
        const long long base = b * row_stride + col0 + lane;
        const float* __restrict__ pe = est + base;
        const float* __restrict__ pr = ref + base;
#pragma unroll 8
        for (int c = wave; c < C; c += kSdWaves) {
            const float e = pe[(long long)c * ld], r = pr[(long long)c * ld];
            const float d = e - r;
            const float sq = d * d, rr = r * r;
            s_l1 += (double)fabsf(d);
            s_sq += (double)sq;
            s_ref += (double)rr;
            if (LOG) {
                const float lg = logf(r) - logf(e);
                s_log += (double)fabsf(lg);
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s_l1 += __shfl_xor(s_l1, m, 64);
        s_sq += __shfl_xor(s_sq, m, 64);
        s_ref += __shfl_xor(s_ref, m, 64);
        if (LOG) s_log += __shfl_xor(s_log, m, 64);
    }
    if (lane == 0) red[wave][0] = s_l1, red[wave][1] = s_sq, red[wave][2] = s_ref, red[wave][3] = s_log;
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSdWaves; ++w) s += red[w][threadIdx.x];
        partial[(b * tiles + blockIdx.x) * 4 + threadIdx.x] = s;
    }
}

// out[b][k] = partial[b][0][k] + partial[b][1][k] + ... in tile order; a row without frames reads nothing and gets four zeros
__global__ __launch_bounds__(kSdThreads) void spec_distance_finish_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                                          const SdRowBlock rows, long long tiles, int b0, int nrows) {
    const int i = threadIdx.x >> 2, k = threadIdx.x & 3;
    if (i >= nrows) return;
    const long long b = b0 + (long long)i;
    const int nt = (rows.e[i] + kSdTile - 1) / kSdTile;
    const double* p = partial + b * tiles * 4 + k;
    double s = 0.0;
    for (int t = 0; t < nt; ++t) s += p[(long long)t * 4];
    out[b * 4 + k] = s;
}

static long long sd_tiles(long long T) { return (T + kSdTile - 1) / kSdTile; }

static size_t sd_workspace_bytes(long long batch, long long T) {
    if (batch <= 0 || T <= 0) return 0;
    const unsigned long long raw = (unsigned long long)batch * (unsigned long long)sd_tiles(T) * 4 * sizeof(double);
    return (size_t)((raw + 255) / 256 * 256);
}

}  // namespace fv

using namespace fv;

extern "C" {

FV_API int32_t fv_spec_distance_tile(void) { return kSdTile; }

FV_API size_t fv_spec_distance_workspace_bytes(int32_t batch, int64_t T) { return sd_workspace_bytes(batch, T); }

FV_API fv_status fv_spec_distance(const float* d_est, const float* d_ref, int64_t row_stride, int64_t ld, int32_t channels, int64_t T,
                                  const int32_t* host_frames, int32_t batch, int32_t flags, double* d_out, void* d_workspace,
                                  size_t workspace_bytes, void* stream) {
    if (batch < 0 || T < 0) {
        set_error("fv_spec_distance: batch = %d and T = %lld must be >= 0", batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (batch == 0) return FV_OK;
    if (!d_est || !d_ref || !host_frames || !d_out) {
        set_error("fv_spec_distance: null argument (%s)", !d_est ? "d_est" : !d_ref ? "d_ref" : !host_frames ? "host_frames" : "d_out");
        return FV_ERR_INVALID;
    }
    if (flags & ~FV_SPEC_DISTANCE_LOG) {
        set_error("fv_spec_distance: unknown flags 0x%x", flags);
        return FV_ERR_INVALID;
    }
    if (channels < 1) {
        set_error("fv_spec_distance: channels = %d must be >= 1", channels);
        return FV_ERR_INVALID;
    }
    if (ld < T) {
        set_error("fv_spec_distance: ld = %lld is below T = %lld", (long long)ld, (long long)T);
        return FV_ERR_INVALID;
    }
    if (row_stride < 0 || row_stride / channels < ld) {      // (floor(row_stride / channels) < ld: the product is never formed)
        set_error("fv_spec_distance: row_stride = %lld is below channels * ld = %d * %lld", (long long)row_stride, channels, (long long)ld);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (host_frames[b] < 0 || host_frames[b] > T) {
            set_error("fv_spec_distance: frames[%d] = %d lies outside [0, T = %lld] (row %d)", b, host_frames[b], (long long)T, b);
            return FV_ERR_INVALID;
        }
    const size_t need = sd_workspace_bytes(batch, T);
    if (workspace_bytes < need || (need && !d_workspace)) {
        set_error("fv_spec_distance: the workspace holds %zu bytes, %d rows of %lld columns need %zu (fv_spec_distance_workspace_bytes)",
                  d_workspace ? workspace_bytes : (size_t)0, batch, (long long)T, need);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    auto tile_kernel = (flags & FV_SPEC_DISTANCE_LOG) ? spec_distance_tile_kernel<true> : spec_distance_tile_kernel<false>;
    const long long tiles = sd_tiles(T);
    double* partial = static_cast<double*>(d_workspace);
    return for_each_launch_table<SdRowBlock>(batch, host_frames, [&](const SdRowBlock& blk, int b0, int nz) -> fv_status {
        const int longest = *std::max_element(blk.e, blk.e + nz);
        if (longest > 0) {
            hipLaunchKernelGGL(tile_kernel, dim3((unsigned)sd_tiles(longest), nz), dim3(kSdThreads), 0, s, d_est, d_ref, partial, blk,
                               (long long)row_stride, (long long)ld, (int)channels, tiles, b0);
            FV_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(spec_distance_finish_kernel, dim3(1), dim3(kSdThreads), 0, s, partial, d_out, blk, tiles, b0, nz);
        return FV_OK;
    });
}

}  // extern "C"
