// The two steps of the reference's MMSEncoder (modules/encoders/mms.py) around its backbone (include/fishvoc.h fv_mms_*):
//   mms_partial / mms_apply   HF's zero_mean_unit_var_norm, y = (x - mean) / sqrt(var + 1e-7), each row over its own length
//   mms_interpolate           transpose(1, 2) + F.interpolate(mode="nearest"): time major (b, F, H) -> channel major (b, H, N)
// Both are bandwidth kernels.  Per-row counts travel by value (LaunchTable); nothing at or past a row's count is read, and the outputs hold
// exact zeros there.
//
// Normalisation.  A row is cut into segments of kMmsSeg samples.  mms_partial sums x and x^2 of one segment in fp64 (x^2 of an fp32 value
// is exact in fp64): thread t adds the quads t, t + 256, ... of the segment in index order, a butterfly adds the lanes of a wave, thread 0
// the four waves in order.  mms_apply re-adds the row's partials in ascending order (each wave for itself, a lane fetching one partial), forms mean and 1 / sqrt(var + 1e-7) in fp64, rounds
// both to fp32 once, and writes (x - mean) * rstd: one rounded subtraction, one rounded product.  The order of every sum is fixed by the
// row's length alone, and there are no atomics, so a row has the same bits alone, in any batch, in any row order and padded to any T.
// With T a multiple of 4 (and aligned pointers) whole quads move as 16 bytes; otherwise the same threads take the same elements one float
// at a time, so the two forms agree bit for bit.
//
// Interpolation.  A workgroup moves 64 output frames x 64 channels through a 16 KiB LDS tile: 16 lanes read the 64 channels of one source
// frame as float4 (256 contiguous bytes), the tile is stored channel major, and the write-out reads it back along the frames, so both
// sides of the transpose are contiguous in global memory.  The tile's column is XORed with 4 ((h >> 2) & 7): the four single-float stores of a
// loaded quad are then 2-way on the 32 store banks (free for a 4-byte store), and the 16-byte reads of the write-out, whose four rows
// share h >> 2, fall on 16 distinct 16-byte slots per lane group.  N a multiple of 4: 16-byte stores; otherwise one float per lane, 256
// contiguous bytes per wave.  The source frame is PyTorch's legacy rule, min((int)floorf(j * scale), F_b - 1), with scale = (float)F_b /
// (float)N_b from the host and the product one rounded fp32 multiply.
#include <cmath>

#include "fv_internal.h"

namespace fv {
namespace {

constexpr int kMmsRows = 128;                       // rows per launch: their counts are a LaunchTable
constexpr int kMmsSeg = 4096;                       // samples per segment: 256 threads x 4 quads
constexpr int kMmsTile = 64;                        // frames and channels per interpolation tile
constexpr long long kMmsMaxSamples = 1LL << 30;
constexpr int kMmsMaxChannels = 8192;
constexpr double kMmsEps = 1e-7;                    // HF's zero_mean_unit_var_norm

struct MmsFrames {
    int F, N;                                       // valid source frames and output frames of the row
    float scale;                                    // (float)F / (float)N, 0 where N = 0
};
using MmsFrameBlock = LaunchTable<MmsFrames, kMmsRows>;
using MmsLenBlock = LaunchTable<int, kMmsRows>;

// the quad [i, i + 4) of a row of `len` samples, zeros at and past len (which are not loaded)
template <bool VEC>
__device__ __forceinline__ float4 mms_load_quad(const float* xr, long long i, int len) {
    if (VEC && i + 4 <= len) return *reinterpret_cast<const float4*>(xr + i);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < len) v.x = xr[i];
    if (i + 1 < len) v.y = xr[i + 1];
    if (i + 2 < len) v.z = xr[i + 2];
    if (i + 3 < len) v.w = xr[i + 3];
    return v;
}

// part[(row, seg)] = (sum x, sum x^2) over the samples of segment `seg` below the row's length; segments at or past it are left alone
template <bool VEC>
__global__ __launch_bounds__(256) void mms_partial_kernel(const float* __restrict__ x, long long T, double2* __restrict__ part, int nseg, int row0,
                                                          const MmsLenBlock rows) {
    __shared__ double2 wsum[4];
    const int tid = threadIdx.x, bl = blockIdx.z;
    const int len = rows.e[bl];
    const long long i0 = (long long)blockIdx.x * kMmsSeg;
    if (i0 >= len) return;              // block-uniform
    const float* __restrict__ xr = x + (long long)(row0 + bl) * T;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < kMmsSeg / 1024; ++k) {
        const long long i = i0 + 4 * (tid + 256 * k);
        if (i >= len) break;
        const float4 v = mms_load_quad<VEC>(xr, i, len);
        const double a = v.x, b = v.y, c = v.z, d = v.w;            // zeros past the length change neither sum
        s += a, s += b, s += c, s += d;
        q += a * a, q += b * b, q += c * c, q += d * d;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64), q += __shfl_xor(q, m, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = make_double2(s, q);
    __syncthreads();
    if (tid == 0) {
        double2 t = wsum[0];
        for (int w = 1; w < 4; ++w) t.x += wsum[w].x, t.y += wsum[w].y;
        part[(long long)(row0 + bl) * nseg + blockIdx.x] = t;
    }
}

// y = (x - mean) * rstd below the row's length, 0.0f from there to T.  x == y is allowed: the sums were formed by an earlier launch.
template <bool VEC>
__global__ __launch_bounds__(256) void mms_apply_kernel(const float* x, float* y, long long T, const double2* __restrict__ part, int nseg, int row0,
                                                        const MmsLenBlock rows) {
    const int tid = threadIdx.x, bl = blockIdx.z;
    const int len = rows.e[bl];
    const long long i0 = (long long)blockIdx.x * kMmsSeg;
    const long long base = (long long)(row0 + bl) * T;
    float mean = 0.f, rstd = 0.f;
    if (i0 < len) {                     // block-uniform: every wave re-adds the row's partials in ascending order; a lane loads one of each
        const double2* __restrict__ pr = part + (long long)(row0 + bl) * nseg;      // 64, so the loads are not a chain
        const int ns = (len + kMmsSeg - 1) / kMmsSeg;
        double s = 0.0, q = 0.0;
        for (int k0 = 0; k0 < ns; k0 += 64) {
            const int k = k0 + (tid & 63), n = min(64, ns - k0);
            const double2 p = k < ns ? pr[k] : make_double2(0.0, 0.0);
            for (int j = 0; j < n; ++j) s += __shfl(p.x, j, 64), q += __shfl(p.y, j, 64);
        }
        const double m = s / (double)len;
        const double var = fmax(q / (double)len - m * m, 0.0);
        mean = (float)m;
        rstd = (float)(1.0 / sqrt(var + kMmsEps));
    }
#pragma unroll
    for (int k = 0; k < kMmsSeg / 1024; ++k) {
        const long long i = i0 + 4 * (tid + 256 * k);
        if (i >= T) break;
        float4 v = mms_load_quad<VEC>(x + base, i, len);
        v.x = i < len ? __fmul_rn(__fsub_rn(v.x, mean), rstd) : 0.f;
        v.y = i + 1 < len ? __fmul_rn(__fsub_rn(v.y, mean), rstd) : 0.f;
        v.z = i + 2 < len ? __fmul_rn(__fsub_rn(v.z, mean), rstd) : 0.f;
        v.w = i + 3 < len ? __fmul_rn(__fsub_rn(v.w, mean), rstd) : 0.f;
        float* yr = y + base + i;
        if (VEC) {                      // T is a multiple of 4: the quad lies inside the row
            *reinterpret_cast<float4*>(yr) = v;
        } else {
            yr[0] = v.x;
            if (i + 1 < T) yr[1] = v.y;
            if (i + 2 < T) yr[2] = v.z;
            if (i + 3 < T) yr[3] = v.w;
        }
    }
}

__device__ __forceinline__ int mms_tile_col(int h, int j) { return j ^ (4 * ((h >> 2) & 7)); }

// x: (b, F, H) -> y: (b, H, N); y[b][h][j] = j < N_b ? x[b][src(j)][h] : 0
template <bool VEC>
__global__ __launch_bounds__(256) void mms_interpolate_kernel(const float* __restrict__ x, float* __restrict__ y, long long F, int H, long long N, int row0,
                                                              const MmsFrameBlock rows) {
    __shared__ __attribute__((aligned(16))) float tile[kMmsTile * kMmsTile];        // [channel][frame ^ swizzle]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, bl = blockIdx.z;
    const long long b = row0 + bl;
    const int Fb = rows.e[bl].F, Nb = rows.e[bl].N;
    const float scale = rows.e[bl].scale;
    const int j0 = blockIdx.x * kMmsTile, h0 = blockIdx.y * kMmsTile;
    const bool live = j0 < Nb;          // block-uniform; a tile past the row's frames is all zeros and reads nothing
    if (live) {
        const int c4 = tid & 15, hl = 4 * c4;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int jl = (tid >> 4) + 16 * p, j = j0 + jl;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < Nb && h0 + hl < H) {            // H is a multiple of 4: the quad lies inside the frame
                const int src = min((int)floorf(__fmul_rn((float)j, scale)), Fb - 1);
                v = *reinterpret_cast<const float4*>(x + (b * F + src) * H + h0 + hl);
            }
            const int col = mms_tile_col(hl, jl);   // hl ... hl + 3 share h >> 2
            tile[(hl + 0) * kMmsTile + col] = v.x;
            tile[(hl + 1) * kMmsTile + col] = v.y;
            tile[(hl + 2) * kMmsTile + col] = v.z;
            tile[(hl + 3) * kMmsTile + col] = v.w;
        }
        __syncthreads();
    }
    if (VEC) {
        // a wave writes four channels x 64 frames: 16 lanes x 16 bytes per channel
        const int jl = 4 * (lane & 15), j = j0 + jl;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int hl = 16 * p + 4 * wave + (lane >> 4), h = h0 + hl;
            if (h >= H || j >= N) continue;         // N is a multiple of 4
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = *reinterpret_cast<const float4*>(&tile[hl * kMmsTile + mms_tile_col(hl, jl)]);
            *reinterpret_cast<float4*>(y + (b * H + h) * N + j) = v;
        }
    } else {
        // a wave writes one channel x 64 frames
        const int j = j0 + lane;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int hl = 4 * p + wave, h = h0 + hl;
            if (h >= H || j >= N) continue;
            y[(b * H + h) * N + j] = live ? tile[hl * kMmsTile + mms_tile_col(hl, lane)] : 0.f;
        }
    }
}

int mms_segments(long long T) { return (int)((T + kMmsSeg - 1) / kMmsSeg); }

fv_status mms_check_rows(const char* fn, int32_t batch, int64_t T) {
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kMmsMaxSamples || (long long)batch * T > kMmsMaxSamples) {
        set_error("%s: T = %lld must be >= 0 and batch * T at most 2^30 samples", fn, (long long)T);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

}  // namespace
}  // namespace fv

using namespace fv;

extern "C" {

FV_API int64_t fv_mms_nearest_index(int64_t F, int64_t N, int64_t j) {
    if (F < 1 || N < 1 || j < 0 || j >= N || F > kMmsMaxSamples || N > kMmsMaxSamples) return -1;
    const float scale = (float)F / (float)N;
    const int64_t src = (int64_t)floorf((float)j * scale);          // one rounded fp32 product, as the kernel's __fmul_rn
    return src < F - 1 ? src : F - 1;
}

FV_API size_t fv_mms_normalize_workspace_bytes(int32_t batch, int64_t T) {
    if (mms_check_rows("fv_mms_normalize_workspace_bytes", batch, T)) return 0;
    return (size_t)batch * (size_t)mms_segments(T) * sizeof(double2);
}

FV_API fv_status fv_mms_normalize(const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_y, void* d_workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* fn = "fv_mms_normalize";
    if (const fv_status st = mms_check_rows(fn, batch, T)) return st;
    for (int b = 0; host_lengths && b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > T) {
            set_error("%s: host_lengths[%d] = %d lies outside [0, T = %lld]", fn, b, host_lengths[b], (long long)T);
            return FV_ERR_INVALID;
        }
    if (batch == 0 || T == 0) return FV_OK;
    const int nseg = mms_segments(T);
    const size_t need = (size_t)batch * (size_t)nseg * sizeof(double2);
    if (workspace_bytes < need || !d_workspace) {
        set_error("%s: workspace of %zu bytes is smaller than the %zu that fv_mms_normalize_workspace_bytes(batch = %d, T = %lld) asks for", fn,
                  d_workspace ? workspace_bytes : (size_t)0, need, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (!d_x || !d_y) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : "d_y");
        return FV_ERR_INVALID;
    }
    if ((uintptr_t)d_workspace % 16 || ((uintptr_t)d_x | (uintptr_t)d_y) % 4) {
        set_error("%s: d_workspace must be 16-byte aligned, d_x and d_y 4-byte aligned", fn);
        return FV_ERR_INVALID;
    }
    // everything is validated: enqueue

    hipStream_t s = (hipStream_t)stream;
    double2* part = (double2*)d_workspace;
    const bool vec = T % 4 == 0 && ((uintptr_t)d_x | (uintptr_t)d_y) % 16 == 0;
    auto block = [&](const MmsLenBlock& lens, int row0, int nrows) -> fv_status {
        const dim3 grid((unsigned)nseg, 1, (unsigned)nrows);
        if (vec) {
            hipLaunchKernelGGL(mms_partial_kernel<true>, grid, dim3(256), 0, s, d_x, (long long)T, part, nseg, row0, lens);
            hipLaunchKernelGGL(mms_apply_kernel<true>, grid, dim3(256), 0, s, d_x, d_y, (long long)T, part, nseg, row0, lens);
        } else {
            hipLaunchKernelGGL(mms_partial_kernel<false>, grid, dim3(256), 0, s, d_x, (long long)T, part, nseg, row0, lens);
            hipLaunchKernelGGL(mms_apply_kernel<false>, grid, dim3(256), 0, s, d_x, d_y, (long long)T, part, nseg, row0, lens);
        }
        return FV_OK;
    };
    const fv_status st = for_each_launch_table<MmsLenBlock>(batch, [&](int b) { return host_lengths ? host_lengths[b] : (int)T; }, block);
    if (st == FV_OK) set_last_kernel("mms_apply_kernel");
    return st;
}

FV_API fv_status fv_mms_interpolate(const float* d_x, int64_t F, int32_t H, const int32_t* host_frames, const int32_t* host_out_frames,
                                    int32_t batch, float* d_y, int64_t N, void* stream) {
    const char* fn = "fv_mms_interpolate";
    if (batch < 0 || batch > 65535) {
        set_error("%s: batch = %d must lie in [0, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (H < 4 || H > kMmsMaxChannels || H % 4) {
        set_error("%s: H = %d must lie in [4, %d] and be a multiple of 4 (frames move as 16-byte quads)", fn, H, kMmsMaxChannels);
        return FV_ERR_INVALID;
    }
    if (F < 0 || F > kMmsMaxSamples || (long long)batch * F > kMmsMaxSamples) {
        set_error("%s: F = %lld must be >= 0 and batch * F at most 2^30 frames", fn, (long long)F);
        return FV_ERR_INVALID;
    }
    if (N < 0 || N > kMmsMaxSamples || (long long)batch * N > kMmsMaxSamples) {
        set_error("%s: N = %lld must be >= 0 and batch * N at most 2^30 frames", fn, (long long)N);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b) {
        const long long fb = host_frames ? host_frames[b] : F, nb = host_out_frames ? host_out_frames[b] : N;
        if (fb < 0 || fb > F) {
            set_error("%s: host_frames[%d] = %lld lies outside [0, F = %lld]", fn, b, fb, (long long)F);
            return FV_ERR_INVALID;
        }
        if (nb < 0 || nb > N) {
            set_error("%s: host_out_frames[%d] = %lld lies outside [0, N = %lld]", fn, b, nb, (long long)N);
            return FV_ERR_INVALID;
        }
        if (fb == 0 && nb > 0) {
            set_error("%s: row %d has no source frame (host_frames[%d] = 0) for its %lld output frames", fn, b, b, nb);
            return FV_ERR_INVALID;
        }
    }
    if (batch == 0 || N == 0) return FV_OK;
    if (!d_y || (!d_x && F > 0)) {
        set_error("%s: null %s", fn, !d_y ? "d_y" : "d_x");
        return FV_ERR_INVALID;
    }
    if ((uintptr_t)d_x % 16 || (uintptr_t)d_y % 4) {
        set_error("%s: d_x must be 16-byte aligned (frames move as 16-byte quads), d_y 4-byte aligned", fn);
        return FV_ERR_INVALID;
    }
    // everything is validated: enqueue

    hipStream_t s = (hipStream_t)stream;
    const bool vec = N % 4 == 0 && (uintptr_t)d_y % 16 == 0;
    auto block = [&](const MmsFrameBlock& rows, int row0, int nrows) -> fv_status {
        const dim3 grid((unsigned)((N + kMmsTile - 1) / kMmsTile), (unsigned)((H + kMmsTile - 1) / kMmsTile), (unsigned)nrows);
        if (vec) hipLaunchKernelGGL(mms_interpolate_kernel<true>, grid, dim3(256), 0, s, d_x, d_y, (long long)F, (int)H, (long long)N, row0, rows);
        else hipLaunchKernelGGL(mms_interpolate_kernel<false>, grid, dim3(256), 0, s, d_x, d_y, (long long)F, (int)H, (long long)N, row0, rows);
        return FV_OK;
    };
    auto entry = [&](int b) {
        MmsFrames e{};
        e.F = host_frames ? host_frames[b] : (int)F, e.N = host_out_frames ? host_out_frames[b] : (int)N;
        e.scale = e.N > 0 ? (float)e.F / (float)e.N : 0.f;
        return e;
    };
    const fv_status st = for_each_launch_table<MmsFrameBlock>(batch, entry, block);
    if (st == FV_OK) set_last_kernel("mms_interpolate_kernel");
    return st;
}

}  // extern "C"
