// Sample-rate conversion (fv_resample_*, include/fishvoc.h): the polyphase windowed-sinc resampler of torchaudio.transforms.Resample as a banded
// FIR on the vector ALU.  Host: the filter design in float64 (fv_resample_design, no GPU), the object, the stream, the pool of sessions
// (fv_respool_*).  Device: one kernel body for whole rows and one for a pool's items, each in two forms (table staged in LDS / read from global
// memory), around one output loop.
//
// Output m = f n + p reads x[f o + first[p] - width + i], i < count[p] (count <= Kp: 13 taps for 44100 -> 48000, 73 for 48000 -> 8000), where the
// dense form of the reference holds 2 width + o = 161 ... 475 taps per output, all but the band zero: an MFMA GEMM over the dense form would do
// 7 - 14 times the work, so this is a VALU kernel bound by LDS reads (two per multiply-add) and memory.
//
// Tiling.  s(m) = f o + first[p] (the first input sample of output m, shifted by width so that it is never negative) does not decrease with m.
// Tile t of a launch owns the outputs with s(m) in [X0 + t kResTile, X0 + (t + 1) kResTile): a contiguous range of m, found in the kernel from
// first[] alone (count_below), that reads the input samples [X - width, X - width + kResTile + Kp - 1).  The workgroup stages the table and that span
// in LDS (16-byte loads from 16-byte boundaries of memory, whatever the row's own alignment; samples outside the row's [0, length) are zeros and never loaded) and consecutive lanes write
// consecutive m.  All index arithmetic across a row is 64-bit: m o passes 2^31 on long clips.
//
// Summation order: ascending i in one accumulator, fmaf — a function of the phase alone.  Tiles, rows, launch sizes and a stream's chunking
// change which workgroup computes an output, never its value: that is what the bit-identity guarantees of the header rest on.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "sample_pool.h"

namespace fv {
namespace {

constexpr int kResTile = 4096;      // input samples per tile (fv_resample_input_tile)
constexpr int kResThreads = 256;
constexpr size_t kResLdsBudget = 64 * 1024;   // table + staged tile per workgroup: two workgroups per CU beside each other in 160 KiB

// #{(f, p) : f >= 0, 0 <= p < n, f o + arr[p] < X} for a non-decreasing arr >= 0 (first[]: the outputs that start before X; first[] + count[]:
// the outputs whose band has ended)
template <class T>
__host__ __device__ inline long long count_below(const T* arr, int n, int o, long long X) {
    const long long amin = arr[0], amax = arr[n - 1];
    if (X <= amin) return 0;
    const long long full = X > amax ? (X - amax + o - 1) / o : 0;   // frames f < full have every phase below X
    long long total = full * n;
    for (long long f = full; f * o + amin < X; ++f) {
        const long long r = X - f * o;
        int lo = 0, hi = n;                                       // first p with arr[p] >= r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (arr[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        total += lo;
    }
    return total;
}

struct ResampleParams {
    const float* x;            // rows of input columns; column c of a row is the input sample in_origin + c
    float* y;                  // rows of outputs; column 0 is output m_begin
    const int* lengths;        // per-row input length (NULL: len for every row)
    const uint32_t* table;     // first[n], count[n], taps[n][kpad], padded to a multiple of 4 dwords
    long long x_stride, y_stride;
    long long len;             // input samples of a row (the clamp of lengths[])
    long long in_origin;       // may be negative (a stream's first pushes): samples before 0 are zeros
    long long m_begin, m_end;
    long long X0;              // s(m_begin)
    int ntiles;
    int o, n, width, kpad, table_dwords, sx;   // sx: staged samples, a multiple of 4
};

// how the kernel holds its table: plain pointers into LDS (staged by the workgroup itself), or __restrict__ pointers into global memory that
// nothing writes during the launch
template <bool kGlobalTable>
struct TablePtr {
    using I = const int*;
    using F = const float*;
};
template <>
struct TablePtr<true> {
    using I = const int* __restrict__;
    using F = const float* __restrict__;
};

// The outputs [m_lo, m_hi) of one tile, lane `tid` taking every kResThreads-th: the sum of every kernel in this file, whole rows and pools alike.
// s_x[0] is the input sample X - width - shift of the row; outputs from M_b on are zeros (a ragged row's tail); yr[m] is where output m goes.
template <bool kGlobalTable>
__device__ __forceinline__ void resample_tile_outputs(typename TablePtr<kGlobalTable>::I s_first, typename TablePtr<kGlobalTable>::I s_count,
                                                      typename TablePtr<kGlobalTable>::F s_taps, const float* s_x, int n, int o, int kpad,
                                                      long long X, int shift, long long m_lo, long long m_hi, long long M_b, float* yr, int tid) {
    long long m = m_lo + tid;
    if (m >= m_hi) return;
    const long long f0 = m / n;
    int ph = (int)(m - f0 * n);
    int base = (int)(f0 * o - X) + shift;             // LDS index of the sample f o - width
    const int dp = kResThreads % n, db = (kResThreads / n) * o;
    for (; m < m_hi; m += kResThreads) {
        float acc = 0.f;
        if (m < M_b) {
            const float* xs = s_x + base + s_first[ph];
            const float* tp = s_taps + ph * kpad;
            const int cnt = s_count[ph];
            // (unrolled by four so that the LDS reads of four taps are in flight together; the sum stays one ascending chain)
#pragma unroll 4
            for (int i = 0; i < cnt; ++i) acc = fmaf(tp[i], xs[i], acc);
        }
        yr[m] = acc;
        ph += dp;
        base += db;
        if (ph >= n) {
            ph -= n;
            base += o;
        }
    }
}

// kGlobalTable: first[], count[] and the taps are read where they lie, in global memory (fv_global_resample_create: a table of any size, served
// by L2), and LDS holds the input tile alone.  Tiling, indices and the sum of an output are the same statements in both forms.
template <bool kGlobalTable>
__device__ __forceinline__ void resample_body(const ResampleParams& p) {
    extern __shared__ __align__(16) uint32_t smem[];
    const uint32_t* table = kGlobalTable ? p.table : smem;
    const typename TablePtr<kGlobalTable>::I s_first = (const int*)table;
    const typename TablePtr<kGlobalTable>::I s_count = s_first + p.n;
    const typename TablePtr<kGlobalTable>::F s_taps = (const float*)(s_count + p.n);
    float* s_x = (float*)(smem + (kGlobalTable ? 0 : p.table_dwords));
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % p.ntiles;
    const long long row = blockIdx.x / p.ntiles;

    if (!kGlobalTable)
        for (int q = tid; q < p.table_dwords / 4; q += kResThreads) ((uint4*)smem)[q] = ((const uint4*)p.table)[q];

    long long len_b = p.len;
    if (p.lengths) len_b = min((long long)max(p.lengths[row], 0), p.len);
    const long long M_b = p.lengths ? min(p.m_end, (len_b * p.n + p.o - 1) / p.o) : p.m_end;   // the row's own outputs; zeros follow

    const long long X = p.X0 + (long long)tile * kResTile;
    const long long a0 = X - p.width - p.in_origin;   // column of the first sample this tile reads
    const float* xr = p.x + row * p.x_stride;
    const int mis = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3);   // the row's own offset from a 16-byte boundary, in floats
    const int shift = (int)((a0 + mis) & 3);
    const long long c0 = a0 - shift;                  // ... moved down to a 16-byte boundary of memory: xr + c0 is aligned
    const long long vlo = p.in_origin < 0 ? -p.in_origin : 0;   // valid columns [vlo, vhi): the samples [0, len_b)
    const long long vhi = len_b - p.in_origin;
    for (int q = tid; q < p.sx / 4; q += kResThreads) {
        const long long c = c0 + 4 * q;
        float4 v;
        if (c >= vlo && c + 4 <= vhi) {
            v = *(const float4*)(xr + c);
        } else {
            v.x = (c >= vlo && c < vhi) ? xr[c] : 0.f;
            v.y = (c + 1 >= vlo && c + 1 < vhi) ? xr[c + 1] : 0.f;
            v.z = (c + 2 >= vlo && c + 2 < vhi) ? xr[c + 2] : 0.f;
            v.w = (c + 3 >= vlo && c + 3 < vhi) ? xr[c + 3] : 0.f;
        }
        ((float4*)s_x)[q] = v;
    }
    __syncthreads();

    const long long m_lo = tile == 0 ? p.m_begin : max(p.m_begin, count_below(s_first, p.n, p.o, X));
    const long long m_hi = tile == p.ntiles - 1 ? p.m_end : min(p.m_end, count_below(s_first, p.n, p.o, X + kResTile));
    resample_tile_outputs<kGlobalTable>(s_first, s_count, s_taps, s_x, p.n, p.o, p.kpad, X, shift, m_lo, m_hi, M_b,
                                        p.y + row * p.y_stride - p.m_begin, tid);
}

__global__ __launch_bounds__(kResThreads) void resample_kernel(const ResampleParams p) { resample_body<false>(p); }
__global__ __launch_bounds__(kResThreads) void resample_global_kernel(const ResampleParams p) { resample_body<true>(p); }

// ---------------------------------------------------------------------------------------------
// The pool form (fv_respool_step): one launch serves up to kSamplePoolBlock items, each a session with its own counters.  blockIdx.y picks the
// item's entry (by value, fv_internal.h: first = E, count = E' - E, carry_origin = N - H, chunk_origin = N, avail = N'), blockIdx.x its tile:
// entry k owns the tiles of [s(E), s(E' - 1)], split as resample_run splits a row's, and finds X0 = s(first) and its own tile count from first[]
// (read from global memory: the LDS copy is not staged yet).  The grid is as wide as the block's largest tile count; a workgroup past its
// entry's last tile only stores its share of the zero tail.  A tile's samples come from two places: sample j >= chunk_origin from
// chunk[item][j - chunk_origin], 0 <= j < chunk_origin from the slot's carry buf[bit][slot][j - carry_origin], and j < 0 or j >= avail is 0.0f and
// never loaded.  fv_respool_step has checked that no output of the step reads below carry_origin; the up to three samples that only the
// 16-byte alignment puts in front of the first tile are staged as zeros rather than loaded.
// ---------------------------------------------------------------------------------------------
struct ResamplePoolParams {
    const float* chunk;        // (items, chunk_stride); NULL when no entry's chunk holds a sample
    const float* buf0;         // the pool's two (S, H) carry buffers
    const float* buf1;
    float* y;                  // (items, y_stride): columns [0, out_cols) of an entry's row are written
    const uint32_t* table;
    long long chunk_stride, y_stride, H;
    int out_cols, max_tiles;
    int o, n, width, kpad, table_dwords, sx;
};

template <bool kGlobalTable>
__device__ __forceinline__ void resample_pool_body(const ResamplePoolParams& p, const SamplePoolBlock& tab) {
    extern __shared__ __align__(16) uint32_t smem[];
    const uint32_t* table = kGlobalTable ? p.table : smem;
    const typename TablePtr<kGlobalTable>::I s_first = (const int*)table;
    const typename TablePtr<kGlobalTable>::I s_count = s_first + p.n;
    const typename TablePtr<kGlobalTable>::F s_taps = (const float*)(s_count + p.n);
    float* s_x = (float*)(smem + (kGlobalTable ? 0 : p.table_dwords));
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const SamplePoolEntry e = tab.e[blockIdx.y];
    float* yrow = p.y + (long long)e.item * p.y_stride;

    // the zero tail [count, out_cols) of the row, shared among the max_tiles workgroups of the entry
    for (long long c = e.count + (long long)tile * kResThreads + tid; c < p.out_cols; c += (long long)p.max_tiles * kResThreads) yrow[c] = 0.f;
    if (e.count <= 0) return;

    const int* g_first = (const int*)p.table;
    const long long m_begin = e.first, m_end = e.first + e.count;
    const long long X0 = (m_begin / p.n) * p.o + g_first[m_begin % p.n];
    const long long X_last = ((m_end - 1) / p.n) * p.o + g_first[(m_end - 1) % p.n];
    const int ntiles = (int)((X_last - X0) / kResTile) + 1;
    if (tile >= ntiles) return;

    if (!kGlobalTable)
        for (int q = tid; q < p.table_dwords / 4; q += kResThreads) ((uint4*)smem)[q] = ((const uint4*)p.table)[q];

    const long long X = X0 + (long long)tile * kResTile;
    const long long j0 = X - p.width;                 // the first sample this tile reads
    const long long chunk_len = e.avail - e.chunk_origin;
    const float* cr = chunk_len > 0 ? p.chunk + (long long)e.item * p.chunk_stride : nullptr;
    const float* carry = (e.bit ? p.buf1 : p.buf0) + (long long)e.slot * p.H;
    const int mis = (int)((reinterpret_cast<uintptr_t>(cr) >> 2) & 3);   // the chunk row's own offset from a 16-byte boundary, in floats
    const int shift = (int)((j0 - e.chunk_origin + mis) & 3);
    const long long js = j0 - shift;                  // ... moved down so that cr + (js - chunk_origin) lies on a 16-byte boundary of memory
    const long long lo = max(0LL, e.carry_origin);    // samples [lo, chunk_origin) are carried, [chunk_origin, avail) lie in the chunk
    auto sample = [&](long long j) -> float {
        if (j < lo || j >= e.avail) return 0.f;
        return j >= e.chunk_origin ? cr[j - e.chunk_origin] : carry[j - e.carry_origin];
    };
    for (int q = tid; q < p.sx / 4; q += kResThreads) {
        const long long j = js + 4 * q;
        float4 v;
        if (j >= e.chunk_origin && j + 4 <= e.avail) {
            v = *(const float4*)(cr + (j - e.chunk_origin));
        } else {
            v.x = sample(j);
            v.y = sample(j + 1);
            v.z = sample(j + 2);
            v.w = sample(j + 3);
        }
        ((float4*)s_x)[q] = v;
    }
    __syncthreads();

    const long long m_lo = tile == 0 ? m_begin : max(m_begin, count_below(s_first, p.n, p.o, X));
    const long long m_hi = tile == ntiles - 1 ? m_end : min(m_end, count_below(s_first, p.n, p.o, X + kResTile));
    resample_tile_outputs<kGlobalTable>(s_first, s_count, s_taps, s_x, p.n, p.o, p.kpad, X, shift, m_lo, m_hi, m_end, yrow - m_begin, tid);
}

__global__ __launch_bounds__(kResThreads) void resample_pool_kernel(const ResamplePoolParams p, const SamplePoolBlock tab) {
    resample_pool_body<false>(p, tab);
}
__global__ __launch_bounds__(kResThreads) void resample_pool_global_kernel(const ResamplePoolParams p, const SamplePoolBlock tab) {
    resample_pool_body<true>(p, tab);
}

constexpr double kKaiserBeta = 14.769656459379492;

double bessel_i0(double x) {   // sum_k ((x / 2)^k / k!)^2
    const double q = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

struct Design {
    int o = 0, n = 0, width = 0, kp = 0;
    std::vector<int> first, count;
    std::vector<float> taps;   // n x kp
};

fv_status check_config(const fv_resample_config* c, const char* fn) {
    if (!c) {
        set_error("%s: null config", fn);
        return FV_ERR_INVALID;
    }
    if (c->orig_freq <= 0) {
        set_error("%s: orig_freq = %d must be > 0", fn, c->orig_freq);
        return FV_ERR_INVALID;
    }
    if (c->new_freq <= 0) {
        set_error("%s: new_freq = %d must be > 0", fn, c->new_freq);
        return FV_ERR_INVALID;
    }
    if (c->lowpass_filter_width < 1) {
        set_error("%s: lowpass_filter_width = %d must be >= 1", fn, c->lowpass_filter_width);
        return FV_ERR_INVALID;
    }
    if (!(c->rolloff > 0.0 && c->rolloff <= 1.0)) {
        set_error("%s: rolloff = %g must lie in (0, 1]", fn, c->rolloff);
        return FV_ERR_INVALID;
    }
    if (c->method != FV_RESAMPLE_SINC_HANN && c->method != FV_RESAMPLE_SINC_KAISER) {
        set_error("%s: method = %d is neither FV_RESAMPLE_SINC_HANN (0) nor FV_RESAMPLE_SINC_KAISER (1)", fn, c->method);
        return FV_ERR_INVALID;
    }
    if (std::isnan(c->beta)) {
        set_error("%s: beta is NaN", fn);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// sizes and the band of every phase; the taps only when asked (the band alone costs n * Kp evaluations, never the dense n * (2 width + o))
fv_status design(const fv_resample_config* c, const char* fn, Design& d, bool with_taps) {
    if (const fv_status r = check_config(c, fn)) return r;
    const int g = std::gcd(c->orig_freq, c->new_freq);
    const int o = c->orig_freq / g, n = c->new_freq / g, lpw = c->lowpass_filter_width;
    const double base = std::min(o, n) * c->rolloff;
    const double wd = std::ceil(lpw * (double)o / base);
    if (wd > (double)(1 << 24)) {
        set_error("%s: %d -> %d Hz needs a filter of half width %.0f input samples, more than 2^24", fn, c->orig_freq, c->new_freq, wd);
        return FV_ERR_UNSUPPORTED;
    }
    const int width = (int)wd;
    const long long dense = 2LL * width + o;
    const double half = lpw * (double)o / base;
    auto t_of = [&](long long j, int p) { return ((double)(j - width) / o - (double)p / n) * base; };
    d.o = o, d.n = n, d.width = width, d.kp = 0;
    d.first.assign(n, 0);
    d.count.assign(n, 0);
    for (int p = 0; p < n; ++p) {
        const double centre = width + (double)p * o / n;
        const long long jlo = std::max(0LL, (long long)std::floor(centre - half) - 2);
        const long long jhi = std::min(dense - 1, (long long)std::ceil(centre + half) + 2);
        long long first = -1, last = -1;
        for (long long j = jlo; j <= jhi; ++j)
            if (std::fabs(t_of(j, p)) < lpw) {      // the band, by its definition: the computed window is 4e-33 at its edge, not 0
                if (first < 0) first = j;
                last = j;
            }
        if (first < 0) {
            set_error("%s: internal: phase %d of %d -> %d Hz has an empty band", fn, p, c->orig_freq, c->new_freq);
            return FV_ERR_INVALID;
        }
        d.first[p] = (int)first;
        d.count[p] = (int)(last - first + 1);
        d.kp = std::max(d.kp, d.count[p]);
    }
    for (int p = 1; p < n; ++p)
        if (d.first[p] < d.first[p - 1] || d.first[p] + d.count[p] < d.first[p - 1] + d.count[p - 1]) {
            set_error("%s: internal: the bands of %d -> %d Hz do not advance with the phase at p = %d", fn, c->orig_freq, c->new_freq, p);
            return FV_ERR_INVALID;
        }
    if (d.first[n - 1] > d.first[0] + o || d.first[n - 1] + d.count[n - 1] > d.first[0] + d.count[0] + o) {
        set_error("%s: internal: the bands of %d -> %d Hz do not advance from one frame to the next", fn, c->orig_freq, c->new_freq);
        return FV_ERR_INVALID;
    }
    if (!with_taps) return FV_OK;
    const double beta = c->beta > 0 ? c->beta : kKaiserBeta, i0b = bessel_i0(beta), scale = base / o;
    d.taps.assign((size_t)n * d.kp, 0.f);
    for (int p = 0; p < n; ++p)
        for (int i = 0; i < d.count[p]; ++i) {
            double t = t_of(d.first[p] + i, p);
            t = std::min(std::max(t, (double)-lpw), (double)lpw);
            double win;
            if (c->method == FV_RESAMPLE_SINC_HANN) {
                const double cs = std::cos(t * M_PI / lpw / 2);
                win = cs * cs;
            } else {
                const double u = t / lpw;
                win = bessel_i0(beta * std::sqrt(std::max(0.0, 1 - u * u))) / i0b;
            }
            t *= M_PI;
            const double sinc = t == 0 ? 1.0 : std::sin(t) / t;
            d.taps[(size_t)p * d.kp + i] = (float)(sinc * win * scale);
        }
    return FV_OK;
}

}  // namespace
}  // namespace fv

using namespace fv;

struct fv_resample {
    fv_resample_config cfg{};
    Design d;
    std::vector<int> end;       // first[] + count[]
    int kpad = 0, table_dwords = 0, sx = 0;
    uint32_t* d_table = nullptr;
    bool global_table = false;   // fv_global_resample_create: the kernel reads the table from global memory
    ~fv_resample() {
        if (d_table) (void)hipFree(d_table);
    }
    long long s_of(long long m) const { return (m / d.n) * d.o + d.first[(size_t)(m % d.n)]; }
    long long out_len(long long L) const { return (L * d.n + d.o - 1) / d.o; }
    long long emit_count(long long N) const { return count_below(end.data(), d.n, d.o, N + d.width + 1); }
};

// the core's buffers are the work buffers [last H samples | chunk] with row stride H + max_chunk rounded up to 4: buf[cur] holds the samples
// [N - H - prev_c, N)
struct fv_resample_stream : SampleStream {
    fv_resample* r = nullptr;
    int prev_c = 0;
};

static constexpr long long kResMaxLen = kSampleStreamMaxLen;   // n L stays far inside 64 bits

// outputs [m_begin, m_end) of every row into y columns [0, m_end - m_begin)
static fv_status resample_run(const fv_resample* r, const char* fn, const float* x, long long x_stride, long long in_origin, const int* d_lengths,
                              long long len, float* y, long long y_stride, int batch, long long m_begin, long long m_end, hipStream_t s) {
    if (batch <= 0 || m_end <= m_begin) return FV_OK;
    ResampleParams p{};
    p.x = x, p.y = y, p.lengths = d_lengths, p.table = r->d_table;
    p.x_stride = x_stride, p.y_stride = y_stride, p.len = len, p.in_origin = in_origin;
    p.m_begin = m_begin, p.m_end = m_end, p.X0 = r->s_of(m_begin);
    const long long ntiles = (r->s_of(m_end - 1) - p.X0) / kResTile + 1;
    if (ntiles * batch >= (1LL << 24)) {
        set_error("%s: %lld tiles x %d rows, more than 2^24 workgroups in one launch; split the batch", fn, ntiles, batch);
        return FV_ERR_UNSUPPORTED;
    }
    p.ntiles = (int)ntiles;
    p.o = r->d.o, p.n = r->d.n, p.width = r->d.width, p.kpad = r->kpad, p.table_dwords = r->table_dwords, p.sx = r->sx;
    if (r->global_table) {
        hipLaunchKernelGGL(resample_global_kernel, dim3((unsigned)(ntiles * batch)), dim3(kResThreads), (size_t)r->sx * 4, s, p);
        FV_HIP_CHECK(hipGetLastError());
        set_last_kernel("resample_global_kernel");
        return FV_OK;
    }
    const size_t lds = ((size_t)r->table_dwords + r->sx) * 4;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(ntiles * batch)), dim3(kResThreads), lds, s, p);
    FV_HIP_CHECK(hipGetLastError());
    set_last_kernel("resample_kernel");
    return FV_OK;
}

// pitch_shift.hip: the outputs [0, m_end) of `batch` rows of `len` samples (fv_resample_forward without its argument checks)
fv_status fv::resample_rows(const fv_resample* r, const char* fn, const float* x, long long x_stride, long long len, float* y, long long y_stride,
                            int batch, long long m_end, hipStream_t s) {
    return resample_run(r, fn, x, x_stride, 0, nullptr, len, y, y_stride, batch, 0, m_end, s);
}

long long fv::resample_emit_count(const fv_resample* r, long long N) { return r->emit_count(N); }
int fv::resample_band_taps(const fv_resample* r) { return r->d.kp; }

extern "C" {

FV_API fv_status fv_resample_design(const fv_resample_config* cfg, int32_t* o, int32_t* n, int32_t* width, int32_t* kp, int32_t* first,
                                    int32_t* count, int32_t phase_cap, float* taps, int64_t taps_cap) {
    if (!o || !n || !width || !kp) {
        set_error("fv_resample_design: null output (o, n, width and kp are always written)");
        return FV_ERR_INVALID;
    }
    Design d;
    if (const fv_status r = design(cfg, "fv_resample_design", d, taps != nullptr)) return r;
    *o = d.o, *n = d.n, *width = d.width, *kp = d.kp;
    if ((first || count) && phase_cap < d.n) {
        set_error("fv_resample_design: first / count hold %d entries, %d -> %d Hz has %d phases", phase_cap, cfg->orig_freq, cfg->new_freq, d.n);
        return FV_ERR_INVALID;
    }
    if (taps && taps_cap < (int64_t)d.n * d.kp) {
        set_error("fv_resample_design: taps holds %lld floats, %d -> %d Hz needs %d x %d", (long long)taps_cap, cfg->orig_freq, cfg->new_freq, d.n,
                  d.kp);
        return FV_ERR_INVALID;
    }
    if (first) std::copy(d.first.begin(), d.first.end(), first);
    if (count) std::copy(d.count.begin(), d.count.end(), count);
    if (taps) std::copy(d.taps.begin(), d.taps.end(), taps);
    return FV_OK;
}

FV_API int32_t fv_resample_input_tile(void) { return kResTile; }

}  // extern "C"

// both create entries: the same design, the same table layout; global_table decides where the kernel reads it and what must fit in LDS
static fv_status resample_create(const fv_resample_config* cfg, fv_resample** out, bool global_table, const char* fn) {
    if (!out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_resample> r(new fv_resample());
    if (const fv_status st = design(cfg, fn, r->d, false)) return st;
    const Design& d0 = r->d;
    const long long kpad = d0.kp | 1;   // odd rows: lanes on consecutive phases read consecutive LDS banks
    const long long table = ((2LL * d0.n + (long long)d0.n * kpad + 3) / 4) * 4, sx = (((long long)kResTile + d0.kp + 3 + 3) / 4) * 4;
    if (global_table) {
        if (sx * 4 > (long long)kResLdsBudget) {
            set_error("%s: %d -> %d Hz has bands of %d taps: the staged input (the %d-sample tile plus one band, %lld bytes) passes the LDS "
                      "budget of %zu", fn, cfg->orig_freq, cfg->new_freq, d0.kp, kResTile, sx * 4, kResLdsBudget);
            return FV_ERR_UNSUPPORTED;
        }
        if (table * 4 > (1LL << 30)) {
            set_error("%s: %d -> %d Hz needs a table of %d phases x %d taps, %lld bytes: more than the limit of 2^30", fn, cfg->orig_freq,
                      cfg->new_freq, d0.n, d0.kp, table * 4);
            return FV_ERR_UNSUPPORTED;
        }
    } else if ((table + sx) * 4 > (long long)kResLdsBudget) {
        set_error("fv_resample_create: %d -> %d Hz needs a table of %d phases x %d taps (%lld bytes with its index rows); beside the %d-sample "
                  "input tile that is %lld bytes of LDS, over the budget of %zu", cfg->orig_freq, cfg->new_freq, d0.n, d0.kp, table * 4, kResTile,
                  (table + sx) * 4, kResLdsBudget);
        return FV_ERR_UNSUPPORTED;
    }
    if (const fv_status st = design(cfg, fn, r->d, true)) return st;
    const Design& d = r->d;
    r->cfg = *cfg;
    r->global_table = global_table;
    r->kpad = (int)kpad, r->table_dwords = (int)table, r->sx = (int)sx;
    r->end.resize(d.n);
    for (int p = 0; p < d.n; ++p) r->end[p] = d.first[p] + d.count[p];
    std::vector<uint32_t> host((size_t)table, 0u);
    for (int p = 0; p < d.n; ++p) {
        host[p] = (uint32_t)d.first[p];
        host[d.n + p] = (uint32_t)d.count[p];
        std::memcpy(&host[2 * (size_t)d.n + (size_t)p * kpad], &d.taps[(size_t)p * d.kp], sizeof(float) * d.kp);
    }
    FV_HIP_CHECK(hipMalloc((void**)&r->d_table, host.size() * 4));
    FV_HIP_CHECK(hipMemcpy(r->d_table, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    *out = r.release();
    return FV_OK;
}

extern "C" {

FV_API fv_status fv_resample_create(const fv_resample_config* cfg, fv_resample** out) {
    return resample_create(cfg, out, false, "fv_resample_create");
}

FV_API fv_status fv_global_resample_create(const fv_resample_config* cfg, fv_resample** out) {
    return resample_create(cfg, out, true, "fv_global_resample_create");
}

FV_API void fv_resample_destroy(fv_resample* r) { delete r; }

FV_API int64_t fv_resample_output_length(const fv_resample* r, int64_t L) {
    if (!r || L < 0 || L > kResMaxLen) return -1;
    return r->out_len(L);
}

FV_API fv_status fv_resample_check_lengths(const fv_resample* r, const int32_t* host_lengths, int32_t batch, int64_t L) {
    if (!r || !host_lengths || batch < 0) {
        set_error("fv_resample_check_lengths: null or negative argument");
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > L) {
            set_error("fv_resample_forward: lengths[%d] = %d lies outside [0, L = %lld]", b, host_lengths[b], (long long)L);
            return FV_ERR_INVALID;
        }
    return FV_OK;
}

FV_API fv_status fv_resample_forward(fv_resample* r, const float* d_x, int64_t x_row_stride, const int32_t* d_lengths, float* d_y,
                                     int64_t y_row_stride, int32_t batch, int64_t L, void* stream) {
    if (!r) {
        set_error("fv_resample_forward: null resampler");
        return FV_ERR_INVALID;
    }
    if (batch < 0 || L < 0 || L > kResMaxLen) {
        set_error("fv_resample_forward: batch = %d and L = %lld must be >= 0 (L <= 2^40)", batch, (long long)L);
        return FV_ERR_INVALID;
    }
    const long long M = r->out_len(L);
    if (batch == 0 || L == 0) return FV_OK;
    if (!d_x || !d_y) {
        set_error("fv_resample_forward: null %s", d_x ? "d_y" : "d_x");
        return FV_ERR_INVALID;
    }
    if (x_row_stride < L || y_row_stride < M) {
        set_error("fv_resample_forward: row strides (%lld, %lld) are shorter than the rows (L = %lld, %lld outputs)", (long long)x_row_stride,
                  (long long)y_row_stride, (long long)L, M);
        return FV_ERR_INVALID;
    }
    const float *x_end = d_x + (int64_t)(batch - 1) * x_row_stride + L, *y_end = d_y + (int64_t)(batch - 1) * y_row_stride + M;
    if (d_x < y_end && d_y < x_end) {
        set_error("fv_resample_forward: d_y overlaps d_x; the resampler does not run in place (workgroups read their neighbours' input)");
        return FV_ERR_INVALID;
    }
    return resample_run(r, "fv_resample_forward", d_x, x_row_stride, 0, d_lengths, L, d_y, y_row_stride, batch, 0, M, (hipStream_t)stream);
}

FV_API fv_status fv_resample_stream_create(fv_resample* r, int32_t batch, int32_t max_chunk, fv_resample_stream** out) {
    if (!r || !out) {
        set_error("fv_resample_stream_create: null argument");
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_resample_stream> st(new fv_resample_stream());
    st->r = r;
    const int H = (r->d.kp + 3) / 4 * 4;   // an output not yet emitted starts less than Kp samples before N
    if (const fv_status rs = st->create("fv_resample_stream_create", batch, max_chunk, H, ((long long)H + max_chunk + 3) / 4 * 4)) return rs;
    *out = st.release();
    return FV_OK;
}

FV_API int64_t fv_resample_stream_pending(const fv_resample_stream* s) { return s ? s->r->out_len(s->N) - s->E : 0; }

static fv_status resample_stream_step(fv_resample_stream* st, const float* d_x, int64_t x_row_stride, int32_t c, bool flush, float* d_y,
                                      int64_t y_row_stride, int64_t* emitted, void* stream) {
    const char* fn = flush ? "fv_resample_stream_flush" : "fv_resample_stream_push";
    if (emitted) *emitted = 0;
    if (!st || !emitted) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    long long N2;
    bool noop;
    if (const fv_status rs = st->admit(fn, "fv_resample_stream_reset", d_x, x_row_stride, c, flush, &N2, &noop)) return rs;
    if (noop) return FV_OK;
    const fv_resample* r = st->r;
    const long long E2 = flush ? r->out_len(N2) : std::max(st->E, r->emit_count(N2));
    const long long k = E2 - st->E;
    if (k > 0 && (!d_y || y_row_stride < k)) {
        set_error("%s: %s (this call emits %lld outputs per row)", fn, d_y ? "y_row_stride is shorter than the output" : "null output", k);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool run = !flush || k > 0;
    if (run) {
        const int nc = flush ? 0 : c;
        float* next = st->buf[st->cur ^ 1];
        if (const fv_status rs = launch_sample_carry(st->buf[st->cur], next, d_x, st->stride, x_row_stride, st->B, st->N, st->N - st->H,
                                                     st->N - st->H - st->prev_c, st->H + nc, s))
            return rs;
        if (const fv_status rs = resample_run(r, fn, next, st->stride, st->N - st->H, nullptr, N2, d_y, y_row_stride, st->B, st->E, E2, s)) return rs;
        st->prev_c = nc;
    }
    *emitted = k;
    st->commit(N2, E2, flush, run);
    return FV_OK;
}

FV_API fv_status fv_resample_stream_push(fv_resample_stream* s, const float* d_x, int64_t x_row_stride, int32_t c, float* d_y,
                                         int64_t y_row_stride, int64_t* emitted, void* stream) {
    return resample_stream_step(s, d_x, x_row_stride, c, false, d_y, y_row_stride, emitted, stream);
}

FV_API fv_status fv_resample_stream_flush(fv_resample_stream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream) {
    return resample_stream_step(s, nullptr, 0, 0, true, d_y, y_row_stride, emitted, stream);
}

FV_API fv_status fv_resample_stream_reset(fv_resample_stream* s) {
    if (!s) {
        set_error("fv_resample_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->reset();
    return FV_OK;
}

FV_API void fv_resample_stream_destroy(fv_resample_stream* s) { delete s; }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// The pool (fv_respool_*): the sample pool's counters and carry (sample_pool.h) around resample_pool_kernel.
// ---------------------------------------------------------------------------------------------
struct fv_respool : SamplePool {
    fv_resample* r = nullptr;
    long long max_out = 0;      // fv_respool_max_outputs
};

// the host half of resample_create: the design's sizes and end[], enough for out_len / emit_count / s_of (fv_respool_plan)
static fv_status resample_rule(const fv_resample_config* cfg, const char* fn, fv_resample& r) {
    if (const fv_status st = design(cfg, fn, r.d, false)) return st;
    r.cfg = *cfg;
    r.end.resize((size_t)r.d.n);
    for (int p = 0; p < r.d.n; ++p) r.end[(size_t)p] = r.d.first[(size_t)p] + r.d.count[(size_t)p];
    return FV_OK;
}

// The emission rule of one step, after the pool's admit: E2[i] = flush ? out_len(N2) : max(E, emit_count(N2)).
static void respool_emission(const fv_resample& r, const int64_t* emitted, const fv_wavpool_item* items, int count, const long long* N2,
                             long long* E2) {
    for (int i = 0; i < count; ++i) {
        const long long E = emitted[items[i].session];
        E2[i] = items[i].flush ? std::max(E, r.out_len(N2[i])) : std::max(E, r.emit_count(N2[i]));
    }
}

// The most one item emits in one step (the derivation: include/fishvoc.h): g(N) = out_len(N + max_chunk) - emit_count(N) just before each of
// the n jumps of emit_count in one period of o samples, past the point from which emit_count is periodic.
static long long respool_max_outputs(const fv_resample& r, int max_chunk) {
    const Design& d = r.d;
    long long best = 0;
    for (int p = 0; p < d.n; ++p) {
        const long long N = 2LL * d.o + r.end[(size_t)p] - d.width - 1;   // frame 2: end[0] >= end[n - 1] - o, so N >= end[n - 1] - width - o
        best = std::max(best, r.out_len(N + max_chunk) - r.emit_count(N));
    }
    return best;
}

fv_status fv::resample_rule_create(const fv_resample_config* cfg, const char* fn, fv_resample** out) {
    std::unique_ptr<fv_resample> r(new fv_resample());
    if (const fv_status st = resample_rule(cfg, fn, *r)) return st;
    *out = r.release();
    return FV_OK;
}
long long fv::resample_pool_max_outputs(const fv_resample* r, int max_chunk) { return respool_max_outputs(*r, max_chunk); }

extern "C" {

FV_API fv_status fv_respool_create(fv_resample* r, int32_t sessions, int32_t max_chunk, fv_respool** out) {
    const char* fn = "fv_respool_create";
    if (out) *out = nullptr;
    if (!r || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_respool> p(new fv_respool());
    p->r = r;
    const int H = (r->d.kp + 3) / 4 * 4;   // an output not yet emitted starts less than Kp samples before N (fv_resample_stream_create)
    if (const fv_status rs = p->create(fn, sessions, max_chunk, H)) return rs;
    p->max_out = respool_max_outputs(*r, max_chunk);
    *out = p.release();
    return FV_OK;
}

FV_API int64_t fv_respool_max_outputs(const fv_respool* p) { return p ? p->max_out : 0; }

FV_API int64_t fv_respool_received(const fv_respool* p, int32_t s) { return sample_pool_received(p, s); }

FV_API int64_t fv_respool_emitted(const fv_respool* p, int32_t s) { return sample_pool_emitted(p, s); }

FV_API int64_t fv_respool_pending(const fv_respool* p, int32_t s) {
    return p && s >= 0 && s < p->S ? p->r->out_len(p->N[(size_t)s]) - p->E[(size_t)s] : 0;
}

FV_API int64_t fv_respool_plan(const fv_resample_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* outputs_out) {
    const char* fn = "fv_respool_plan";
    fv_resample r;
    if (const fv_status st = resample_rule(cfg, fn, r)) return st;
    if (const fv_status st = sample_pool_range(fn, sessions, max_chunk)) return st;
    return sample_pool_plan(fn, sessions, max_chunk, received, emitted, flushed, items, count, outputs_out,
                            [&](const long long* N2, long long* E2) {
                                respool_emission(r, emitted, items, count, N2, E2);
                                return FV_OK;
                            });
}

FV_API fv_status fv_respool_step(fv_respool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int64_t out_stride, int32_t out_cols, int64_t* outputs_out, void* stream) {
    const char* fn = "fv_respool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    for (int i = 0; outputs_out && i < count; ++i) outputs_out[i] = 0;
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status rs = p->admit(fn, "fv_respool_reset", items, count, d_chunks, chunk_stride, N2.data())) return rs;
    const fv_resample* r = p->r;
    respool_emission(*r, p->E.data(), items, count, N2.data(), E2.data());
    if (const fv_status rs = sample_pool_output(fn, "outputs", items, count, p->E.data(), E2.data(), 1, d_out != nullptr, out_stride, out_cols))
        return rs;
    // one table entry per item, in item order: every row of d_out is written (E2 - E <= out_cols: it fits an int); `carry` the items that push samples
    std::vector<SamplePoolEntry> fir, carry;
    p->build_entries(items, count, N2.data(), E2.data(), fir, carry);
    std::vector<int> tiles((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        const SamplePoolEntry& en = fir[(size_t)i];
        const long long E = en.first;
        if (en.count > 0) {
            const long long X0 = r->s_of(E), j0 = X0 - r->d.width;
            if (en.carry_origin > 0 && j0 < en.carry_origin) {   // (cannot happen: an output not yet emitted starts less than Kp <= H samples before N)
                set_error("%s: internal: output %lld of session %d reads sample %lld, before the %d carried samples that end at %lld", fn, E,
                          items[i].session, j0, p->H, en.chunk_origin);
                return FV_ERR_INVALID;
            }
            tiles[(size_t)i] = (int)((r->s_of(E2[(size_t)i] - 1) - X0) / kResTile + 1);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (count > 0 && out_cols > 0 && d_out) {
        ResamplePoolParams q{};
        q.chunk = d_chunks, q.buf0 = p->buf[0], q.buf1 = p->buf[1], q.y = d_out, q.table = r->d_table;
        q.chunk_stride = chunk_stride, q.y_stride = out_stride, q.H = p->H, q.out_cols = out_cols;
        q.o = r->d.o, q.n = r->d.n, q.width = r->d.width, q.kpad = r->kpad, q.table_dwords = r->table_dwords, q.sx = r->sx;
        const fv_status rs = for_each_launch_table<SamplePoolBlock>(count, fir.data(), [&](const SamplePoolBlock& blk, int k0, int nz) {
            q.max_tiles = std::max(1, *std::max_element(tiles.begin() + k0, tiles.begin() + k0 + nz));
            const dim3 grid((unsigned)q.max_tiles, (unsigned)nz);
            if (r->global_table) {
                hipLaunchKernelGGL(resample_pool_global_kernel, grid, dim3(kResThreads), (size_t)r->sx * 4, s, q, blk);
                set_last_kernel("resample_pool_global_kernel");
            } else {
                hipLaunchKernelGGL(resample_pool_kernel, grid, dim3(kResThreads), ((size_t)r->table_dwords + r->sx) * 4, s, q, blk);
                set_last_kernel("resample_pool_kernel");
            }
            return FV_OK;
        });
        if (rs) return rs;
    }
    if (const fv_status rs = launch_sample_pool_carry(p->buf[0], p->buf[1], p->H, d_chunks, chunk_stride, carry.data(), (int)carry.size(), s))
        return rs;
    for (int i = 0; outputs_out && i < count; ++i) outputs_out[i] = E2[(size_t)i] - p->E[(size_t)items[i].session];
    p->commit(items, count, N2.data(), E2.data());
    return FV_OK;
}

FV_API fv_status fv_respool_reset(fv_respool* p, int32_t session) { return sample_pool_reset(p, "fv_respool_reset", session); }

FV_API void fv_respool_destroy(fv_respool* p) { delete p; }

}  // extern "C"
