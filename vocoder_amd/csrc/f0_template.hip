// F0 tracking and pitch templates (fv_f0_*, fv_template_*, include/fishvoc.h): what a user of the template generators (refinegan.py:287,
// hifigan.py:226) brings from a CPU F0 tracker today, on the GPU.
//
//   yin_f0_kernel              one workgroup per (row, frame): the frame staged once in LDS, the direct-form difference function
//                              d(tau) = sum_{j < Wi} (x[j] - x[j + tau])^2 with four consecutive lags per lane, the cumulative-mean normalisation as
//                              a scan over 64-lag chunks, the first dip as an integer min-reduction, the parabola by one lane
//   f0_increment_kernel        f0 (Hz) -> F = rint(f0 / sr * 2^32), the phase increment per sample in turns / 2^32 as uint32; 0 = unvoiced
//   f0_template_sums_kernel    per kTmplChunk samples of a row: the sum of the interpolated increments, wrapping uint32
//   f0_template_kernel         carry = the sums of the chunks before this one; a workgroup scan inside the chunk; sin / sawtooth of the phase
//   osc_stream_sums_kernel,    the same two levels on the frames a stream has staged (fv_osc_stream_*), the carry started from the phase the
//   osc_stream_kernel          call before left on the device
//   yin_pool_kernel            yin_f0_kernel's frame (one body, yin_frame_body) per item of a pool of sessions that advance independently
//                              (fv_yinpool_*): the frame staged from the slot's carry and the item's chunk row
//   osc_pool_increment_kernel, the oscillator's levels per item of such a pool (fv_oscpool_*): increments from the slot's two carried frames and
//   osc_pool_sums_kernel,      the item's F0 row, chunk sums, and the samples with the slot's own carried phase.  One fv_oscpool_step is these
//   osc_pool_kernel            three launches and one carry launch per 32 items, whatever the number of sessions
// The streams (fv_yin_stream_*, fv_osc_stream_*) sit on the sample streams' carry core (sample_stream.h): the tracker carries the last samples of
// every row and runs yin_f0_kernel on [carried | chunk]; the oscillator carries the last two F0 frames, as its "samples", and the phase.
//
// Why the direct form: E(0) + E(tau) - 2 r(tau) cancels in fp32 exactly where d is small, the voiced case.  Every d(tau) is one fp32 accumulator
// over ascending j with fused multiply-adds, and the running sum is scanned in chunks of 64 lags whatever the launch: a frame's bits depend on
// the plan alone.  Why integers for the phase: the same reason as pv_scan_synth_kernel's accumulator (pitch_shift.hip) — the sum never grows
// and is exact in any order.  The sample streams' carry core (sample_stream.h) carries the last H samples of a row from call to call; a prefix
// sum has no such history, so the two-level scan here is its own.  The pools sit on the per-session form of that core (sample_pool.h), with a
// ping-pong bit per slot for the carry and another for the oscillator's phase.
#include <memory>

#include "engine_internal.h"
#include "sample_pool.h"
#include "sample_stream.h"

namespace fv {
namespace {

constexpr int kF0MaxFrame = 4096;       // W: the staged frame, d, its scan and the chunk totals stay under 64 KiB of LDS
constexpr int64_t kF0MaxLen = 1LL << 30;
constexpr int kF0Rows = 32;             // rows per launch: their lengths are a LaunchTable (fv_internal.h)
constexpr int kYinLags = 4;             // consecutive lags per lane: one 16-byte LDS read feeds sixteen subtract-and-FMAs
constexpr int kYinMaxThreads = 512;
constexpr int kTmplItems = 8;           // consecutive samples per thread
constexpr int kTmplChunk = 256 * kTmplItems;

using F0RowBlock = LaunchTable<int, kF0Rows>;

struct YinPlan {
    int sr = 0, W = 0, hop = 0, tau_min = 0, tau_max = 0, Wi = 0;
    float threshold = 0.f;
    __host__ __device__ int lags() const { return tau_max + 1; }   // d(1) ... d(tau_max + 1)
    // lanes of the lag loop: lane u owns the lags [4 u, 4 u + 4) (lag 0 is computed and is exactly 0); a function of the plan alone
    __host__ __device__ int units() const { return (lags() + kYinLags) / kYinLags; }
    int threads() const {
        const int passes = (units() + kYinMaxThreads - 1) / kYinMaxThreads;
        return ((units() + passes - 1) / passes + 63) / 64 * 64;
    }
    __host__ __device__ int d_elems() const { return (lags() + 1 + 63) / 64 * 64; }
    size_t lds_bytes() const { return (size_t)(W + 8 + 2 * d_elems() + d_elems() / 64 + 32) * sizeof(float); }
};

fv_status make_yin_plan(const fv_f0_config* c, const char* fn, YinPlan& p) {
    if (!c) {
        set_error("%s: null config", fn);
        return FV_ERR_INVALID;
    }
    if (c->sample_rate <= 0) {
        set_error("%s: sample_rate = %d must be > 0", fn, c->sample_rate);
        return FV_ERR_INVALID;
    }
    if (c->hop_length < 1) {
        set_error("%s: hop_length = %d must be >= 1", fn, c->hop_length);
        return FV_ERR_INVALID;
    }
    if (c->frame_length < 2 || c->frame_length % 2) {
        set_error("%s: frame_length = %d must be even and >= 2", fn, c->frame_length);
        return FV_ERR_INVALID;
    }
    if (!(c->fmin > 0.0) || !std::isfinite(c->fmin) || !(c->fmax > 0.0) || !std::isfinite(c->fmax)) {
        set_error("%s: fmin = %g and fmax = %g must be positive and finite", fn, c->fmin, c->fmax);
        return FV_ERR_INVALID;
    }
    if (!(c->threshold > 0.0 && c->threshold <= 1.0)) {
        set_error("%s: threshold = %g must lie in (0, 1]", fn, c->threshold);
        return FV_ERR_INVALID;
    }
    const double tmax = std::floor((double)c->sample_rate / c->fmin), tmin = std::floor((double)c->sample_rate / c->fmax);
    if (tmax > (double)(1 << 24)) {
        set_error("%s: fmin = %g gives a longest lag of %g samples; raise fmin", fn, c->fmin, tmax);
        return FV_ERR_INVALID;
    }
    p.sr = c->sample_rate, p.W = c->frame_length, p.hop = c->hop_length, p.threshold = (float)c->threshold;
    p.tau_max = (int)tmax, p.tau_min = std::max(2, (int)tmin);
    p.Wi = p.W - (p.tau_max + 1);
    if (p.tau_min >= p.tau_max) {
        set_error("%s: fmin = %g and fmax = %g at %d Hz give lags [%d, %d]: no lag to search; lower fmin or raise fmax", fn, c->fmin, c->fmax,
                  c->sample_rate, p.tau_min, p.tau_max);
        return FV_ERR_INVALID;
    }
    if (2 * (long long)p.Wi < p.tau_max) {
        set_error("%s: frame_length = %d leaves an integration window of %d samples, less than half the longest lag (%d, from fmin = %g); raise "
                  "frame_length or fmin", fn, p.W, p.Wi, p.tau_max, c->fmin);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

__device__ __forceinline__ float wave_scan_add(float v, int lane) {   // inclusive, Hillis-Steele: the order is the same on every launch
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const float u = __shfl_up(v, sh, 64);
        if (lane >= sh) v += u;
    }
    return v;
}

// One frame, staged by the caller in xs = lds[0 .. W + 8) (the frame, then zeros): the difference function, the cumulative-mean normalisation,
// the threshold search and the parabolic step, by the whole workgroup of pl.threads(); thread 0 stores the frame's values (ap_out may be NULL).
// LDS: xs[W + 8] | dl[d_elems] (d, then d') | cs[d_elems] (the prefix inside a 64-lag chunk) | ct[d_elems / 64] (chunk totals) | red[32].
// The one body of yin_f0_kernel (whole rows, lockstep streams) and yin_pool_kernel (per-session items): a frame's bits depend on the plan alone.
__device__ __forceinline__ void yin_frame_body(float* lds, const YinPlan& pl, float* __restrict__ f0_out, float* __restrict__ ap_out) {
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int W = pl.W, Wi = pl.Wi, NL = pl.lags(), DE = pl.d_elems();
    float* xs = lds;
    float* dl = xs + W + 8;
    float* cs = dl + DE;
    float* ct = cs + DE;
    float* red = ct + DE / 64;
    for (int i = tid; i < DE; i += nthr) dl[i] = 0.f;
    __syncthreads();

    // the lag loop: lane u holds d(4 u + r), r < 4, in four accumulators; x[j .. j + 3] is a broadcast, x[j + 4 u ...] consecutive 16-byte slots.
    // Measured against the plain form (one lag per lane, x[j] and x[j + tau] read per pair) on 32 x 10 s at 44.1 kHz: 1.94 ms against 2.50 ms
    // (profiles/LOG.md R21.1); the plain form was not kept.
    for (int u = tid; u < pl.units(); u += nthr) {
        const int tau0 = kYinLags * u;
        float acc[kYinLags] = {0.f, 0.f, 0.f, 0.f};
        const float* xw = xs + tau0;
        const int main_end = Wi & ~3;
        float4 w0 = *reinterpret_cast<const float4*>(xw);
        for (int j = 0; j < main_end; j += 4) {
            const float4 a = *reinterpret_cast<const float4*>(xs + j);
            const float4 w1 = *reinterpret_cast<const float4*>(xw + j + 4);
            const float av[4] = {a.x, a.y, a.z, a.w};
            const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                for (int r = 0; r < kYinLags; ++r) {
                    const float df = av[jj] - w[jj + r];
                    acc[r] = fmaf(df, df, acc[r]);
                }
            }
            w0 = w1;
        }
        for (int j = main_end; j < Wi; ++j) {
            const float a = xs[j];
#pragma unroll
            for (int r = 0; r < kYinLags; ++r) {
                const float df = a - xw[j + r];
                acc[r] = fmaf(df, df, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kYinLags; ++r)
            if (tau0 + r <= NL) dl[tau0 + r] = acc[r];
    }
    __syncthreads();

    // running sum: chunk c = lags [64 c, 64 c + 64) scanned by one wave; the chunks' totals are then added in chunk order
    const int nchunk = DE / 64;
    for (int c = wave; c < nchunk; c += nwave) {
        const float s = wave_scan_add(dl[64 * c + lane], lane);
        cs[64 * c + lane] = s;
        if (lane == 63) ct[c] = s;
    }
    __syncthreads();
    for (int tau = 1 + tid; tau <= NL; tau += nthr) {
        float off = 0.f;
        for (int c = 0; c < tau / 64; ++c) off += ct[c];
        const float run = off + cs[tau];
        const float d = dl[tau];
        dl[tau] = run == 0.f ? 1.f : d * (float)tau / run;   // (each lag is read and written by this thread alone)
    }
    __syncthreads();

    // the smallest qualifying lag, and the smallest d' for an unvoiced frame
    int best = 0x7fffffff;
    float mn = 3.0e38f;
    for (int tau = pl.tau_min + tid; tau <= pl.tau_max; tau += nthr) {
        const float v = dl[tau];
        if (v < pl.threshold && v <= dl[tau - 1] && v < dl[tau + 1]) best = min(best, tau);
        mn = fminf(mn, v);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        best = min(best, __shfl_xor(best, sh, 64));
        mn = fminf(mn, __shfl_xor(mn, sh, 64));
    }
    if (lane == 0) red[wave] = __int_as_float(best), red[16 + wave] = mn;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nwave; ++w) {
            best = min(best, __float_as_int(red[w]));
            mn = fminf(mn, red[16 + w]);
        }
        float f = 0.f, aper = mn;
        if (best != 0x7fffffff) {
            const float a = dl[best - 1], bb = dl[best], c = dl[best + 1];
            const float den = a - 2.f * bb + c;
            const float delta = den > 0.f ? 0.5f * (a - c) / den : 0.f;
            f = (float)pl.sr / ((float)best + delta);
            aper = bb;
        }
        *f0_out = f;
        if (ap_out) *ap_out = aper;
    }
}

// grid (frames, rows); block pl.threads().  LDS as yin_frame_body lays it out.  Workgroup x computes frame t0 + x into column x.  x[b] holds the
// samples [origin, origin + rows.e[row]) of row b (the whole row: origin 0, t0 0, len the row's length; a stream: its carried samples and the
// chunk), the frame's global indices map to index - origin.  Samples before 0 or at or past limit = origin + len are zeros by index: the
// address is clamped and the value selected, so no sample outside [origin, limit) is loaded.
__global__ __launch_bounds__(kYinMaxThreads) void yin_f0_kernel(const float* __restrict__ x, long long x_stride, F0RowBlock rows, int row0,
                                                                float* __restrict__ f0, float* __restrict__ ap, long long out_stride,
                                                                long long origin, long long t0, YinPlan pl) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int col = blockIdx.x, b = row0 + blockIdx.y;
    const long long t = t0 + col, limit = origin + rows.e[blockIdx.y], first = origin > 0 ? origin : 0;
    float* f0r = f0 + (long long)b * out_stride;
    float* apr = ap + (long long)b * out_stride;
    if (t >= limit / pl.hop) {   // (the whole workgroup leaves: no barrier below is reached by a part of it)
        if (tid == 0) f0r[col] = 0.f, apr[col] = 0.f;
        return;
    }
    const int W = pl.W;
    float* xs = lds;
    const float* xr = x + (long long)b * x_stride;
    const long long lo = t * pl.hop + pl.hop / 2 - W / 2;
    for (int i = tid; i < W + 8; i += nthr) {
        const long long idx = lo + i;
        const bool in = i < W && idx >= first && idx < limit;
        const long long at = idx < first ? first : (idx >= limit ? limit - 1 : idx);
        const float v = xr[at - origin];
        xs[i] = in ? v : 0.f;
    }
    yin_frame_body(lds, pl, f0r + col, apr + col);
}

// The pool form (fv_yinpool_step): grid (out_cols, entries); block pl.threads(); at most kSamplePoolBlock entries per launch, by value
// (fv_internal.h: first = E, count = E' - E, carry_origin = N - H, chunk_origin = N, avail = N').  Workgroup (x, k) computes frame first + x of
// entry k into column x of row `item` and stages it from two places, as resample_pool_body's sample() maps them: sample j in
// [chunk_origin, avail) from the item's chunk row, j in [max(0, carry_origin), chunk_origin) from the slot's carry buf[bit][slot], anything
// else — j < 0, and j >= avail, which only a flushing item's frames ask for — is 0.0f and never loaded.  A column at or past the entry's count
// is an exact zero; ap == NULL: the aperiodicity is not stored.
__global__ __launch_bounds__(kYinMaxThreads) void yin_pool_kernel(const float* __restrict__ chunk, long long chunk_stride,
                                                                  const float* __restrict__ buf0, const float* __restrict__ buf1, long long H,
                                                                  const SamplePoolBlock tab, float* __restrict__ f0, float* __restrict__ ap,
                                                                  long long out_stride, YinPlan pl) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int col = blockIdx.x;
    const SamplePoolEntry e = tab.e[blockIdx.y];
    float* f0r = f0 + (long long)e.item * out_stride;
    float* apr = ap ? ap + (long long)e.item * out_stride : nullptr;
    if (col >= e.count) {   // (the whole workgroup leaves: no barrier below is reached by a part of it)
        if (tid == 0) {
            f0r[col] = 0.f;
            if (apr) apr[col] = 0.f;
        }
        return;
    }
    const int W = pl.W;
    float* xs = lds;
    const float* cr = e.avail > e.chunk_origin ? chunk + (long long)e.item * chunk_stride : nullptr;
    const float* carry = (e.bit ? buf1 : buf0) + (long long)e.slot * H;
    const long long held = e.carry_origin > 0 ? e.carry_origin : 0;   // samples [held, chunk_origin) are carried
    const long long lo = (e.first + col) * pl.hop + pl.hop / 2 - W / 2;
    for (int i = tid; i < W + 8; i += nthr) {
        const long long idx = lo + i;
        float v = 0.f;
        if (i < W && idx >= held && idx < e.avail) v = idx >= e.chunk_origin ? cr[idx - e.chunk_origin] : carry[idx - e.carry_origin];
        xs[i] = v;
    }
    yin_frame_body(lds, pl, f0r + col, apr ? apr + col : nullptr);
}

// F[b][t] = rint(f0 / sr * 2^32) in double for 0 < f0 < sr and t < frames[b], else 0 (unvoiced; NaN and padded frames included)
__global__ __launch_bounds__(256) void f0_increment_kernel(const float* __restrict__ f0, long long f0_stride, F0RowBlock rows, int row0,
                                                           uint32_t* __restrict__ F, int T, int sr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = row0 + blockIdx.y;
    uint32_t v = 0u;
    if (t < rows.e[blockIdx.y]) {
        const float f = f0[(long long)b * f0_stride + t];
        if (f > 0.f && f < (float)sr) v = (uint32_t)__double2ll_rn((double)f / (double)sr * 4294967296.0);
    }
    F[(long long)b * T + t] = v;
}

// The increment of sample n of a row whose staged frames are Fr[lo_c ... hi_c]: between the frame centres a = floor((n - hop / 2) / hop) and
// a + 1, both clamped to [lo_c, hi_c], k samples past centre a; an unvoiced neighbour (F = 0) takes the other one's value.  The whole row:
// lo_c = 0, hi_c = Ti - 1.  A stream counts n and a from the first staged frame, which is frame `o` of the row: lo_c = max(0, -o) and
// hi_c = (frames received) - 1 - o, and n - hop / 2 >= 0 for every sample it emits.
__device__ __forceinline__ uint32_t tmpl_inc(const uint32_t* __restrict__ Fr, int lo_c, int hi_c, int hop, int n) {
    const int m = n - hop / 2;
    const int a = m >= 0 ? m / hop : -1;
    const int k = m - a * hop;
    uint32_t Fa = Fr[min(max(a, lo_c), hi_c)], Fb = Fr[min(max(a + 1, lo_c), hi_c)];
    if (Fa == 0u) Fa = Fb;
    else if (Fb == 0u) Fb = Fa;
    return (uint32_t)(((unsigned long long)Fa * (unsigned)(hop - k) + (unsigned long long)Fb * (unsigned)k) / (unsigned)hop);
}

// One workgroup of 256: the sum of the increments of the samples [n0, n0 + kTmplItems) of every thread that lie before n_end, wrapping; the
// total is returned to thread 0
__device__ __forceinline__ uint32_t tmpl_chunk_sum(const uint32_t* __restrict__ Fr, int lo_c, int hi_c, int hop, int n0, int n_end) {
    __shared__ uint32_t part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i)
        if (n0 + i < n_end) s += tmpl_inc(Fr, lo_c, hi_c, hop, n0 + i);
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// One workgroup of 256: phi[n] = (the phase before the chunk: the threads' `carry` summed) + (the threads before, a workgroup scan) + (this
// thread's own samples); sample n < n_out goes to orow[n - out0], a zero from n_inc on and in an unvoiced frame Fr[n / hop].  phase_after
// (NULL: not wanted): the last thread stores the phase after the chunk's last sample, an ordinary store.
__device__ __forceinline__ void tmpl_chunk_emit(const uint32_t* __restrict__ Fr, int lo_c, int hi_c, int hop, int n0, int n_inc, int n_out,
                                                uint32_t carry, float* __restrict__ orow, int out0, int kind, float amplitude,
                                                uint32_t* __restrict__ phase_after) {
    __shared__ uint32_t part[4], wtot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) carry += __shfl_xor(carry, sh, 64);
    if (lane == 0) part[wave] = carry;
    uint32_t ph[kTmplItems];
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i) {
        if (n0 + i < n_inc) s += tmpl_inc(Fr, lo_c, hi_c, hop, n0 + i);
        ph[i] = s;
    }
    uint32_t inc = s;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const uint32_t v = __shfl_up(inc, sh, 64);
        if (lane >= sh) inc += v;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t base = part[0] + part[1] + part[2] + part[3] + (inc - s);
    for (int w = 0; w < wave; ++w) base += wtot[w];
    if (phase_after && threadIdx.x == 255) *phase_after = base + ph[kTmplItems - 1];
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i) {
        const int n = n0 + i;
        if (n >= n_out) break;
        float v = 0.f;
        if (n < n_inc && Fr[n / hop] != 0u) {
            const uint32_t phi = base + ph[i];
            if (kind == FV_TEMPLATE_SAWTOOTH)
                v = amplitude * ((float)(int32_t)(phi ^ 0x80000000u) * (1.0f / 2147483648.0f));   // 2 phi / 2^32 - 1
            else
                v = amplitude * sinpif((float)(int32_t)phi * (1.0f / 2147483648.0f));   // phi as signed turns: 2 pi phi / 2^32 = pi x
        }
        orow[n - out0] = v;
    }
}

// grid (chunks, rows): sums[b][chunk] = the sum of the chunk's increments, wrapping
__global__ __launch_bounds__(256) void f0_template_sums_kernel(const uint32_t* __restrict__ F, F0RowBlock rows, int row0,
                                                               uint32_t* __restrict__ sums, int T, int hop, int nchunk) {
    const int b = row0 + blockIdx.y, Ti = rows.e[blockIdx.y];
    const uint32_t s = tmpl_chunk_sum(F + (long long)b * T, 0, Ti - 1, hop, blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems, Ti * hop);
    if (threadIdx.x == 0) sums[(long long)b * nchunk + blockIdx.x] = s;
}

// grid (chunks, rows): the carry is the sums of the chunks before this one
__global__ __launch_bounds__(256) void f0_template_kernel(const uint32_t* __restrict__ F, const uint32_t* __restrict__ sums, F0RowBlock rows,
                                                          int row0, float* __restrict__ out, long long out_stride, int T, int hop, int nchunk,
                                                          int kind, float amplitude) {
    const int b = row0 + blockIdx.y, Ti = rows.e[blockIdx.y];
    uint32_t carry = 0u;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) carry += sums[(long long)b * nchunk + c];
    tmpl_chunk_emit(F + (long long)b * T, 0, Ti - 1, hop, blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems, Ti * hop, T * hop, carry,
                    out + (long long)b * out_stride, 0, kind, amplitude, nullptr);
}

// The oscillator stream's two levels, grid (chunks, rows), every row in lockstep.  F[b] holds the increments of `fcount` staged frames, the first
// of them frame `o` of the row; a call emits the samples [n_lo, n_hi) counted from frame o's first sample into the columns [0, n_hi - n_lo).
__global__ __launch_bounds__(256) void osc_stream_sums_kernel(const uint32_t* __restrict__ F, int fcount, uint32_t* __restrict__ sums, int nchunk,
                                                              int lo_c, int hi_c, int hop, int n_lo, int n_hi) {
    const int b = blockIdx.y;
    const uint32_t s = tmpl_chunk_sum(F + (long long)b * fcount, lo_c, hi_c, hop, n_lo + blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems, n_hi);
    if (threadIdx.x == 0) sums[(long long)b * nchunk + blockIdx.x] = s;
}

// the chunk carry starts from phase_in[b], the phase at the start of the first emitted frame (NULL: 0, the utterance's first frame, by index);
// the last chunk's last thread stores the phase after the last emitted sample in phase_out[b], another buffer than phase_in
__global__ __launch_bounds__(256) void osc_stream_kernel(const uint32_t* __restrict__ F, int fcount, const uint32_t* __restrict__ sums, int nchunk,
                                                         const uint32_t* __restrict__ phase_in, uint32_t* __restrict__ phase_out,
                                                         float* __restrict__ out, long long out_stride, int lo_c, int hi_c, int hop, int n_lo,
                                                         int n_hi, int kind, float amplitude) {
    const int b = blockIdx.y;
    uint32_t carry = threadIdx.x == 0 && phase_in ? phase_in[b] : 0u;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) carry += sums[(long long)b * nchunk + c];
    tmpl_chunk_emit(F + (long long)b * fcount, lo_c, hi_c, hop, n_lo + blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems, n_hi, n_hi, carry,
                    out + (long long)b * out_stride, n_lo, kind, amplitude, (int)blockIdx.x == nchunk - 1 ? phase_out + b : nullptr);
}

// The oscillator pool's three levels (fv_oscpool_step), each grid (., entries) with at most kOscPoolBlock entries per launch, by value.  Entry k
// is one item: its slot has received Tn frames, the item brings `fcount - 2` more, and row `item` of F holds the increments of the frames
// [Tn - 2, Tn + c) — the first two from the slot's carry buf[bit][slot], the rest from the item's chunk row — so column 0 is frame o = Tn - 2 of
// the utterance and everything below counts from there, as in the stream: clamp bounds lo_c / hi_c, the emitted samples [n_lo, n_hi) in
// `nchunk` chunks of kTmplChunk.  phase_in: the array (0 / 1) that holds the phase at the start of frame E, -1: E = 0, phase 0 by index; the
// phase after the last emitted sample goes into the array phase_out, the other one.
struct OscPoolEntry {
    int item, slot, bit;
    int phase_in, phase_out;
    int fcount, lo_c, hi_c;
    int n_lo, n_hi, nchunk;
};
constexpr int kOscPoolBlock = 32;
using OscPoolBlock = LaunchTable<OscPoolEntry, kOscPoolBlock>;

// grid (ceil(f_cols / 256), entries), f_cols the block's largest fcount: F[item][t] = the increment of frame o + t, f0_increment_kernel's
// conversion; 0 before the utterance's first frame (t < lo_c: the carry may hold an earlier utterance) and from fcount on
__global__ __launch_bounds__(256) void osc_pool_increment_kernel(const float* __restrict__ chunk, long long chunk_stride,
                                                                 const float* __restrict__ buf0, const float* __restrict__ buf1,
                                                                 const OscPoolBlock tab, uint32_t* __restrict__ F, int f_stride, int f_cols,
                                                                 int sr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= f_cols) return;
    const OscPoolEntry e = tab.e[blockIdx.y];
    uint32_t v = 0u;
    if (t >= e.lo_c && t < e.fcount) {
        const float f = t < 2 ? ((e.bit ? buf1 : buf0) + 2LL * e.slot)[t] : chunk[(long long)e.item * chunk_stride + (t - 2)];
        if (f > 0.f && f < (float)sr) v = (uint32_t)__double2ll_rn((double)f / (double)sr * 4294967296.0);
    }
    F[(long long)e.item * f_stride + t] = v;
}

// grid (the block's largest nchunk, entries): sums[item][chunk], wrapping; a workgroup past its entry's chunks leaves whole
__global__ __launch_bounds__(256) void osc_pool_sums_kernel(const uint32_t* __restrict__ F, int f_stride, uint32_t* __restrict__ sums,
                                                            int sums_stride, const OscPoolBlock tab, int hop) {
    const OscPoolEntry e = tab.e[blockIdx.y];
    if ((int)blockIdx.x >= e.nchunk) return;
    const uint32_t s = tmpl_chunk_sum(F + (long long)e.item * f_stride, e.lo_c, e.hi_c, hop,
                                      e.n_lo + blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems, e.n_hi);
    if (threadIdx.x == 0) sums[(long long)e.item * sums_stride + blockIdx.x] = s;
}

// grid (ceil(out_cols / kTmplChunk), entries): the samples [n_lo, n_hi) of the entry into the columns [0, n_hi - n_lo) of row `item`, exact
// zeros up to out_cols.  A workgroup past its entry's chunks stores its zeros and leaves whole, before any barrier.
__global__ __launch_bounds__(256) void osc_pool_kernel(const uint32_t* __restrict__ F, int f_stride, const uint32_t* __restrict__ sums,
                                                       int sums_stride, const OscPoolBlock tab, uint32_t* phase0, uint32_t* phase1,
                                                       float* __restrict__ out, long long out_stride, int out_cols, int hop, int kind,
                                                       float amplitude) {
    const OscPoolEntry e = tab.e[blockIdx.y];
    float* orow = out + (long long)e.item * out_stride;
    if ((int)blockIdx.x >= e.nchunk) {
        const long long c0 = (long long)blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems;   // this thread's first column
#pragma unroll
        for (int i = 0; i < kTmplItems; ++i)
            if (c0 + i < out_cols) orow[c0 + i] = 0.f;
        return;
    }
    const int c0 = blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems;   // (inside the entry's chunks: below 2^30)
    const uint32_t* pin = e.phase_in < 0 ? nullptr : (e.phase_in ? phase1 : phase0);
    uint32_t* pout = e.phase_out ? phase1 : phase0;
    const uint32_t* srow = sums + (long long)e.item * sums_stride;
    uint32_t carry = threadIdx.x == 0 && pin ? pin[e.slot] : 0u;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) carry += srow[c];
    const int n_out = e.n_lo + (int)min((long long)out_cols, ((long long)blockIdx.x + 1) * kTmplChunk);
    tmpl_chunk_emit(F + (long long)e.item * f_stride, e.lo_c, e.hi_c, hop, e.n_lo + c0, e.n_hi, n_out, carry, orow, e.n_lo, kind, amplitude,
                    (int)blockIdx.x == e.nchunk - 1 ? pout + e.slot : nullptr);
}

// the rows' lengths, checked before anything is enqueued; host == NULL: every row has `whole`
fv_status check_rows(const char* fn, const char* what, const int32_t* host, int batch, int whole) {
    for (int b = 0; host && b < batch; ++b)
        if (host[b] < 0 || host[b] > whole) {
            set_error("%s: row %d has %s = %d, outside [0, %d]", fn, b, what, host[b], whole);
            return FV_ERR_INVALID;
        }
    return FV_OK;
}

}  // namespace
}  // namespace fv

struct fv_f0 {
    fv_f0_config cfg{};
    YinPlan plan;
};

struct fv_template {
    fv_template_config cfg{};
};

static fv_status check_template_config(const fv_template_config* c, const char* fn) {
    if (!c) {
        set_error("%s: null config", fn);
        return FV_ERR_INVALID;
    }
    if (c->sample_rate <= 0 || c->hop_length < 1 || c->hop_length > (1 << 20)) {
        set_error("%s: sample_rate = %d must be > 0 and hop_length = %d in [1, 2^20]", fn, c->sample_rate, c->hop_length);
        return FV_ERR_INVALID;
    }
    if (c->kind != FV_TEMPLATE_SINE && c->kind != FV_TEMPLATE_SAWTOOTH) {
        set_error("%s: kind = %d is neither FV_TEMPLATE_SINE nor FV_TEMPLATE_SAWTOOTH", fn, c->kind);
        return FV_ERR_INVALID;
    }
    if (!std::isfinite(c->amplitude)) {
        set_error("%s: amplitude = %g must be finite", fn, (double)c->amplitude);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// [F (B, T) uint32 | sums (B, chunks) uint32], each part rounded up to 64 words
static size_t template_words(int B, int64_t T, int hop, size_t* f_words) {
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    const size_t nchunk = (size_t)((T * hop + kTmplChunk - 1) / kTmplChunk);
    const size_t nf = up((size_t)B * (size_t)T);
    if (f_words) *f_words = nf;
    return nf + up((size_t)B * nchunk);
}

extern "C" {

FV_API fv_status fv_f0_plan(const fv_f0_config* cfg, int64_t L, int32_t* tau_min, int32_t* tau_max, int32_t* window, int64_t* frames) {
    YinPlan p;
    if (const fv_status st = make_yin_plan(cfg, "fv_f0_plan", p)) return st;
    if (L < 0 || L > kF0MaxLen) {
        set_error("fv_f0_plan: L = %lld must lie in [0, 2^30]", (long long)L);
        return FV_ERR_INVALID;
    }
    if (tau_min) *tau_min = p.tau_min;
    if (tau_max) *tau_max = p.tau_max;
    if (window) *window = p.Wi;
    if (frames) *frames = L / p.hop;
    return FV_OK;
}

FV_API fv_status fv_f0_create(const fv_f0_config* cfg, fv_f0** out) {
    const char* fn = "fv_f0_create";
    if (!out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_f0> p(new fv_f0());
    if (const fv_status st = make_yin_plan(cfg, fn, p->plan)) return st;
    if (p->plan.W > kF0MaxFrame) {
        set_error("%s: frame_length = %d is above %d, what one workgroup stages in LDS", fn, p->plan.W, kF0MaxFrame);
        return FV_ERR_UNSUPPORTED;
    }
    p->cfg = *cfg;
    *out = p.release();
    return FV_OK;
}

FV_API void fv_f0_destroy(fv_f0* p) { delete p; }

FV_API size_t fv_f0_workspace_bytes(const fv_f0* p, int32_t batch, int64_t L) {
    (void)p, (void)batch, (void)L;
    return 0;   // every frame lives in its workgroup's LDS
}

FV_API fv_status fv_f0_forward(fv_f0* p, const float* d_x, int64_t x_row_stride, const int32_t* host_lengths, float* d_f0,
                               float* d_aperiodicity, int64_t out_row_stride, int32_t batch, int64_t L, void* d_workspace,
                               size_t workspace_bytes, void* stream) {
    const char* fn = "fv_f0_forward";
    (void)d_workspace, (void)workspace_bytes;
    if (!p) {
        set_error("%s: null tracker", fn);
        return FV_ERR_INVALID;
    }
    if (batch < 0 || batch > 65535 || L < 0 || L > kF0MaxLen) {
        set_error("%s: batch = %d must lie in [0, 65535] and L = %lld in [0, 2^30]", fn, batch, (long long)L);
        return FV_ERR_INVALID;
    }
    const YinPlan& pl = p->plan;
    const int64_t T = L / pl.hop;
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_x || !d_f0 || !d_aperiodicity) {
        set_error("%s: null %s", fn, !d_x ? "d_x" : (!d_f0 ? "d_f0" : "d_aperiodicity"));
        return FV_ERR_INVALID;
    }
    if (x_row_stride < L || out_row_stride < T) {
        set_error("%s: row strides (%lld, %lld) are shorter than the rows (L = %lld, %lld frames)", fn, (long long)x_row_stride,
                  (long long)out_row_stride, (long long)L, (long long)T);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = check_rows(fn, "length", host_lengths, batch, (int)L)) return st;
    hipStream_t s = (hipStream_t)stream;
    const fv_status st = for_each_launch_table<F0RowBlock>(batch, [&](int b) { return host_lengths ? host_lengths[b] : (int)L; },
                                                           [&](const F0RowBlock& rows, int row0, int count) {
        hipLaunchKernelGGL(yin_f0_kernel, dim3((unsigned)T, count), dim3(pl.threads()), pl.lds_bytes(), s, d_x, (long long)x_row_stride, rows,
                           row0, d_f0, d_aperiodicity, (long long)out_row_stride, 0LL, 0LL, pl);
        return FV_OK;
    });
    if (st == FV_OK) set_last_kernel("yin_f0_kernel");
    return st;
}

FV_API fv_status fv_template_create(const fv_template_config* cfg, fv_template** out) {
    const char* fn = "fv_template_create";
    if (!out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (const fv_status st = check_template_config(cfg, fn)) return st;
    *out = new fv_template{*cfg};
    return FV_OK;
}

FV_API void fv_template_destroy(fv_template* p) { delete p; }

FV_API size_t fv_template_workspace_bytes(const fv_template* p, int32_t batch, int64_t T) {
    if (!p || batch < 1 || T < 1 || T * p->cfg.hop_length > kF0MaxLen) return 0;
    return align_up(template_words(batch, T, p->cfg.hop_length, nullptr) * sizeof(uint32_t), 256);
}

FV_API fv_status fv_template_forward(fv_template* p, const float* d_f0, int64_t f0_row_stride, const int32_t* host_frames, float* d_out,
                                     int64_t out_row_stride, int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* fn = "fv_template_forward";
    if (!p) {
        set_error("%s: null synthesiser", fn);
        return FV_ERR_INVALID;
    }
    const int hop = p->cfg.hop_length;
    if (batch < 0 || batch > 65535 || T < 0 || T * hop > kF0MaxLen) {
        set_error("%s: batch = %d must lie in [0, 65535] and T = %lld frames of %d samples in [0, 2^30] samples", fn, batch, (long long)T, hop);
        return FV_ERR_INVALID;
    }
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_f0 || !d_out) {
        set_error("%s: null %s", fn, d_f0 ? "d_out" : "d_f0");
        return FV_ERR_INVALID;
    }
    if (f0_row_stride < T || out_row_stride < T * hop) {
        set_error("%s: row strides (%lld, %lld) are shorter than the rows (%lld frames, %lld samples)", fn, (long long)f0_row_stride,
                  (long long)out_row_stride, (long long)T, (long long)(T * hop));
        return FV_ERR_INVALID;
    }
    const size_t need = fv_template_workspace_bytes(p, batch, T);
    if (!d_workspace || workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_template_workspace_bytes)", fn, d_workspace ? workspace_bytes : (size_t)0, need);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = check_rows(fn, "frames", host_frames, batch, (int)T)) return st;
    size_t f_words = 0;
    (void)template_words(batch, T, hop, &f_words);
    uint32_t* F = (uint32_t*)d_workspace;
    uint32_t* sums = F + f_words;
    const int nchunk = (int)((T * hop + kTmplChunk - 1) / kTmplChunk);
    hipStream_t s = (hipStream_t)stream;
    const fv_status st = for_each_launch_table<F0RowBlock>(batch, [&](int b) { return host_frames ? host_frames[b] : (int)T; },
                                                           [&](const F0RowBlock& rows, int row0, int count) -> fv_status {
        hipLaunchKernelGGL(f0_increment_kernel, dim3((unsigned)((T + 255) / 256), count), dim3(256), 0, s, d_f0, (long long)f0_row_stride, rows,
                           row0, F, (int)T, p->cfg.sample_rate);
        FV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(f0_template_sums_kernel, dim3(nchunk, count), dim3(256), 0, s, F, rows, row0, sums, (int)T, hop, nchunk);
        FV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(f0_template_kernel, dim3(nchunk, count), dim3(256), 0, s, F, sums, rows, row0, d_out, (long long)out_row_stride,
                           (int)T, hop, nchunk, p->cfg.kind, p->cfg.amplitude);
        return FV_OK;
    });
    if (st == FV_OK) set_last_kernel("f0_template_kernel");
    return st;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Streams.  buf[cur] holds the samples (tracker) or F0 frames (oscillator) [N - H - prev_c, N) of every row; a push writes [N - H, N + c) into
// buf[cur ^ 1] and runs on it, the flush runs on buf[cur] as it stands.
// ---------------------------------------------------------------------------------------------
struct fv_yin_stream : SampleStream {
    fv_f0* p = nullptr;
    int prev_c = 0;
};

struct fv_osc_stream : SampleStream {
    fv_template* p = nullptr;
    int prev_c = 0, pcur = 0;
    uint32_t* aux = nullptr;   // one allocation: F (B, 2 + max_chunk) | sums (B, chunks) | phase[2] (B)
    uint32_t *F = nullptr, *sums = nullptr, *phase[2] = {nullptr, nullptr};
    ~fv_osc_stream() {
        if (aux) (void)hipFree(aux);
    }
};

static long long yin_ready(const YinPlan& pl, long long N) {
    const long long need = pl.hop / 2 + pl.W / 2;
    return N < need ? 0 : std::min(1 + (N - need) / pl.hop, N / pl.hop);
}

static long long yin_pending(const YinPlan& pl, long long N, long long E) {
    return std::max(0LL, N - std::max(0LL, E * pl.hop + pl.hop / 2 - pl.W / 2));
}

static fv_status yin_stream_step(fv_yin_stream* st, const float* d_wave, int64_t row_stride, int32_t c, bool flush, float* d_f0, float* d_ap,
                                 int64_t out_row_stride, int64_t* frames_out, void* stream) {
    const char* fn = flush ? "fv_yin_stream_flush" : "fv_yin_stream_push";
    if (frames_out) *frames_out = 0;
    if (!st || !frames_out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    long long N2;
    bool noop;
    if (const fv_status rs = st->admit(fn, "fv_yin_stream_reset", d_wave, row_stride, c, flush, &N2, &noop)) return rs;
    if (noop) return FV_OK;
    const YinPlan& pl = st->p->plan;
    const long long E2 = flush ? N2 / pl.hop : std::max(st->E, yin_ready(pl, N2));
    const long long k = E2 - st->E;
    if (k > 0 && (!d_f0 || !d_ap || out_row_stride < k)) {
        set_error("%s: %s (this call emits %lld frames per row)", fn,
                  !d_f0 ? "null d_f0" : (!d_ap ? "null d_aperiodicity" : "out_row_stride is shorter than the output"), k);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const float* x = st->buf[st->cur];
    long long origin = st->N - st->H - st->prev_c;
    if (!flush) {
        float* next = st->buf[st->cur ^ 1];
        if (const fv_status rs = launch_sample_carry(st->buf[st->cur], next, d_wave, st->stride, row_stride, st->B, st->N, st->N - st->H, origin,
                                                     (long long)st->H + c, s))
            return rs;
        x = next, origin = st->N - st->H;
        st->prev_c = c;
    }
    if (k > 0) {
        const fv_status rs = for_each_launch_table<F0RowBlock>(st->B, [&](int) { return (int)(N2 - origin); },
                                                               [&](const F0RowBlock& rows, int row0, int count) {
            hipLaunchKernelGGL(yin_f0_kernel, dim3((unsigned)k, count), dim3(pl.threads()), pl.lds_bytes(), s, x, st->stride, rows, row0, d_f0,
                               d_ap, (long long)out_row_stride, origin, st->E, pl);
            return FV_OK;
        });
        if (rs) return rs;
        set_last_kernel("yin_f0_kernel");
    }
    *frames_out = k;
    st->commit(N2, E2, flush, !flush);
    return FV_OK;
}

static fv_status osc_stream_step(fv_osc_stream* st, const float* d_f0, int64_t row_stride, int32_t c, bool flush, float* d_out,
                                 int64_t out_row_stride, int64_t* samples_out, void* stream) {
    const char* fn = flush ? "fv_osc_stream_flush" : "fv_osc_stream_push";
    if (samples_out) *samples_out = 0;
    if (!st || !samples_out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    long long T2;
    bool noop;
    if (const fv_status rs = st->admit(fn, "fv_osc_stream_reset", d_f0, row_stride, c, flush, &T2, &noop)) return rs;
    if (noop) return FV_OK;
    const fv_template_config& cfg = st->p->cfg;
    const int hop = cfg.hop_length;
    const long long E2 = flush ? T2 : std::max(st->E, T2 - 1);
    const long long k = E2 - st->E;
    if (k > 0 && (!d_out || out_row_stride < k * hop)) {
        set_error("%s: %s (this call emits %lld samples per row)", fn, d_out ? "out_row_stride is shorter than the output" : "null output", k * hop);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const float* x = st->buf[st->cur];
    long long o = st->N - st->H - st->prev_c;   // the row's frame that column 0 of x holds
    int fcount = st->H + st->prev_c;
    if (!flush) {
        float* next = st->buf[st->cur ^ 1];
        if (const fv_status rs = launch_sample_carry(st->buf[st->cur], next, d_f0, st->stride, row_stride, st->B, st->N, st->N - st->H, o,
                                                     (long long)st->H + c, s))
            return rs;
        x = next, o = st->N - st->H, fcount = st->H + c;
        st->prev_c = c;
    }
    if (k > 0) {
        const fv_status rs = for_each_launch_table<F0RowBlock>(st->B, [&](int) { return fcount; },
                                                               [&](const F0RowBlock& rows, int row0, int count) {
            hipLaunchKernelGGL(f0_increment_kernel, dim3((unsigned)((fcount + 255) / 256), count), dim3(256), 0, s, x, st->stride, rows, row0,
                               st->F, fcount, cfg.sample_rate);
            return FV_OK;
        });
        if (rs) return rs;
        const int n_lo = (int)((st->E - o) * hop), n_hi = (int)((E2 - o) * hop);
        const int nchunk = (n_hi - n_lo + kTmplChunk - 1) / kTmplChunk;
        const int lo_c = o < 0 ? (int)-o : 0, hi_c = (int)(T2 - 1 - o);
        hipLaunchKernelGGL(osc_stream_sums_kernel, dim3(nchunk, st->B), dim3(256), 0, s, st->F, fcount, st->sums, nchunk, lo_c, hi_c, hop, n_lo, n_hi);
        FV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(osc_stream_kernel, dim3(nchunk, st->B), dim3(256), 0, s, st->F, fcount, st->sums, nchunk,
                           st->E > 0 ? st->phase[st->pcur] : nullptr, st->phase[st->pcur ^ 1], d_out, (long long)out_row_stride, lo_c, hi_c, hop, n_lo,
                           n_hi, cfg.kind, cfg.amplitude);
        FV_HIP_CHECK(hipGetLastError());
        st->pcur ^= 1;
        set_last_kernel("osc_stream_kernel");
    }
    *samples_out = k * hop;
    st->commit(T2, E2, flush, !flush);
    return FV_OK;
}

extern "C" {

FV_API int64_t fv_yin_frames_ready(const fv_f0_config* cfg, int64_t N) {
    YinPlan p;
    if (make_yin_plan(cfg, "fv_yin_frames_ready", p)) return -1;
    if (N < 0 || N > kSampleStreamMaxLen) {
        set_error("fv_yin_frames_ready: N = %lld must lie in [0, 2^40]", (long long)N);
        return -1;
    }
    return yin_ready(p, N);
}

FV_API fv_status fv_yin_stream_create(fv_f0* p, int32_t batch, int32_t max_chunk_samples, fv_yin_stream** out) {
    if (!p || !out) {
        set_error("fv_yin_stream_create: null argument");
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_yin_stream> st(new fv_yin_stream());
    st->p = p;
    // a frame not yet emitted starts less than H samples before N: W when hop <= W, half a hop more than half a frame otherwise
    const int H = p->plan.W / 2 + std::max(p->plan.W / 2, (p->plan.hop + 1) / 2);
    if (const fv_status rs = st->create("fv_yin_stream_create", batch, max_chunk_samples, H, ((long long)H + max_chunk_samples + 3) / 4 * 4))
        return rs;
    *out = st.release();
    return FV_OK;
}

FV_API int64_t fv_yin_stream_pending_samples(const fv_yin_stream* s) { return s ? yin_pending(s->p->plan, s->N, s->E) : 0; }

FV_API fv_status fv_yin_stream_push(fv_yin_stream* s, const float* d_wave, int64_t row_stride, int32_t c, float* d_f0, float* d_aperiodicity,
                                    int64_t out_row_stride, int64_t* frames_out, void* stream) {
    return yin_stream_step(s, d_wave, row_stride, c, false, d_f0, d_aperiodicity, out_row_stride, frames_out, stream);
}

FV_API fv_status fv_yin_stream_flush(fv_yin_stream* s, float* d_f0, float* d_aperiodicity, int64_t out_row_stride, int64_t* frames_out,
                                     void* stream) {
    return yin_stream_step(s, nullptr, 0, 0, true, d_f0, d_aperiodicity, out_row_stride, frames_out, stream);
}

FV_API fv_status fv_yin_stream_reset(fv_yin_stream* s) {
    if (!s) {
        set_error("fv_yin_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->reset();
    return FV_OK;
}

FV_API void fv_yin_stream_destroy(fv_yin_stream* s) { delete s; }

FV_API fv_status fv_osc_stream_create(fv_template* p, int32_t batch, int32_t max_chunk_frames, fv_osc_stream** out) {
    const char* fn = "fv_osc_stream_create";
    if (!p || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    const int hop = p->cfg.hop_length;
    if (max_chunk_frames >= 1 && (2LL + max_chunk_frames) * hop > kF0MaxLen) {
        set_error("%s: max_chunk_frames = %d frames of %d samples, with the two carried frames, pass 2^30 samples", fn, max_chunk_frames, hop);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_osc_stream> st(new fv_osc_stream());
    st->p = p;
    const long long stride = (2LL + max_chunk_frames + 3) / 4 * 4;
    if (const fv_status rs = st->create(fn, batch, max_chunk_frames, 2, stride)) return rs;
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    const size_t nchunk = (size_t)(((long long)max_chunk_frames * hop + kTmplChunk - 1) / kTmplChunk);
    const size_t nf = up((size_t)batch * (size_t)(2 + max_chunk_frames)), ns = up((size_t)batch * nchunk), np = up((size_t)batch);
    FV_HIP_CHECK(hipMalloc((void**)&st->aux, (nf + ns + 2 * np) * sizeof(uint32_t)));
    st->F = st->aux, st->sums = st->F + nf, st->phase[0] = st->sums + ns, st->phase[1] = st->phase[0] + np;
    *out = st.release();
    return FV_OK;
}

FV_API int64_t fv_osc_stream_pending_frames(const fv_osc_stream* s) { return s ? s->N - s->E : 0; }

FV_API fv_status fv_osc_stream_push(fv_osc_stream* s, const float* d_f0, int64_t row_stride, int32_t c, float* d_out, int64_t out_row_stride,
                                    int64_t* samples_out, void* stream) {
    return osc_stream_step(s, d_f0, row_stride, c, false, d_out, out_row_stride, samples_out, stream);
}

FV_API fv_status fv_osc_stream_flush(fv_osc_stream* s, float* d_out, int64_t out_row_stride, int64_t* samples_out, void* stream) {
    return osc_stream_step(s, nullptr, 0, 0, true, d_out, out_row_stride, samples_out, stream);
}

FV_API fv_status fv_osc_stream_reset(fv_osc_stream* s) {
    if (!s) {
        set_error("fv_osc_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->reset();
    return FV_OK;
}

FV_API void fv_osc_stream_destroy(fv_osc_stream* s) { delete s; }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Pools (fv_yinpool_*, fv_oscpool_*): the streams' rules per session on the per-session carry core (sample_pool.h).  Slot s carries its last H
// samples (tracker) or its last two F0 frames (oscillator) in buf[cur[s]] row s; the oscillator's phase at the start of frame E lies in
// phase[pcur[s]][s], and an item that emits writes the other array and flips that slot's bit alone.
// ---------------------------------------------------------------------------------------------
struct fv_yinpool : SamplePool {
    fv_f0* p = nullptr;
    long long max_frames = 0;   // fv_yinpool_max_frames
};

struct fv_oscpool : SamplePool {
    fv_template* p = nullptr;
    std::vector<unsigned char> pcur;   // the slot's phase is in phase[pcur[s]][s]
    uint32_t* aux = nullptr;           // one allocation: F (S, f_stride) | sums (S, sums_stride) | phase[2] (S)
    uint32_t *F = nullptr, *sums = nullptr, *phase[2] = {nullptr, nullptr};
    int f_stride = 0, sums_stride = 0;
    ~fv_oscpool() {
        if (aux) (void)hipFree(aux);
    }
};

// The most one tracker item emits: a push of max_chunk samples that also flushes, from a state with E = ready(N):
// g(N) = (N + max_chunk) / hop - ready(N).  From N = hop / 2 + W / 2 on, ready(N + hop) = ready(N) + 1, so g has the period hop there.
static long long yinpool_max_frames(const YinPlan& pl, int max_chunk) {
    long long best = 0;
    for (long long N = 0; N < pl.hop / 2 + pl.W / 2 + 2LL * pl.hop; ++N) best = std::max(best, (N + max_chunk) / pl.hop - yin_ready(pl, N));
    return best;
}

// The emission rules of one step, after the pool's admit
static void yinpool_emission(const YinPlan& pl, const int64_t* emitted, const fv_wavpool_item* items, int count, const long long* N2,
                             long long* E2) {
    for (int i = 0; i < count; ++i) {
        const long long E = emitted[items[i].session];
        E2[i] = std::max(E, items[i].flush ? N2[i] / pl.hop : yin_ready(pl, N2[i]));
    }
}

static void oscpool_emission(const int64_t* emitted, const fv_wavpool_item* items, int count, const long long* T2, long long* E2) {
    for (int i = 0; i < count; ++i) E2[i] = std::max((long long)emitted[items[i].session], items[i].flush ? T2[i] : T2[i] - 1);
}

extern "C" {

FV_API fv_status fv_yinpool_create(fv_f0* f, int32_t sessions, int32_t max_chunk, fv_yinpool** out) {
    const char* fn = "fv_yinpool_create";
    if (out) *out = nullptr;
    if (!f || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_yinpool> p(new fv_yinpool());
    p->p = f;
    const int H = f->plan.W / 2 + std::max(f->plan.W / 2, (f->plan.hop + 1) / 2);   // what fv_yin_stream_create carries
    if (const fv_status rs = p->create(fn, sessions, max_chunk, H)) return rs;
    p->max_frames = yinpool_max_frames(f->plan, max_chunk);
    *out = p.release();
    return FV_OK;
}

FV_API int64_t fv_yinpool_max_frames(const fv_yinpool* p) { return p ? p->max_frames : 0; }

FV_API int64_t fv_yinpool_received(const fv_yinpool* p, int32_t s) { return sample_pool_received(p, s); }

FV_API int64_t fv_yinpool_emitted(const fv_yinpool* p, int32_t s) { return sample_pool_emitted(p, s); }

FV_API int64_t fv_yinpool_pending(const fv_yinpool* p, int32_t s) {
    return p && s >= 0 && s < p->S ? yin_pending(p->p->plan, p->N[(size_t)s], p->E[(size_t)s]) : 0;
}

FV_API int64_t fv_yinpool_plan(const fv_f0_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                               const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out) {
    const char* fn = "fv_yinpool_plan";
    YinPlan pl;
    if (const fv_status st = make_yin_plan(cfg, fn, pl)) return st;
    if (const fv_status st = sample_pool_range(fn, sessions, max_chunk)) return st;
    return sample_pool_plan(fn, sessions, max_chunk, received, emitted, flushed, items, count, frames_out,
                            [&](const long long* N2, long long* E2) {
                                yinpool_emission(pl, emitted, items, count, N2, E2);
                                return FV_OK;
                            });
}

FV_API fv_status fv_yinpool_step(fv_yinpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_f0, float* d_aperiodicity, int64_t out_stride, int32_t out_cols, int64_t* frames_out, void* stream) {
    const char* fn = "fv_yinpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    for (int i = 0; frames_out && i < count; ++i) frames_out[i] = 0;
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status rs = p->admit(fn, "fv_yinpool_reset", items, count, d_chunks, chunk_stride, N2.data())) return rs;
    const YinPlan& pl = p->p->plan;
    yinpool_emission(pl, p->E.data(), items, count, N2.data(), E2.data());
    if (const fv_status rs = sample_pool_output(fn, "frames", items, count, p->E.data(), E2.data(), 1, d_f0 != nullptr, out_stride, out_cols))
        return rs;
    // one table entry per item, in item order: every row of the outputs is written; `carry` the items that push samples
    std::vector<SamplePoolEntry> rows, carry;
    p->build_entries(items, count, N2.data(), E2.data(), rows, carry);      // E2 - E <= out_cols: it fits an int
    for (int i = 0; i < count; ++i) {
        const SamplePoolEntry& en = rows[(size_t)i];
        const long long lo = en.first * pl.hop + pl.hop / 2 - pl.W / 2;
        if (en.count > 0 && en.carry_origin > 0 && lo < en.carry_origin) {   // (cannot happen: a frame not yet emitted starts less than H samples before N)
            set_error("%s: internal: frame %lld of session %d reads sample %lld, before the %d carried samples that end at %lld", fn, en.first,
                      items[i].session, lo, p->H, en.chunk_origin);
            return FV_ERR_INVALID;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (count > 0 && out_cols > 0 && d_f0) {
        const fv_status rs = for_each_launch_table<SamplePoolBlock>(count, rows.data(), [&](const SamplePoolBlock& blk, int, int nz) {
            hipLaunchKernelGGL(yin_pool_kernel, dim3((unsigned)out_cols, (unsigned)nz), dim3(pl.threads()), pl.lds_bytes(), s, d_chunks,
                               (long long)chunk_stride, p->buf[0], p->buf[1], (long long)p->H, blk, d_f0, d_aperiodicity, (long long)out_stride, pl);
            return FV_OK;
        });
        if (rs) return rs;
        set_last_kernel("yin_pool_kernel");
    }
    if (const fv_status rs = launch_sample_pool_carry(p->buf[0], p->buf[1], p->H, d_chunks, chunk_stride, carry.data(), (int)carry.size(), s))
        return rs;
    for (int i = 0; frames_out && i < count; ++i) frames_out[i] = E2[(size_t)i] - p->E[(size_t)items[i].session];
    p->commit(items, count, N2.data(), E2.data());
    return FV_OK;
}

FV_API fv_status fv_yinpool_reset(fv_yinpool* p, int32_t session) { return sample_pool_reset(p, "fv_yinpool_reset", session); }

FV_API void fv_yinpool_destroy(fv_yinpool* p) { delete p; }

FV_API fv_status fv_oscpool_create(fv_template* t, int32_t sessions, int32_t max_chunk_frames, fv_oscpool** out) {
    const char* fn = "fv_oscpool_create";
    if (out) *out = nullptr;
    if (!t || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    const int hop = t->cfg.hop_length;
    if (max_chunk_frames >= 1 && (2LL + max_chunk_frames) * hop > kF0MaxLen) {
        set_error("%s: max_chunk_frames = %d frames of %d samples, with the two carried frames, pass 2^30 samples", fn, max_chunk_frames, hop);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_oscpool> p(new fv_oscpool());
    p->p = t;
    if (const fv_status rs = p->create(fn, sessions, max_chunk_frames, 2)) return rs;
    p->pcur.assign((size_t)sessions, 0);
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    p->f_stride = (int)((2LL + max_chunk_frames + 3) / 4 * 4);
    p->sums_stride = (int)(((1LL + max_chunk_frames) * hop + kTmplChunk - 1) / kTmplChunk);   // a flushing item emits at most max_chunk + 1 frames
    const size_t nf = up((size_t)sessions * (size_t)p->f_stride), ns = up((size_t)sessions * (size_t)p->sums_stride), np = up((size_t)sessions);
    FV_HIP_CHECK(hipMalloc((void**)&p->aux, (nf + ns + 2 * np) * sizeof(uint32_t)));
    p->F = p->aux, p->sums = p->F + nf, p->phase[0] = p->sums + ns, p->phase[1] = p->phase[0] + np;
    *out = p.release();
    return FV_OK;
}

FV_API int64_t fv_oscpool_max_frames(const fv_oscpool* p) { return p ? (int64_t)p->max_chunk + 1 : 0; }

FV_API int64_t fv_oscpool_received(const fv_oscpool* p, int32_t s) { return sample_pool_received(p, s); }

FV_API int64_t fv_oscpool_emitted(const fv_oscpool* p, int32_t s) { return sample_pool_emitted(p, s); }

FV_API int64_t fv_oscpool_pending(const fv_oscpool* p, int32_t s) { return p && s >= 0 && s < p->S ? p->N[(size_t)s] - p->E[(size_t)s] : 0; }

FV_API int64_t fv_oscpool_plan(const fv_template_config* cfg, int32_t sessions, int32_t max_chunk_frames, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* frames_out) {
    const char* fn = "fv_oscpool_plan";
    if (const fv_status st = check_template_config(cfg, fn)) return st;
    if (const fv_status st = sample_pool_range(fn, sessions, max_chunk_frames)) return st;
    return sample_pool_plan(fn, sessions, max_chunk_frames, received, emitted, flushed, items, count, frames_out,
                            [&](const long long* T2, long long* E2) {
                                oscpool_emission(emitted, items, count, T2, E2);
                                return FV_OK;
                            });
}

FV_API fv_status fv_oscpool_step(fv_oscpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int64_t out_stride, int32_t out_cols, int64_t* frames_out, void* stream) {
    const char* fn = "fv_oscpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    for (int i = 0; frames_out && i < count; ++i) frames_out[i] = 0;
    std::vector<long long> T2((size_t)std::max(count, 0)), E2(T2.size());
    if (const fv_status rs = p->admit(fn, "fv_oscpool_reset", items, count, d_chunks, chunk_stride, T2.data())) return rs;
    const fv_template_config& cfg = p->p->cfg;
    const int hop = cfg.hop_length;
    oscpool_emission(p->E.data(), items, count, T2.data(), E2.data());
    if (const fv_status rs = sample_pool_output(fn, "samples", items, count, p->E.data(), E2.data(), hop, d_out != nullptr, out_stride, out_cols))
        return rs;
    std::vector<OscPoolEntry> rows((size_t)count);
    std::vector<SamplePoolEntry> carry;
    for (int i = 0; i < count; ++i) {
        const size_t s = (size_t)items[i].session;
        const long long Tn = p->N[s], E = p->E[s], o = Tn - 2;   // column 0 of the item's F row is frame o
        const int c = items[i].samples;
        if (E - o < 1 || E - o > 2) {   // (cannot happen: between calls Tn - E is 0 or 1)
            set_error("%s: internal: session %d has received %lld frames and emitted %lld", fn, items[i].session, Tn, E);
            return FV_ERR_INVALID;
        }
        OscPoolEntry en{};
        en.item = i, en.slot = items[i].session, en.bit = (int)p->cur[s];
        en.phase_in = E > 0 ? (int)p->pcur[s] : -1, en.phase_out = (int)p->pcur[s] ^ 1;
        en.fcount = 2 + c, en.lo_c = o < 0 ? (int)-o : 0, en.hi_c = (int)(T2[(size_t)i] - 1 - o);
        en.n_lo = (int)((E - o) * hop), en.n_hi = (int)((E2[(size_t)i] - o) * hop);
        en.nchunk = (en.n_hi - en.n_lo + kTmplChunk - 1) / kTmplChunk;
        rows[(size_t)i] = en;
        if (c > 0) carry.push_back(p->entry(i, items[i], T2[(size_t)i], E2[(size_t)i]));   // H = 2: the carry's origin is o
    }
    hipStream_t s = (hipStream_t)stream;
    if (count > 0 && out_cols > 0 && d_out) {
        const unsigned out_chunks = (unsigned)(((long long)out_cols + kTmplChunk - 1) / kTmplChunk);
        const fv_status rs = for_each_launch_table<OscPoolBlock>(count, rows.data(), [&](const OscPoolBlock& blk, int, int nz) -> fv_status {
            int nchunk = 0, fcols = 0;
            for (int k = 0; k < nz; ++k)
                if (blk.e[k].nchunk > 0) nchunk = std::max(nchunk, blk.e[k].nchunk), fcols = std::max(fcols, blk.e[k].fcount);
            if (nchunk > 0) {   // (an entry that emits nothing needs no increments: its workgroups only store zeros)
                hipLaunchKernelGGL(osc_pool_increment_kernel, dim3((unsigned)((fcols + 255) / 256), (unsigned)nz), dim3(256), 0, s, d_chunks,
                                   (long long)chunk_stride, p->buf[0], p->buf[1], blk, p->F, p->f_stride, fcols, cfg.sample_rate);
                FV_HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(osc_pool_sums_kernel, dim3((unsigned)nchunk, (unsigned)nz), dim3(256), 0, s, p->F, p->f_stride, p->sums,
                                   p->sums_stride, blk, hop);
                FV_HIP_CHECK(hipGetLastError());
            }
            hipLaunchKernelGGL(osc_pool_kernel, dim3(out_chunks, (unsigned)nz), dim3(256), 0, s, p->F, p->f_stride, p->sums, p->sums_stride, blk,
                               p->phase[0], p->phase[1], d_out, (long long)out_stride, out_cols, hop, cfg.kind, cfg.amplitude);
            return FV_OK;
        });
        if (rs) return rs;
        set_last_kernel("osc_pool_kernel");
    }
    if (const fv_status rs = launch_sample_pool_carry(p->buf[0], p->buf[1], p->H, d_chunks, chunk_stride, carry.data(), (int)carry.size(), s))
        return rs;
    for (int i = 0; i < count; ++i) {
        const size_t sl = (size_t)items[i].session;
        const long long k = E2[(size_t)i] - p->E[sl];
        if (frames_out) frames_out[i] = k;
        if (k > 0) p->pcur[sl] ^= 1;   // the step wrote the slot's other phase
    }
    p->commit(items, count, T2.data(), E2.data());
    return FV_OK;
}

FV_API fv_status fv_oscpool_reset(fv_oscpool* p, int32_t session) { return sample_pool_reset(p, "fv_oscpool_reset", session); }

FV_API void fv_oscpool_destroy(fv_oscpool* p) { delete p; }

}  // extern "C"
