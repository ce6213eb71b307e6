// F0 tracking and pitch templates (fv_f0_*, fv_template_*, include/fishvoc.h): what a user of the template generators (refinegan.py:287,
// hifigan.py:226) brings from a CPU F0 tracker today, on the GPU.
//
//   yin_f0_kernel              one workgroup per (row, frame): the frame staged once in LDS, the direct-form difference function
//                              d(tau) = sum_{j < Wi} (x[j] - x[j + tau])^2 with four consecutive lags per lane, the cumulative-mean normalisation as
//                              a scan over 64-lag chunks, the first dip as an integer min-reduction, the parabola by one lane
//   f0_increment_kernel        f0 (Hz) -> F = rint(f0 / sr * 2^32), the phase increment per sample in turns / 2^32 as uint32; 0 = unvoiced
//   f0_template_sums_kernel    per kTmplChunk samples of a row: the sum of the interpolated increments, wrapping uint32
//   f0_template_kernel         carry = the sums of the chunks before this one; a workgroup scan inside the chunk; sin / sawtooth of the phase
//
// Why the direct form: E(0) + E(tau) - 2 r(tau) cancels in fp32 exactly where d is small, the voiced case.  Every d(tau) is one fp32 accumulator
// over ascending j with fused multiply-adds, and the running sum is scanned in chunks of 64 lags whatever the launch: a frame's bits depend on
// the plan alone.  Why integers for the phase: the same reason as pv_scan_synth_kernel's accumulator (pitch_shift.hip) — the sum never grows
// and is exact in any order.  The sample streams' carry core (sample_stream.h) carries the last H samples of a row from call to call; a prefix
// sum has no such history, so the two-level scan here is its own.
#include <memory>

#include "engine_internal.h"

namespace fv {
namespace {

constexpr int kF0MaxFrame = 4096;       // W: the staged frame, d, its scan and the chunk totals stay under 64 KiB of LDS
constexpr int64_t kF0MaxLen = 1LL << 30;
constexpr int kF0Rows = 32;             // per-row lengths travel by value, kF0Rows rows per launch (as LogmelRowBlock's do)
constexpr int kYinLags = 4;             // consecutive lags per lane: one 16-byte LDS read feeds sixteen subtract-and-FMAs
constexpr int kYinMaxThreads = 512;
constexpr int kTmplItems = 8;           // consecutive samples per thread
constexpr int kTmplChunk = 256 * kTmplItems;

struct F0RowBlock {
    int len[kF0Rows];
};

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

// grid (frames T, rows); block pl.threads().  LDS: xs[W + 8] (the frame, then zeros) | dl[d_elems] (d, then d') | cs[d_elems] (the prefix inside
// a 64-lag chunk) | ct[d_elems / 64] (chunk totals) | red[32].  Samples before 0 or at or past the row's length are zeros by index: the address is
// clamped and the value selected, so no sample past the length is loaded.
__global__ __launch_bounds__(kYinMaxThreads) void yin_f0_kernel(const float* __restrict__ x, long long x_stride, F0RowBlock rows, int row0,
                                                                float* __restrict__ f0, float* __restrict__ ap, long long out_stride, int T,
                                                                YinPlan pl) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int t = blockIdx.x, b = row0 + blockIdx.y;
    const int len = rows.len[blockIdx.y];
    float* f0r = f0 + (long long)b * out_stride;
    float* apr = ap + (long long)b * out_stride;
    if (t >= len / pl.hop) {   // (the whole workgroup leaves: no barrier below is reached by a part of it)
        if (tid == 0) f0r[t] = 0.f, apr[t] = 0.f;
        return;
    }
    const int W = pl.W, Wi = pl.Wi, NL = pl.lags(), DE = pl.d_elems();
    float* xs = lds;
    float* dl = xs + W + 8;
    float* cs = dl + DE;
    float* ct = cs + DE;
    float* red = ct + DE / 64;
    const float* xr = x + (long long)b * x_stride;
    const long long lo = (long long)t * pl.hop + pl.hop / 2 - W / 2;
    for (int i = tid; i < W + 8; i += nthr) {
        const long long idx = lo + i;
        const bool in = i < W && idx >= 0 && idx < len;
        const long long at = idx < 0 ? 0 : (idx >= len ? len - 1 : idx);
        const float v = xr[at];
        xs[i] = in ? v : 0.f;
    }
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
        f0r[t] = f;
        apr[t] = aper;
    }
}

// F[b][t] = rint(f0 / sr * 2^32) in double for 0 < f0 < sr and t < frames[b], else 0 (unvoiced; NaN and padded frames included)
__global__ __launch_bounds__(256) void f0_increment_kernel(const float* __restrict__ f0, long long f0_stride, F0RowBlock rows, int row0,
                                                           uint32_t* __restrict__ F, int T, int sr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = row0 + blockIdx.y;
    uint32_t v = 0u;
    if (t < rows.len[blockIdx.y]) {
        const float f = f0[(long long)b * f0_stride + t];
        if (f > 0.f && f < (float)sr) v = (uint32_t)__double2ll_rn((double)f / (double)sr * 4294967296.0);
    }
    F[(long long)b * T + t] = v;
}

// The increment of sample n of a row of Ti frames: between the frame centres a = floor((n - hop / 2) / hop) and a + 1, both clamped to
// [0, Ti - 1], k samples past centre a; an unvoiced neighbour (F = 0) takes the other one's value
__device__ __forceinline__ uint32_t tmpl_inc(const uint32_t* __restrict__ Fr, int Ti, int hop, int n) {
    const int m = n - hop / 2;
    const int a = m >= 0 ? m / hop : -1;
    const int k = m - a * hop;
    uint32_t Fa = Fr[min(max(a, 0), Ti - 1)], Fb = Fr[min(a + 1, Ti - 1)];
    if (Fa == 0u) Fa = Fb;
    else if (Fb == 0u) Fb = Fa;
    return (uint32_t)(((unsigned long long)Fa * (unsigned)(hop - k) + (unsigned long long)Fb * (unsigned)k) / (unsigned)hop);
}

// grid (chunks, rows): sums[b][chunk] = the sum of the chunk's increments, wrapping
__global__ __launch_bounds__(256) void f0_template_sums_kernel(const uint32_t* __restrict__ F, F0RowBlock rows, int row0,
                                                               uint32_t* __restrict__ sums, int T, int hop, int nchunk) {
    __shared__ uint32_t part[4];
    const int b = row0 + blockIdx.y, Ti = rows.len[blockIdx.y], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Ni = Ti * hop;
    const uint32_t* Fr = F + (long long)b * T;
    const int n0 = blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems;
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i)
        if (n0 + i < Ni) s += tmpl_inc(Fr, Ti, hop, n0 + i);
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[(long long)b * nchunk + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// grid (chunks, rows): phi[n] = sum_{m <= n} inc[m] = (the chunks before) + (the threads before, a workgroup scan) + (this thread's own samples)
__global__ __launch_bounds__(256) void f0_template_kernel(const uint32_t* __restrict__ F, const uint32_t* __restrict__ sums, F0RowBlock rows,
                                                          int row0, float* __restrict__ out, long long out_stride, int T, int hop, int nchunk,
                                                          int kind, float amplitude) {
    __shared__ uint32_t part[4], wtot[4];
    const int b = row0 + blockIdx.y, Ti = rows.len[blockIdx.y], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = T * hop, Ni = Ti * hop;
    const uint32_t* Fr = F + (long long)b * T;
    float* orow = out + (long long)b * out_stride;
    const int n0 = blockIdx.x * kTmplChunk + threadIdx.x * kTmplItems;
    uint32_t carry = 0u;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) carry += sums[(long long)b * nchunk + c];
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) carry += __shfl_xor(carry, sh, 64);
    if (lane == 0) part[wave] = carry;
    uint32_t ph[kTmplItems];
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i) {
        if (n0 + i < Ni) s += tmpl_inc(Fr, Ti, hop, n0 + i);
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
#pragma unroll
    for (int i = 0; i < kTmplItems; ++i) {
        const int n = n0 + i;
        if (n >= N) break;
        float v = 0.f;
        if (n < Ni && Fr[n / hop] != 0u) {
            const uint32_t phi = base + ph[i];
            if (kind == FV_TEMPLATE_SAWTOOTH)
                v = amplitude * ((float)(int32_t)(phi ^ 0x80000000u) * (1.0f / 2147483648.0f));   // 2 phi / 2^32 - 1
            else
                v = amplitude * sinpif((float)(int32_t)phi * (1.0f / 2147483648.0f));   // phi as signed turns: 2 pi phi / 2^32 = pi x
        }
        orow[n] = v;
    }
}

// the lengths of the rows [row0, row0 + count) by value; host == NULL: every row has `whole`
fv_status row_block(const char* fn, const char* what, const int32_t* host, int row0, int count, int whole, F0RowBlock& rb) {
    for (int i = 0; i < kF0Rows; ++i) {
        const int v = i < count ? (host ? host[row0 + i] : whole) : 0;
        if (v < 0 || v > whole) {
            set_error("%s: row %d has %s = %d, outside [0, %d]", fn, row0 + i, what, v, whole);
            return FV_ERR_INVALID;
        }
        rb.len[i] = v;
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
    std::vector<F0RowBlock> blocks((batch + kF0Rows - 1) / kF0Rows);   // everything is validated before anything is enqueued
    for (size_t i = 0; i < blocks.size(); ++i)
        if (const fv_status st = row_block(fn, "length", host_lengths, (int)i * kF0Rows, std::min(kF0Rows, batch - (int)i * kF0Rows), (int)L,
                                           blocks[i]))
            return st;
    hipStream_t s = (hipStream_t)stream;
    for (size_t i = 0; i < blocks.size(); ++i) {
        const int row0 = (int)i * kF0Rows, count = std::min(kF0Rows, batch - row0);
        hipLaunchKernelGGL(yin_f0_kernel, dim3((unsigned)T, count), dim3(pl.threads()), pl.lds_bytes(), s, d_x, (long long)x_row_stride,
                           blocks[i], row0, d_f0, d_aperiodicity, (long long)out_row_stride, (int)T, pl);
        FV_HIP_CHECK(hipGetLastError());
    }
    set_last_kernel("yin_f0_kernel");
    return FV_OK;
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
    std::vector<F0RowBlock> blocks((batch + kF0Rows - 1) / kF0Rows);
    for (size_t i = 0; i < blocks.size(); ++i)
        if (const fv_status st = row_block(fn, "frames", host_frames, (int)i * kF0Rows, std::min(kF0Rows, batch - (int)i * kF0Rows), (int)T,
                                           blocks[i]))
            return st;
    size_t f_words = 0;
    (void)template_words(batch, T, hop, &f_words);
    uint32_t* F = (uint32_t*)d_workspace;
    uint32_t* sums = F + f_words;
    const int nchunk = (int)((T * hop + kTmplChunk - 1) / kTmplChunk);
    hipStream_t s = (hipStream_t)stream;
    for (size_t i = 0; i < blocks.size(); ++i) {
        const int row0 = (int)i * kF0Rows, count = std::min(kF0Rows, batch - row0);
        hipLaunchKernelGGL(f0_increment_kernel, dim3((unsigned)((T + 255) / 256), count), dim3(256), 0, s, d_f0, (long long)f0_row_stride,
                           blocks[i], row0, F, (int)T, p->cfg.sample_rate);
        FV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(f0_template_sums_kernel, dim3(nchunk, count), dim3(256), 0, s, F, blocks[i], row0, sums, (int)T, hop, nchunk);
        FV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(f0_template_kernel, dim3(nchunk, count), dim3(256), 0, s, F, sums, blocks[i], row0, d_out,
                           (long long)out_row_stride, (int)T, hop, nchunk, p->cfg.kind, p->cfg.amplitude);
        FV_HIP_CHECK(hipGetLastError());
    }
    set_last_kernel("f0_template_kernel");
    return FV_OK;
}

}  // extern "C"
