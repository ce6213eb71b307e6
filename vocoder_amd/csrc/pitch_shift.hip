// Pitch shift (fv_pitch_shift_*, include/fishvoc.h): librosa.effects.pitch_shift of fish_vocoder/test.py:61-62 — a phase-vocoder time stretch by
// rate = n / o, then a resample from orig_freq back to sr — restated in integers where librosa keeps floats.
//
//   pv_frame_kernel        wave -> the zero-padded polyphase signal (B, hop, T + taps - 1) of the centred frames (polyphase_reflect_kernel's
//                          layout, zeros where that one reflects)
//   [STFT conv]            the window-folded DFT basis the log-mel front-end uses (stft_basis) -> Sp (B, 2 nb, T)
//   pv_polar_kernel        Sp -> |D| (float) and Theta (phase in turns, uint32 fixed point), each (B, nb, T + 2), the last two columns zero
//   pv_scan_synth_kernel   one wave per (b, k) row: an exclusive scan of Theta[j + 1] - Theta[j] over the T' output frames in wrapping uint32
//                          arithmetic (the wrap is the modulo 2 pi), magnitude interpolation, sincospi -> S (B, 2 nb, T')
//   [inverse-DFT conv]     the ISTFT head's basis (istft_basis) -> frames (B, n_fft, T')
//   istft_ola_kernel       overlap-add, envelope, crop n_fft / 2, Ls samples
//   resample_global_kernel orig_freq -> sr (resample.hip), cut or zero-padded to L
//
// Why integers: librosa's accumulator grows by about pi per hop and bin — 1e6 rad after 200 000 samples, where fp32 resolves 0.06 rad.  In
// turns modulo 1 the sum never grows: a uint32 holds it to 2^-32 turns, exactly, in any summation order.
#include <memory>
#include <numeric>

#include "engine_internal.h"

namespace fv {
namespace {

constexpr int64_t kPvMaxLen = 1LL << 30;

// yp[b][r][tp] = wave[b][tp hop + r - pad] inside [0, L), else 0.  The address is clamped and the value selected: no sample at or past L is loaded.
__global__ __launch_bounds__(256) void pv_frame_kernel(const float* __restrict__ wave, float* __restrict__ yp, long long x_stride, long long L,
                                                       int hop, int TP, int pad) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* wb = wave + (long long)b * x_stride;
    for (int i = ty; i < 32; i += 8) {   // read: consecutive lanes = consecutive samples (r) of frame slot t0 + i
        const int tp = t0 + i, r = r0 + tx;
        const long long idx = (long long)tp * hop + r - pad;
        const bool in = tp < TP && r < hop && idx >= 0 && idx < L;
        const long long at = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
        const float v = wb[at];
        tile[i][tx] = in ? v : 0.f;
    }
    __syncthreads();
    float* yb = yp + (long long)b * hop * TP;
    for (int i = ty; i < 32; i += 8) {   // write: consecutive lanes = consecutive frame slots
        const int r = r0 + i, tp = t0 + tx;
        if (r < hop && tp < TP) yb[(long long)r * TP + tp] = tile[tx][i];
    }
}

// mag = |D| (no epsilon: silence stays exact zero), theta = angle(D) in turns as uint32; columns T and T + 1 are zero
__global__ __launch_bounds__(256) void pv_polar_kernel(const float* __restrict__ spec, float* __restrict__ mag, uint32_t* __restrict__ theta,
                                                       int nb, int T) {
    const int T2 = T + 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nb * T2) return;
    const int b = blockIdx.y;
    const int k = (int)(i / T2), t = (int)(i - (long long)k * T2);
    float m = 0.f;
    uint32_t th = 0u;
    if (t < T) {
        const float* sb = spec + (long long)b * 2 * nb * T;
        const float re = sb[(long long)k * T + t], im = sb[(long long)(nb + k) * T + t];
        m = sqrtf(fmaf(re, re, im * im));
        if (re != 0.f || im != 0.f) th = (uint32_t)__double2ll_rn((double)atan2f(im, re) * (4294967296.0 / (2.0 * M_PI)));
    }
    mag[(long long)b * nb * T2 + i] = m;
    theta[(long long)b * nb * T2 + i] = th;
}

// One wave per (b, k) row walks the T' output columns 64 at a time, kPvUnroll chunks per trip.  Column s: q = s n, j = q / o, alpha = (q % o) / o;
// Phi[s] = Theta[0] + sum_{u < s} (Theta[j_u + 1] - Theta[j_u]): a wave-level exclusive scan (six __shfl_up steps) plus the carried total, all in
// wrapping uint32.  Lanes read and write consecutive columns; no LDS, no atomics, Phi is never stored.
// Each column pays one 64-bit division (q / o) beside the sincospif, and alpha = rem * (1 / o) rounds twice where rem / o would round once
// (within 2^-23, far inside the parity bar).  The kernel has not been timed (profiles/LOG.md R15.1), so stepping j and the remainder from column
// to column (as resample_body steps ph and base) is an untried option, not a known gain.
constexpr int kPvUnroll = 2;

__global__ __launch_bounds__(256) void pv_scan_synth_kernel(const float* __restrict__ mag, const uint32_t* __restrict__ theta,
                                                            float* __restrict__ spec, int rows, int nb, int T, int Tout, int o, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;   // (whole waves leave: the shuffles below always see 64 lanes)
    const int b = row / nb, k = row - b * nb;
    const float* mr = mag + (long long)row * (T + 2);
    const uint32_t* tr = theta + (long long)row * (T + 2);
    float* re = spec + ((long long)b * 2 * nb + k) * Tout;
    float* im = re + (long long)nb * Tout;
    const float inv_o = 1.0f / (float)o;
    uint32_t carry = tr[0];
    for (int s0 = 0; s0 < Tout; s0 += 64 * kPvUnroll) {
#pragma unroll
        for (int u = 0; u < kPvUnroll; ++u) {
            const int s = s0 + u * 64 + lane;
            const bool live = s < Tout;
            const long long q = (long long)(live ? s : 0) * n;
            const int j = (int)(q / o), rem = (int)(q - (long long)j * o);   // j <= T - 1: columns j and j + 1 exist
            const uint32_t th0 = tr[j], th1 = tr[j + 1];
            const float m0 = mr[j], m1 = mr[j + 1];
            const uint32_t d = live ? th1 - th0 : 0u;
            uint32_t inc = d;
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) {
                const uint32_t v = __shfl_up(inc, sh, 64);
                if (lane >= sh) inc += v;
            }
            const uint32_t phi = carry + (inc - d);
            carry += __shfl(inc, 63, 64);
            if (live) {
                const float alpha = (float)rem * inv_o;
                const float m = fmaf(alpha, m1, (1.0f - alpha) * m0);
                float sn, cs;
                sincospif((float)(int32_t)phi * (1.0f / 2147483648.0f), &sn, &cs);   // phi as signed turns in [-1/2, 1/2): 2 pi phi / 2^32 = pi x
                re[s] = m * cs;
                im[s] = m * sn;
            }
        }
    }
}

__global__ void pv_zero_tail_kernel(float* y, long long y_stride, long long from, long long to) {
    const long long i = from + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) y[(long long)blockIdx.y * y_stride + i] = 0.f;
}

struct Plan {
    int orig_freq = 0, o = 0, n = 0, N = 0, hop = 0;
};

fv_status make_plan(const fv_pitch_shift_config* c, const char* fn, Plan& p) {
    if (!c) {
        set_error("%s: null config", fn);
        return FV_ERR_INVALID;
    }
    if (c->sample_rate <= 0) {
        set_error("%s: sample_rate = %d must be > 0", fn, c->sample_rate);
        return FV_ERR_INVALID;
    }
    if (!std::isfinite(c->n_steps)) {
        set_error("%s: n_steps = %g must be finite", fn, c->n_steps);
        return FV_ERR_INVALID;
    }
    if (c->bins_per_octave < 1) {
        set_error("%s: bins_per_octave = %d must be >= 1", fn, c->bins_per_octave);
        return FV_ERR_INVALID;
    }
    if (c->n_fft < 2) {
        set_error("%s: n_fft = %d must be >= 2", fn, c->n_fft);
        return FV_ERR_INVALID;
    }
    if (c->hop_length < 0) {
        set_error("%s: hop_length = %d must be >= 0 (0: n_fft / 4)", fn, c->hop_length);
        return FV_ERR_INVALID;
    }
    if (c->freq_granularity < 1) {
        set_error("%s: freq_granularity = %d must be >= 1", fn, c->freq_granularity);
        return FV_ERR_INVALID;
    }
    const double f = std::floor((double)c->sample_rate * std::pow(2.0, c->n_steps / (double)c->bins_per_octave) + 0.5);
    if (!(f >= 1.0 && f <= 2147483647.0)) {
        set_error("%s: n_steps = %g moves %d Hz to %g Hz, outside [1, 2^31)", fn, c->n_steps, c->sample_rate, f);
        return FV_ERR_INVALID;
    }
    int of = (int)f;
    of -= of % c->freq_granularity;
    if (of < 1) {
        set_error("%s: n_steps = %g with freq_granularity = %d leaves orig_freq = 0", fn, c->n_steps, c->freq_granularity);
        return FV_ERR_INVALID;
    }
    const int g = std::gcd(of, c->sample_rate);
    p.orig_freq = of, p.o = of / g, p.n = c->sample_rate / g;
    p.N = c->n_fft, p.hop = c->hop_length ? c->hop_length : c->n_fft / 4;
    if (p.hop < 1 || p.N % p.hop || p.N % 2 || p.hop % 2) {
        set_error("%s: n_fft = %d and hop_length = %d: n_fft must be a multiple of hop_length and both even", fn, p.N, p.hop);
        return FV_ERR_UNSUPPORTED;
    }
    return FV_OK;
}

struct Lengths {
    int64_t T = 0, Tout = 0, Ls = 0, M = 0;
};
Lengths lengths_of(const Plan& p, int64_t L) {
    Lengths l;
    l.T = 1 + L / p.hop;
    l.Tout = (l.T * p.o + p.n - 1) / p.n;
    l.Ls = (2 * L * p.o + p.n) / (2 * (int64_t)p.n);
    l.M = ((int64_t)p.n * l.Ls + p.o - 1) / p.o;
    return l;
}

fv_resample_config resample_config(const fv_pitch_shift_config& c, const Plan& p) {
    fv_resample_config r{};
    r.orig_freq = p.orig_freq, r.new_freq = c.sample_rate, r.lowpass_filter_width = c.lowpass_filter_width;
    r.rolloff = c.rolloff, r.method = c.method, r.beta = c.beta;
    return r;
}

}  // namespace
}  // namespace fv

struct fv_pitch_shift {
    fv_pitch_shift_config cfg{};
    Plan plan;
    int nb = 0, taps = 0;
    ConvLayer stft, idft;
    float* d_win2 = nullptr;
    fv_resample* rs = nullptr;   // NULL when orig_freq == sample_rate: the call is a copy
    ~fv_pitch_shift() {
        conv_layer_destroy(stft);
        conv_layer_destroy(idft);
        if (d_win2) (void)hipFree(d_win2);
        fv_resample_destroy(rs);
    }
    bool identity() const { return plan.orig_freq == cfg.sample_rate; }

    // [Yp (B, hop, T + taps - 1) | Sp (B, 2 nb, T) | Mg (B, nb, T + 2) | Th (same, uint32) | S2 (B, 2 nb, T') | Fr (B, N, T') | St (B, Ls)], each
    // part rounded up to 64 floats
    struct Parts {
        float *Yp, *Sp, *Mg, *S2, *Fr, *St;
        uint32_t* Th;
        size_t elems;
    };
    Parts carve(float* ws, int B, const Lengths& l) const {
        auto up = [](size_t v) { return (v + 63) / 64 * 64; };
        const size_t b = (size_t)B;
        const size_t n_yp = up(b * plan.hop * (size_t)(l.T + taps - 1)), n_sp = up(b * 2 * nb * (size_t)l.T), n_mg = up(b * nb * (size_t)(l.T + 2));
        const size_t n_s2 = up(b * 2 * nb * (size_t)l.Tout), n_fr = up(b * plan.N * (size_t)l.Tout), n_st = up(b * (size_t)l.Ls);
        Parts p;
        p.Yp = ws, p.Sp = p.Yp + n_yp, p.Mg = p.Sp + n_sp, p.Th = (uint32_t*)(p.Mg + n_mg);
        p.S2 = p.Mg + 2 * n_mg, p.Fr = p.S2 + n_s2, p.St = p.Fr + n_fr;
        p.elems = n_yp + n_sp + 2 * n_mg + n_s2 + n_fr + n_st;
        return p;
    }
};

// the time stretch of `B` rows into rows of Ls samples at y (stride y_stride >= Ls)
static fv_status pv_stretch(fv_pitch_shift* p, const float* d_x, long long x_stride, float* y, long long y_stride, int B, long long L,
                            const Lengths& l, const fv_pitch_shift::Parts& w, hipStream_t s) {
    const Plan& pl = p->plan;
    const int hop = pl.hop, N = pl.N, nb = p->nb, T = (int)l.T, Tout = (int)l.Tout, TP = T + p->taps - 1;
    hipLaunchKernelGGL(pv_frame_kernel, dim3((TP + 31) / 32, (hop + 31) / 32, B), dim3(256), 0, s, d_x, w.Yp, x_stride, L, hop, TP, N / 2);
    FV_HIP_CHECK(hipGetLastError());
    ConvRun r;
    r.batch = B, r.t_in = TP, r.x = w.Yp, r.y = w.Sp;
    if (const fv_status st = conv_layer_run(p->stft, r, s)) return st;
    const long long per = (long long)nb * (T + 2);
    hipLaunchKernelGGL(pv_polar_kernel, dim3((unsigned)((per + 255) / 256), B), dim3(256), 0, s, w.Sp, w.Mg, w.Th, nb, T);
    FV_HIP_CHECK(hipGetLastError());
    const int rows = B * nb;
    hipLaunchKernelGGL(pv_scan_synth_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w.Mg, w.Th, w.S2, rows, nb, T, Tout, pl.o, pl.n);
    FV_HIP_CHECK(hipGetLastError());
    set_last_kernel("pv_scan_synth_kernel");
    r = ConvRun();
    r.batch = B, r.t_in = Tout, r.x = w.S2, r.y = w.Fr;
    if (const fv_status st = conv_layer_run(p->idft, r, s)) return st;
    // (every sample below Ls lies under a frame: Ls <= L o / n + 1/2 < T' hop + N / 2; where the envelope is zero the kernel writes 0)
    float* dst = y_stride == l.Ls ? y : w.St;
    if (const fv_status st = launch_istft_ola(w.Fr, p->d_win2, dst, B, N, Tout, hop, N / 2, l.Ls, s)) return st;
    if (dst != y)
        FV_HIP_CHECK(hipMemcpy2DAsync(y, (size_t)y_stride * 4, dst, (size_t)l.Ls * 4, (size_t)l.Ls * 4, (size_t)B, hipMemcpyDeviceToDevice, s));
    return FV_OK;
}

static fv_status pv_call(fv_pitch_shift* p, const char* fn, bool whole, const float* d_x, int64_t x_row_stride, float* d_y, int64_t y_row_stride,
                         int32_t batch, int64_t L, void* ws, size_t ws_bytes, void* stream) {
    if (!p) {
        set_error("%s: null pitch shifter", fn);
        return FV_ERR_INVALID;
    }
    if (batch < 0 || batch > 65535 || L < 0 || L > kPvMaxLen) {
        set_error("%s: batch = %d must lie in [0, 65535] and L = %lld in [0, 2^30]", fn, batch, (long long)L);
        return FV_ERR_INVALID;
    }
    if (batch == 0 || L == 0) return FV_OK;
    const Lengths l = lengths_of(p->plan, L);
    const int64_t out = whole ? L : l.Ls;
    if (out == 0) return FV_OK;   // (a stretch of a row so short that round(L o / n) = 0)
    if (!d_x || !d_y) {
        set_error("%s: null %s", fn, d_x ? "d_y" : "d_x");
        return FV_ERR_INVALID;
    }
    if (x_row_stride < L || y_row_stride < out) {
        set_error("%s: row strides (%lld, %lld) are shorter than the rows (L = %lld, %lld outputs)", fn, (long long)x_row_stride,
                  (long long)y_row_stride, (long long)L, (long long)out);
        return FV_ERR_INVALID;
    }
    const float *x_end = d_x + (int64_t)(batch - 1) * x_row_stride + L, *y_end = d_y + (int64_t)(batch - 1) * y_row_stride + out;
    if (d_x < y_end && d_y < x_end) {
        set_error("%s: d_y overlaps d_x; the pitch shift does not run in place (every frame reads n_fft input samples)", fn);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (p->identity()) {   // rate 1: a bit-for-bit copy
        FV_HIP_CHECK(hipMemcpy2DAsync(d_y, (size_t)y_row_stride * 4, d_x, (size_t)x_row_stride * 4, (size_t)L * 4, (size_t)batch,
                                      hipMemcpyDeviceToDevice, s));
        return FV_OK;
    }
    if ((int64_t)p->plan.N * l.Tout >= (1LL << 31) || l.T + p->taps >= (1LL << 30)) {
        set_error("%s: L = %lld gives %lld stretched frames of %d samples, more than 2^31 elements per row; split the row", fn, (long long)L,
                  (long long)l.Tout, p->plan.N);
        return FV_ERR_UNSUPPORTED;
    }
    const size_t need = fv_pitch_shift_workspace_bytes(p, batch, L);
    if (!ws || ws_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_pitch_shift_workspace_bytes)", fn, ws ? ws_bytes : (size_t)0, need);
        return FV_ERR_INVALID;
    }
    const fv_pitch_shift::Parts w = p->carve((float*)ws, batch, l);
    if (!whole) return pv_stretch(p, d_x, x_row_stride, d_y, y_row_stride, batch, L, l, w, s);
    if (l.Ls > 0)
        if (const fv_status st = pv_stretch(p, d_x, x_row_stride, w.St, l.Ls, batch, L, l, w, s)) return st;
    const int64_t keep = std::min<int64_t>(l.M, L);   // (Ls = 0: M = 0, the rows are zeros)
    if (const fv_status st = resample_rows(p->rs, fn, w.St, l.Ls, l.Ls, d_y, y_row_stride, batch, keep, s)) return st;
    if (keep < L) {
        hipLaunchKernelGGL(pv_zero_tail_kernel, dim3((unsigned)((L - keep + 255) / 256), batch), dim3(256), 0, s, d_y, (long long)y_row_stride,
                           (long long)keep, (long long)L);
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

extern "C" {

FV_API fv_status fv_pitch_shift_plan(const fv_pitch_shift_config* cfg, int32_t* orig_freq, int32_t* o, int32_t* n) {
    Plan p;
    if (const fv_status st = make_plan(cfg, "fv_pitch_shift_plan", p)) return st;
    if (orig_freq) *orig_freq = p.orig_freq;
    if (o) *o = p.o;
    if (n) *n = p.n;
    return FV_OK;
}

FV_API fv_status fv_pitch_shift_lengths(const fv_pitch_shift_config* cfg, int64_t L, int64_t* frames, int64_t* frames_out, int64_t* stretched,
                                        int64_t* resampled) {
    Plan p;
    if (const fv_status st = make_plan(cfg, "fv_pitch_shift_lengths", p)) return st;
    if (L < 0 || L > kPvMaxLen) {
        set_error("fv_pitch_shift_lengths: L = %lld must lie in [0, 2^30]", (long long)L);
        return FV_ERR_INVALID;
    }
    const Lengths l = lengths_of(p, L);
    if (frames) *frames = l.T;
    if (frames_out) *frames_out = l.Tout;
    if (stretched) *stretched = l.Ls;
    if (resampled) *resampled = l.M;
    return FV_OK;
}

FV_API fv_status fv_pitch_shift_create(const fv_pitch_shift_config* cfg, fv_pitch_shift** out) {
    const char* fn = "fv_pitch_shift_create";
    if (!out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_pitch_shift> p(new fv_pitch_shift());
    if (const fv_status st = make_plan(cfg, fn, p->plan)) return st;
    p->cfg = *cfg;
    const Plan& pl = p->plan;
    const fv_resample_config rc = resample_config(*cfg, pl);
    {   // the filter's own checks (lowpass_filter_width, rolloff, method, beta), before anything is allocated
        int32_t o, n, width, kp;
        if (const fv_status st = fv_resample_design(&rc, &o, &n, &width, &kp, nullptr, nullptr, 0, nullptr, 0)) return st;
    }
    if (p->identity()) {
        *out = p.release();
        return FV_OK;
    }
    const int N = pl.N, hop = pl.hop;
    p->nb = N / 2 + 1, p->taps = N / hop;
    std::vector<float> win(N), win2(N);
    for (int i = 0; i < N; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / N));   // hann, periodic
    for (int i = 0; i < N; ++i) win2[i] = win[i] * win[i];
    const std::vector<float> wst = stft_basis(win, N, hop, p->taps), wid = istft_basis(win, N);
    fv_status st;
    if ((st = conv_layer_create(p->stft, false, hop, 2 * p->nb, p->taps, 1, 0, 1, wst.data(), nullptr))) return st;
    if ((st = conv_layer_create(p->idft, false, 2 * p->nb, N, 1, 1, 0, 1, wid.data(), nullptr))) return st;
    if ((st = upload(win2, &p->d_win2))) return st;
    if ((st = fv_global_resample_create(&rc, &p->rs))) return st;
    *out = p.release();
    return FV_OK;
}

FV_API void fv_pitch_shift_destroy(fv_pitch_shift* p) { delete p; }

FV_API size_t fv_pitch_shift_workspace_bytes(const fv_pitch_shift* p, int32_t batch, int64_t L) {
    if (!p || batch < 1 || L < 1 || L > kPvMaxLen || p->identity()) return 0;
    return align_up(p->carve(nullptr, batch, lengths_of(p->plan, L)).elems * sizeof(float), 256);
}

FV_API fv_status fv_pitch_shift_stretch(fv_pitch_shift* p, const float* d_x, int64_t x_row_stride, float* d_y, int64_t y_row_stride,
                                        int32_t batch, int64_t L, void* d_workspace, size_t workspace_bytes, void* stream) {
    return pv_call(p, "fv_pitch_shift_stretch", false, d_x, x_row_stride, d_y, y_row_stride, batch, L, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_pitch_shift_forward(fv_pitch_shift* p, const float* d_x, int64_t x_row_stride, float* d_y, int64_t y_row_stride,
                                        int32_t batch, int64_t L, void* d_workspace, size_t workspace_bytes, void* stream) {
    return pv_call(p, "fv_pitch_shift_forward", true, d_x, x_row_stride, d_y, y_row_stride, batch, L, d_workspace, workspace_bytes, stream);
}

}  // extern "C"
