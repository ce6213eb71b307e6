// Pitch shift (fv_pitch_shift_*, include/fishvoc.h): librosa.effects.pitch_shift of fish_vocoder/test.py:61-62 — a phase-vocoder time stretch by
// rate = n / o, then a resample from orig_freq back to sr — restated in integers where librosa keeps floats.
//
//   pv_frame_kernel        wave -> the zero-padded polyphase signal (B, hop, T + taps - 1) of the centred frames (polyphase_reflect_kernel's
//                          layout, zeros where that one reflects; frame_kernels.hip)
//   [STFT conv]            the window-folded DFT basis the log-mel front-end uses (stft_basis) -> Sp (B, 2 nb, T)
//   pv_polar_kernel        Sp -> |D| (float) and Theta (phase in turns, uint32 fixed point), each (B, nb, T + 2), the last two columns zero
//   pv_scan_synth_kernel   one wave per (b, k) row: an exclusive scan of Theta[j + 1] - Theta[j] over the T' output frames in wrapping uint32
//                          arithmetic (the wrap is the modulo 2 pi), magnitude interpolation, sincospi -> S (B, 2 nb, T')
//   [inverse-DFT conv]     the ISTFT head's basis (istft_basis) -> frames (B, n_fft, T')
//   istft_ola_kernel       overlap-add, envelope, crop n_fft / 2, Ls samples (frame_kernels.hip)
//   resample_global_kernel orig_freq -> sr (resample.hip), cut or zero-padded to L
//
// The stream (fv_pv_stream_*) runs the same chain on the frames, columns and samples that a push made ready (the rule is stream_ready below);
// every stage is the whole row's body behind another fetch (pv_scan_row here, polyphase_tile and ola_tile in frame_kernels.hip):
//   pv_frame_window_kernel       the polyphase signal of the analysis frames [A, A2) from the carried samples plus the chunk
//   pv_scan_synth_stream_kernel  the scan over the stretched frames [S, S2), resumed from the carried column A - 1 and the carried Phi
//   istft_ola_window_kernel      the stretched samples [Y, Y2) from the carried frames plus the new ones
//   pv_frame_carry_kernel        the last n_fft / hop synthesised frames, into the other buffer of the pair
// with pv_polar_kernel, the two convs (always in batch-invariant mode) and an fv_resample_stream between and behind them.
//
// The pool (fv_pvpool_*) runs it for sessions that advance independently: the same bodies behind a third fetch, one table entry per item,
//   pv_frame_pool_window_kernel   the window from the slot's carried samples plus the item's chunk row (frame_kernels.hip)
//   pv_polar_pool_kernel          rows padded to the step's largest dA; every column from an entry's own dA on is written as zero
//   pv_scan_synth_pool_kernel     the scan per (entry, k) row, the slot's polar carry in, its other half out
//   istft_ola_pool_window_kernel, pv_frame_pool_carry_kernel   per-entry (S, dS, Tend, Y, Y2) and the slot's frame carry (frame_kernels.hip)
// with the two convs once per step over all rows and an inner fv_respool behind them.
//
// Why integers: librosa's accumulator grows by about pi per hop and bin — 1e6 rad after 200 000 samples, where fp32 resolves 0.06 rad.  In
// turns modulo 1 the sum never grows: a uint32 holds it to 2^-32 turns, exactly, in any summation order.
#include <memory>
#include <numeric>
#include <optional>

#include "engine_internal.h"
#include "sample_pool.h"
#include "sample_stream.h"

namespace fv {
namespace {

constexpr int64_t kPvMaxLen = 1LL << 30;

// one bin of one column: |D| (no epsilon: silence stays exact zero) and angle(D) in turns as uint32
__device__ __forceinline__ void pv_polar(float re, float im, float& m, uint32_t& th) {
    m = sqrtf(fmaf(re, re, im * im));
    th = 0u;
    if (re != 0.f || im != 0.f) th = (uint32_t)__double2ll_rn((double)atan2f(im, re) * (4294967296.0 / (2.0 * M_PI)));
}

// mag = |D|, theta = angle(D); columns T and T + 1 are zero
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
        pv_polar(sb[(long long)k * T + t], sb[(long long)(nb + k) * T + t], m, th);
    }
    mag[(long long)b * nb * T2 + i] = m;
    theta[(long long)b * nb * T2 + i] = th;
}

// The pool's tables (fv_pvpool_step): tensor row k0 + (block index) is one entry, at most kSamplePoolBlock per launch, by value
struct PvScanEntry {
    int slot, pbit;        // the slot's polar carry is in pol[pbit]; an entry with dA > 0 or dS > 0 writes pol[pbit ^ 1]
    int dA, dS;            // analysed columns [A, A + dA) and stretched frames [S, S + dS) of this row
    long long A, S;
};
using PvScanBlock = LaunchTable<PvScanEntry, kSamplePoolBlock>;

// pv_polar_kernel per entry: spec (rows, 2 nb, T) is the conv over rows padded to the launch's largest dA = T, mag / theta (rows, nb, T + 2).
// Entry i owns the columns below dA_i; every column from dA_i on is WRITTEN as zero — column dA_i of the conv reads taps - 1 real polyphase
// slots and is not zero on its own, and a flushing entry reads its columns dA_i and dA_i + 1 as the row's columns T and T + 1.
__global__ __launch_bounds__(256) void pv_polar_pool_kernel(const float* __restrict__ spec, float* __restrict__ mag, uint32_t* __restrict__ theta,
                                                            const PvScanBlock tab, int nb, int T, int k0) {
    const int T2 = T + 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nb * T2) return;
    const long long row = k0 + blockIdx.y;
    const int dA = tab.e[blockIdx.y].dA;
    const int k = (int)(i / T2), t = (int)(i - (long long)k * T2);
    float m = 0.f;
    uint32_t th = 0u;
    if (t < dA) {
        const float* sb = spec + row * 2 * nb * T;
        pv_polar(sb[(long long)k * T + t], sb[(long long)(nb + k) * T + t], m, th);
    }
    mag[row * nb * T2 + i] = m;
    theta[row * nb * T2 + i] = th;
}

// One wave walks the dS output columns [start, start + dS) of one (b, k) row 64 at a time, kPvUnroll chunks per trip.  Column s: q = s n, j = q / o,
// alpha = (q % o) / o; Phi[s] = Theta[0] + sum_{u < s} (Theta[j_u + 1] - Theta[j_u]): a wave-level exclusive scan (six __shfl_up steps) plus the
// carried total, all in wrapping uint32.  `carry` is Phi[start] on entry and Phi[start + dS] on return.  cols(j, m, th) fetches column j of |D| and
// Theta; its Index type is the width j is kept in.  Lanes read and write consecutive columns; no LDS, no atomics, Phi is never stored.
// Each column pays one 64-bit division (q / o) beside the sincospif, and alpha = rem * (1 / o) rounds twice where rem / o would round once
// (within 2^-23, far inside the parity bar).  Stepping j and the remainder from column to column (as resample_body steps ph and base) is an
// untried option, not a known gain.
constexpr int kPvUnroll = 2;

template <class Cols>
__device__ __forceinline__ void pv_scan_row(const Cols& cols, float* __restrict__ re, float* __restrict__ im, long long start, int dS,
                                            uint32_t& carry, int o, int n) {
    using Index = typename Cols::Index;
    const int lane = threadIdx.x & 63;
    const float inv_o = 1.0f / (float)o;
    for (int s0 = 0; s0 < dS; s0 += 64 * kPvUnroll) {
#pragma unroll
        for (int u = 0; u < kPvUnroll; ++u) {
            const int s = s0 + u * 64 + lane;
            const bool live = s < dS;
            const long long q = (start + (live ? s : 0)) * n;
            const Index j = (Index)(q / o);
            const int rem = (int)(q - (long long)j * o);
            float m0, m1;
            uint32_t th0, th1;
            cols(j, m0, th0);
            cols(j + 1, m1, th1);
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

// the whole row: columns [0, T + 2) in place, j <= T - 1 so that columns j and j + 1 exist; the scan starts from Theta[0]
struct PvRowCols {
    using Index = int;
    const float* mr;
    const uint32_t* tr;
    __device__ __forceinline__ void operator()(int j, float& m, uint32_t& th) const { m = mr[j], th = tr[j]; }
};

__global__ __launch_bounds__(256) void pv_scan_synth_kernel(const float* __restrict__ mag, const uint32_t* __restrict__ theta,
                                                            float* __restrict__ spec, int rows, int nb, int T, int Tout, int o, int n) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;   // (whole waves leave: the shuffles of the scan always see 64 lanes)
    const int b = row / nb, k = row - b * nb;
    const PvRowCols cols{mag + (long long)row * (T + 2), theta + (long long)row * (T + 2)};
    float* re = spec + ((long long)b * 2 * nb + k) * Tout;
    uint32_t carry = cols.tr[0];
    pv_scan_row(cols, re, re + (long long)nb * Tout, 0, Tout, carry, o, n);
}

// The stream's window: mr / tr hold the analysed columns [A, A + dA) and two zero columns behind them (read at the flush only, where they are
// the columns T and T + 1); column A - 1 is the carried (cm, ct).  w = j - A lies in [-1, dA + 1] by the rule and is clamped, so that no address
// leaves the window.
struct PvWindowCols {
    using Index = long long;
    const float* mr;
    const uint32_t* tr;
    float cm;
    uint32_t ct;
    long long A;
    int dA;
    __device__ __forceinline__ void operator()(long long j, float& m, uint32_t& th) const {
        long long w = j - A;
        w = w > dA + 1 ? dA + 1 : w;
        const int at = w < 0 ? 0 : (int)w;
        const float mw = mr[at];
        const uint32_t tw = tr[at];
        m = w < 0 ? cm : mw;
        th = w < 0 ? ct : tw;
    }
};

// pv_scan_synth_kernel over the stretched frames [S, S + dS), mag / theta: (rows, dA + 2).  The scan starts from the carried total cphi —
// Theta[k][0] plus the increments of the frames [0, S) — or, at S = 0, from Theta[k][0] itself, and lane 0 stores the new total and the new last
// column into the other buffers of the pairs.  The wrapping sum is associative: the bits are the whole row's.
__global__ __launch_bounds__(256) void pv_scan_synth_stream_kernel(const float* __restrict__ mag, const uint32_t* __restrict__ theta,
                                                                   const float* __restrict__ cmag, const uint32_t* __restrict__ ctheta,
                                                                   const uint32_t* __restrict__ cphi, float* __restrict__ nmag,
                                                                   uint32_t* __restrict__ ntheta, uint32_t* __restrict__ nphi,
                                                                   float* __restrict__ spec, int rows, int nb, long long A, int dA, long long S,
                                                                   int dS, int o, int n) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;   // (whole waves leave: the shuffles of the scan always see 64 lanes)
    const int b = row / nb, k = row - b * nb;
    const PvWindowCols cols{mag + (long long)row * (dA + 2), theta + (long long)row * (dA + 2), cmag[row], ctheta[row], A, dA};
    float* re = spec + ((long long)b * 2 * nb + k) * dS;
    uint32_t carry;
    {
        float m0;
        uint32_t t0;
        cols(0, m0, t0);   // (S = 0 means A <= 1: column 0 is in the window or is the carried one)
        carry = S == 0 ? t0 : cphi[row];
    }
    pv_scan_row(cols, re, re + (long long)nb * dS, S, dS, carry, o, n);
    if ((threadIdx.x & 63) == 0) {
        nphi[row] = carry;
        nmag[row] = dA > 0 ? cols.mr[dA - 1] : cols.cm;
        ntheta[row] = dA > 0 ? cols.tr[dA - 1] : cols.ct;
    }
}

// pv_scan_synth_stream_kernel per entry: grid (groups of 4 bins, entries), so a wave is one (entry, k) row and the scan's shuffles see 64
// lanes of one row.  mag / theta: (rows, nb, T + 2) and spec (rows, 2 nb, ld), T / ld the launch's largest dA / dS; the entry's window has its
// own dA, and the columns [dS, ld) of its spec rows are written as zeros.  pol0 / pol1: the pool's two polar carries, each
// [mag (S, nb) | theta (S, nb) | phi (S, nb)] with `sn` = S nb; the entry reads half pbit and, if it analysed or synthesised, writes the other.
__global__ __launch_bounds__(256) void pv_scan_synth_pool_kernel(const float* __restrict__ mag, const uint32_t* __restrict__ theta,
                                                                 const float* pol0, const float* pol1, float* __restrict__ spec,
                                                                 const PvScanBlock tab, long long sn, int nb, int T, int ld, int o, int n, int k0) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nb) return;   // (whole waves leave: the shuffles of the scan always see 64 lanes)
    const PvScanEntry e = tab.e[blockIdx.y];
    const long long row = (long long)(k0 + blockIdx.y) * nb + k, cr = (long long)e.slot * nb + k;
    const float* cur = e.pbit ? pol1 : pol0;
    float* next = (float*)(e.pbit ? pol0 : pol1);
    float* re = spec + ((long long)(k0 + blockIdx.y) * 2 * nb + k) * ld;
    float* im = re + (long long)nb * ld;
    for (int c = e.dS + (threadIdx.x & 63); c < ld; c += 64) re[c] = 0.f, im[c] = 0.f;
    if (e.dA <= 0 && e.dS <= 0) return;
    const PvWindowCols cols{mag + row * (T + 2), theta + row * (T + 2), cur[cr], ((const uint32_t*)cur)[sn + cr], e.A, e.dA};
    uint32_t carry;
    {
        float m0;
        uint32_t t0;
        cols(0, m0, t0);   // (S = 0 means A <= 1: column 0 is in the window or is the carried one)
        carry = e.S == 0 ? t0 : ((const uint32_t*)cur)[2 * sn + cr];
    }
    pv_scan_row(cols, re, im, e.S, e.dS, carry, o, n);
    if ((threadIdx.x & 63) == 0) {
        ((uint32_t*)next)[2 * sn + cr] = carry;
        next[cr] = e.dA > 0 ? cols.mr[e.dA - 1] : cols.cm;
        ((uint32_t*)next)[sn + cr] = e.dA > 0 ? cols.tr[e.dA - 1] : cols.ct;
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

// The stream rule (include/fishvoc.h): after N samples, A analysis frames read no sample at or after N; S stretched frames have both their columns
// among those; Y stretched samples lie under frames that all exist and below Ls(N)
struct Ready {
    int64_t A = 0, S = 0, Y = 0;
};
Ready stream_ready(const Plan& p, int64_t N) {
    const int64_t F = p.N, h = p.hop;
    Ready r;
    r.A = N < F / 2 ? 0 : (N - F / 2) / h + 1;
    r.S = r.A < 2 ? 0 : ((r.A - 1) * p.o + p.n - 1) / p.n;
    r.Y = std::min(std::max<int64_t>(0, r.S * h - F / 2), (2 * N * p.o + p.n) / (2 * (int64_t)p.n));
    return r;
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
    bool invariant = false;      // fv_pv_set_batch_invariant: the whole-row calls run their two convs in batch-invariant mode, as the stream does
    ~fv_pitch_shift() {
        conv_layer_destroy(stft);
        conv_layer_destroy(idft);
        if (d_win2) (void)hipFree(d_win2);
        fv_resample_destroy(rs);
    }
    bool identity() const { return plan.orig_freq == cfg.sample_rate; }

    // The workspace of a launch over nA analysis frames, nS stretched frames, nY stretched samples and nR resampled ones per row:
    // [Yp (B, hop, nA + taps - 1) | Sp (B, 2 nb, nA) | Mg (B, nb, nA + 2) | Th (same, uint32) | S2 (B, 2 nb, nS) | Fr (B, N, nS) | St (B, nY) |
    //  Rs (B, nR)], each part rounded up to 64 floats.  A whole-row call: (T, T', Ls, 0); a stream: the most of one call (maxA, maxS, maxY, maxR).
    struct Parts {
        float *Yp, *Sp, *Mg, *S2, *Fr, *St, *Rs;
        uint32_t* Th;
        size_t elems;
    };
    Parts carve(float* ws, int B, size_t nA, size_t nS, size_t nY, size_t nR) const {
        auto up = [](size_t v) { return (v + 63) / 64 * 64; };
        const size_t b = (size_t)B;
        const size_t n_yp = up(b * plan.hop * (nA + taps - 1)), n_sp = up(b * 2 * nb * nA), n_mg = up(b * nb * (nA + 2));
        const size_t n_s2 = up(b * 2 * nb * nS), n_fr = up(b * plan.N * nS), n_st = up(b * nY), n_rs = up(b * nR);
        Parts w;
        w.Yp = ws, w.Sp = w.Yp + n_yp, w.Mg = w.Sp + n_sp, w.Th = (uint32_t*)(w.Mg + n_mg);
        w.S2 = w.Mg + 2 * n_mg, w.Fr = w.S2 + n_s2, w.St = w.Fr + n_fr, w.Rs = w.St + n_st;
        w.elems = n_yp + n_sp + 2 * n_mg + n_s2 + n_fr + n_st + n_rs;
        return w;
    }
    Parts carve(float* ws, int B, const Lengths& l) const { return carve(ws, B, (size_t)l.T, (size_t)l.Tout, (size_t)l.Ls, 0); }
};

// What every call refuses of its output rows (ny samples each, y_stride apart) against its input rows (nx each): the callers word the errors
enum class OutFault { none, null_out, short_stride, overlap };
static OutFault out_fault(const float* d_x, int64_t x_stride, int64_t nx, const float* d_y, int64_t y_stride, int64_t ny, int B) {
    if (ny <= 0) return OutFault::none;
    if (!d_y) return OutFault::null_out;
    if (y_stride < ny) return OutFault::short_stride;
    if (nx > 0 && d_x) {
        const float *x_end = d_x + (int64_t)(B - 1) * x_stride + nx, *y_end = d_y + (int64_t)(B - 1) * y_stride + ny;
        if (d_x < y_end && d_y < x_end) return OutFault::overlap;
    }
    return OutFault::none;
}

// the time stretch of `B` rows into rows of Ls samples at y (stride y_stride >= Ls)
static fv_status pv_stretch(fv_pitch_shift* p, const float* d_x, long long x_stride, float* y, long long y_stride, int B, long long L,
                            const Lengths& l, const fv_pitch_shift::Parts& w, hipStream_t s) {
    const Plan& pl = p->plan;
    const int hop = pl.hop, N = pl.N, nb = p->nb, T = (int)l.T, Tout = (int)l.Tout, TP = T + p->taps - 1;
    if (const fv_status st = launch_pv_frame(d_x, x_stride, w.Yp, B, L, hop, TP, N / 2, s)) return st;
    // (the default leaves the calling thread's mode alone: the calls keep the kernels, and the bits, they have always had)
    std::optional<AlgoScope> scope;
    if (p->invariant) scope.emplace(FV_CONV_ALGO_AUTO, true);
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
    const OutFault of = out_fault(d_x, x_row_stride, L, d_y, y_row_stride, out, batch);
    if (!d_x || of == OutFault::null_out) {
        set_error("%s: null %s", fn, d_x ? "d_y" : "d_x");
        return FV_ERR_INVALID;
    }
    if (x_row_stride < L || of == OutFault::short_stride) {
        set_error("%s: row strides (%lld, %lld) are shorter than the rows (L = %lld, %lld outputs)", fn, (long long)x_row_stride,
                  (long long)y_row_stride, (long long)L, (long long)out);
        return FV_ERR_INVALID;
    }
    if (of == OutFault::overlap) {
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


// The core's buffers carry the samples: buf[cur] holds [N - H, N), H = n_fft (frame A reads from A h - n_fft / 2 > N - n_fft on).  Polar and phase
// carries are one pair (pol[pcur]: |D| and Theta of column A - 1, Phi after the frames [0, S)), the synthesised frames [S - G, S) another (fr[fcur]).
// Each pair toggles when a launch has written its other half; the rule's counters A, S, Y follow from N alone.
struct fv_pv_stream : SampleStream {
    fv_pitch_shift* p = nullptr;
    fv_resample_stream* rs = nullptr;   // NULL for the pass-through
    long long Er = 0;                    // what rs has emitted
    int G = 0;                           // carried frames
    int maxA = 0, maxS = 0, maxY = 0, maxR = 0;   // the most frames / stretched frames / stretched samples / resampled samples of one call
    float* pol[2] = {nullptr, nullptr};  // one allocation: per half [mag (B, nb) | theta (B, nb) | phi (B, nb)]
    float* fr[2] = {nullptr, nullptr};   // one allocation: (B, n_fft, G) each
    int pcur = 0, fcur = 0;
    ~fv_pv_stream() {
        fv_resample_stream_destroy(rs);
        if (pol[0]) (void)hipFree(pol[0]);
        if (fr[0]) (void)hipFree(fr[0]);
    }
    float* mag(int h) const { return pol[h]; }
    uint32_t* theta(int h) const { return (uint32_t*)(pol[h] + (size_t)B * p->nb); }
    uint32_t* phi(int h) const { return (uint32_t*)(pol[h] + 2 * (size_t)B * p->nb); }

    fv_pitch_shift::Parts carve(float* ws) const { return p->carve(ws, B, (size_t)maxA, (size_t)maxS, (size_t)maxY, (size_t)maxR); }
    size_t ws_bytes() const { return p->identity() ? 0 : align_up(carve(nullptr).elems * sizeof(float), 256); }
};

static fv_status pv_stream_step(fv_pv_stream* st, const float* d_x, int64_t x_row_stride, int32_t c, bool flush, float* d_y, int64_t y_row_stride,
                                int64_t* emitted, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = flush ? "fv_pv_stream_flush" : "fv_pv_stream_push";
    if (emitted) *emitted = 0;
    if (!st || !emitted) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    long long N2;
    bool noop;
    if (const fv_status rs = st->admit(fn, "fv_pv_stream_reset", d_x, x_row_stride, c, flush, &N2, &noop)) return rs;
    if (noop) return FV_OK;
    if (N2 > kPvMaxLen) {
        set_error("%s: more than 2^30 samples in one utterance", fn);
        return FV_ERR_INVALID;
    }
    if (flush && st->N == 0) {   // an utterance without samples: nothing to analyse, nothing comes out
        st->commit(0, 0, true, false);
        return FV_OK;
    }
    fv_pitch_shift* p = st->p;
    const Plan& pl = p->plan;
    const int B = st->B;
    const long long N = st->N;
    hipStream_t s = (hipStream_t)stream;
    const auto check_out = [&](long long k) -> fv_status {
        const OutFault of = out_fault(d_x, x_row_stride, c, d_y, y_row_stride, k, B);
        if (of == OutFault::null_out || of == OutFault::short_stride) {
            set_error("%s: %s (this call emits %lld outputs per row)", fn, d_y ? "y_row_stride is shorter than the output" : "null output", k);
            return FV_ERR_INVALID;
        }
        if (of == OutFault::overlap) {
            set_error("%s: d_y overlaps d_x; the stream does not run in place", fn);
            return FV_ERR_INVALID;
        }
        return FV_OK;
    };
    if (p->identity()) {   // rate 1: a push hands its own samples back bit for bit, the flush has nothing left
        if (const fv_status rs = check_out(c)) return rs;
        if (c > 0)
            FV_HIP_CHECK(hipMemcpy2DAsync(d_y, (size_t)y_row_stride * 4, d_x, (size_t)x_row_stride * 4, (size_t)c * 4, (size_t)B,
                                          hipMemcpyDeviceToDevice, s));
        *emitted = c;
        st->commit(N2, st->E + c, flush, false);
        return FV_OK;
    }
    // what the call makes ready, all of it known before anything is enqueued
    const Ready r1 = stream_ready(pl, N);
    Ready r2 = stream_ready(pl, N2);
    if (flush) {
        const Lengths l = lengths_of(pl, N2);
        r2.A = l.T, r2.S = l.Tout, r2.Y = l.Ls;
    }
    const long long dA = r2.A - r1.A, dS = r2.S - r1.S, dY = r2.Y - r1.Y;
    const long long Er1 = dY > 0 ? std::max(st->Er, resample_emit_count(p->rs, r2.Y)) : st->Er;   // after the inner push
    const long long Er2 = flush ? fv_resample_output_length(p->rs, r2.Y) : Er1;                  // after the inner flush
    const long long E2 = flush ? N2 : std::min(Er2, N2);
    const long long k = E2 - st->E;
    if (!flush && Er2 > N2) {   // (not reached for lowpass_filter_width >= 1: an output's band ends after the samples its own index stands for)
        set_error("%s: internal: the resampler would emit output %lld after %lld input samples", fn, Er2 - 1, N2);
        return FV_ERR_INVALID;
    }
    if (dA < 0 || dS < 0 || dY < 0 || k < 0 || dA > st->maxA || dS > st->maxS || dY > st->maxY || Er2 - st->Er > st->maxR) {
        set_error("%s: internal: %lld frames, %lld stretched frames, %lld stretched samples, %lld resampled in one call; the stream was sized for "
                  "%d, %d, %d, %d", fn, dA, dS, dY, Er2 - st->Er, st->maxA, st->maxS, st->maxY, st->maxR);
        return FV_ERR_INVALID;
    }
    if (const fv_status rs = check_out(k)) return rs;
    const bool work = dA > 0 || dS > 0 || dY > 0 || k > 0;
    if (work && (!ws || ws_bytes < st->ws_bytes())) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_pv_stream_workspace_bytes)", fn, ws ? ws_bytes : (size_t)0, st->ws_bytes());
        return FV_ERR_INVALID;
    }
    const fv_pitch_shift::Parts w = st->carve((float*)ws);
    const int hop = pl.hop, F = pl.N, nb = p->nb, G = st->G, H = st->H;
    {
        const AlgoScope scope(FV_CONV_ALGO_AUTO, true);   // every column one fixed-order sum, whatever the launch holds
        if (dA > 0) {
            const int TP = (int)dA + p->taps - 1;
            if (const fv_status rs = launch_pv_frame_window(st->buf[st->cur], st->stride, d_x, x_row_stride, w.Yp, B, N, H, N2, r1.A, hop, TP, F / 2, s))
                return rs;
            ConvRun r;
            r.batch = B, r.t_in = TP, r.x = w.Yp, r.y = w.Sp;
            if (const fv_status rs = conv_layer_run(p->stft, r, s)) return rs;
        }
        if (dA > 0 || dS > 0) {
            const long long per = (long long)nb * (dA + 2);
            hipLaunchKernelGGL(pv_polar_kernel, dim3((unsigned)((per + 255) / 256), B), dim3(256), 0, s, w.Sp, w.Mg, w.Th, nb, (int)dA);
            FV_HIP_CHECK(hipGetLastError());
            const int rows = B * nb, pc = st->pcur;
            hipLaunchKernelGGL(pv_scan_synth_stream_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w.Mg, w.Th, st->mag(pc), st->theta(pc),
                               st->phi(pc), st->mag(pc ^ 1), st->theta(pc ^ 1), st->phi(pc ^ 1), w.S2, rows, nb, (long long)r1.A, (int)dA,
                               (long long)r1.S, (int)dS, pl.o, pl.n);
            FV_HIP_CHECK(hipGetLastError());
            set_last_kernel("pv_scan_synth_stream_kernel");
            st->pcur ^= 1;
        }
        if (!flush)
            if (const fv_status rs = launch_sample_carry(st->buf[st->cur], st->buf[st->cur ^ 1], d_x, st->stride, x_row_stride, B, N, N2 - H, N - H,
                                                         H, s))
                return rs;
        if (dS > 0) {
            ConvRun r;
            r.batch = B, r.t_in = (int)dS, r.x = w.S2, r.y = w.Fr;
            if (const fv_status rs = conv_layer_run(p->idft, r, s)) return rs;
        }
    }
    if (dY > 0) {
        if (const fv_status rs = launch_istft_ola_window(w.Fr, st->fr[st->fcur], p->d_win2, w.St, B, F, hop, F / 2, G, r1.S, (int)dS, r2.S, r1.Y,
                                                         r2.Y, s))
            return rs;
    }
    if (dS > 0) {
        if (const fv_status rs = launch_pv_frame_carry(w.Fr, st->fr[st->fcur], st->fr[st->fcur ^ 1], B, F, G, r1.S, (int)dS, s)) return rs;
        st->fcur ^= 1;
    }
    // the resampler: a push writes the caller's rows; the flush goes through Rs, because its last outputs may lie past L
    float* dst = flush ? w.Rs : d_y;
    const long long dst_stride = flush ? st->maxR : y_row_stride;
    int64_t got = 0;
    if (dY > 0) {
        if (const fv_status rs = fv_resample_stream_push(st->rs, w.St, dY, (int32_t)dY, dst, dst_stride, &got, stream)) return rs;
        if (got != Er1 - st->Er) {
            set_error("%s: internal: the resampler emitted %lld outputs where the rule says %lld", fn, (long long)got, Er1 - st->Er);
            return FV_ERR_INVALID;
        }
    }
    if (flush) {
        int64_t rest = 0;
        if (const fv_status rs = fv_resample_stream_flush(st->rs, w.Rs + got, dst_stride, &rest, stream)) return rs;
        const long long keep = std::min(Er2, N2) - st->E;   // (Ls = 0: nothing came out, the rows end in zeros)
        if (keep > 0)
            FV_HIP_CHECK(hipMemcpy2DAsync(d_y, (size_t)y_row_stride * 4, w.Rs, (size_t)dst_stride * 4, (size_t)keep * 4, (size_t)B,
                                          hipMemcpyDeviceToDevice, s));
        if (keep < k) {
            hipLaunchKernelGGL(pv_zero_tail_kernel, dim3((unsigned)((k - keep + 255) / 256), B), dim3(256), 0, s, d_y, (long long)y_row_stride,
                               (long long)std::max(keep, 0LL), (long long)k);
            FV_HIP_CHECK(hipGetLastError());
        }
    }
    *emitted = k;
    st->Er = Er2;
    st->commit(N2, E2, flush, !flush);
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------
// The pool (fv_pvpool_*): the sample pool's counters and sample carry (sample_pool.h) around the stream's chain, every stage behind a per-entry
// fetch.  Per slot two more ping-pong pairs with a bit each: the polar carry (pbit flips when the step analysed or synthesised for the slot)
// and the last G frames (fbit flips when it synthesised).  The resampler stage is an inner fv_respool on the shifter's own resampler.
// ---------------------------------------------------------------------------------------------
// The host rule of one pool: everything fv_pvpool_plan needs.  rs: the resampler's rule (NULL for the identity shift).
struct PvPoolRule {
    Plan pl;
    const fv_resample* rs = nullptr;
    int max_chunk = 0;
    long long maxA = 0, maxS = 0, maxY = 0, maxR = 0, max_out = 0;
    bool identity() const { return rs == nullptr; }
    long long emitted_after(long long N) const {   // E(N) between flushes
        return std::min(resample_emit_count(rs, stream_ready(pl, N).Y), N);
    }
};

// The bounds of one step, for a push of max_chunk = c samples that also flushes, from any state N (N2 = N + c):
//   dA = T(N2) - A(N) <= (c + F / 2) / h + 1: T = 1 + N2 / h, and A(N) = (N - F / 2) / h + 1 (0 below F / 2, where T <= 1 + (c + F / 2 - 1) / h)
//   dS = T'(N2) - S(N) <= ceil((dA + 1) o / n) + 1: T' = ceil(T o / n), S = ceil((A - 1) o / n) (0 for A < 2, which is that formula's value or above)
//   dY = Ls(N2) - Y(N) < dS h + F where Y = max(0, S h - F / 2) (Ls < T' h + F / 2), and <= c o / n + 1 where Y = Ls(N)
//   the resampler: an inner pool item of dY <= maxY samples that flushes, fv_respool_max_outputs of that pool
//   outputs: N2 - E(N) = c + (N - E(N)).  N - E(N) grows by one per sample and falls only where A(N) steps, at N = F / 2 + a h, so its largest
//   value stands at some N_a = F / 2 + a h - 1.  A step of a by n moves S by o, Y by o h and the resampler's count by n h = the step of N: past
//   the start-up (Y beyond the resampler's clamp at 0) N - E(N) has period n in a, and in the start-up every clamp (A, S, Y, the count at 0)
//   only raises E.  So the bound is the largest N_a - E(N_a) over n consecutive a past the start-up: exact, some state attains it.
static void pvpool_bounds(PvPoolRule& r) {
    const Plan& pl = r.pl;
    const long long c = r.max_chunk;
    if (r.identity()) {
        r.max_out = c;
        return;
    }
    const long long F = pl.N, h = pl.hop, o = pl.o, n = pl.n;
    r.maxA = (c + F / 2) / h + 2;
    r.maxS = ((r.maxA + 1) * o + n - 1) / n + 2;
    r.maxY = std::max(r.maxS * h + F, (c * o + n - 1) / n + 2);
    r.maxR = r.maxY <= (1 << 28) ? resample_pool_max_outputs(r.rs, (int)r.maxY) : 0;
    const long long need = 4 * o + 2LL * resample_band_taps(r.rs);
    long long a0 = (((need + F) * n + o - 1) / o + 2 * F + 2 * h) / h + 2;
    while (stream_ready(pl, F / 2 + a0 * h - 1).Y < need) a0 += n;
    long long lag = 0;
    for (long long a = a0; a < a0 + n; ++a) {
        const long long N = F / 2 + a * h - 1;
        lag = std::max(lag, N - r.emitted_after(N));
    }
    r.max_out = c + lag;
}

// What one item does in a step; all of it host arithmetic from the slot's N and E
struct PvPoolMove {
    long long N = 0, N2 = 0, E2 = 0, k = 0, keep = 0;   // keep: outputs that come from the resampler, the rest of k are zeros
    Ready r1, r2;
    long long dA = 0, dS = 0, dY = 0, Er = 0, Er2 = 0;  // the inner pool's emitted count before and after
    bool active = false;                                // the item runs the chain (a row of the step's tensors)
};

// The pool's own plan after sample_pool_admit: the 2^30 limit and the step's bounds, each refusal naming item and session.  Changes nothing.
static fv_status pvpool_moves(const PvPoolRule& r, const char* fn, const int64_t* received, const int64_t* emitted, const fv_wavpool_item* items,
                              int count, const long long* N2, std::vector<PvPoolMove>& mv) {
    mv.assign((size_t)std::max(count, 0), PvPoolMove());
    for (int i = 0; i < count; ++i) {
        const int s = items[i].session;
        const bool flush = items[i].flush != 0;
        PvPoolMove& m = mv[(size_t)i];
        m.N = received[s], m.N2 = N2[i];
        const long long E = emitted[s];
        if (m.N2 > kPvMaxLen) {
            set_error("%s: item %d takes session %d past 2^30 samples in one utterance (%lld + %d)", fn, i, s, m.N, items[i].samples);
            return FV_ERR_INVALID;
        }
        if (r.identity()) {   // rate 1: the item's own samples
            m.E2 = E + items[i].samples, m.k = m.keep = items[i].samples;
            continue;
        }
        if (flush && m.N2 == 0) continue;   // an utterance without samples: nothing to analyse, nothing comes out
        m.r1 = stream_ready(r.pl, m.N), m.r2 = stream_ready(r.pl, m.N2);
        if (flush) {
            const Lengths l = lengths_of(r.pl, m.N2);
            m.r2.A = l.T, m.r2.S = l.Tout, m.r2.Y = l.Ls;
        }
        m.dA = m.r2.A - m.r1.A, m.dS = m.r2.S - m.r1.S, m.dY = m.r2.Y - m.r1.Y;
        m.Er = resample_emit_count(r.rs, m.r1.Y);
        m.Er2 = flush ? std::max(m.Er, (long long)fv_resample_output_length(r.rs, m.r2.Y)) : std::max(m.Er, resample_emit_count(r.rs, m.r2.Y));
        if (!flush && m.Er2 > m.N2) {   // (not reached for lowpass_filter_width >= 1: an output's band ends after the samples its own index stands for)
            set_error("%s: internal: item %d (session %d): the resampler would emit output %lld after %lld input samples", fn, i, s, m.Er2 - 1, m.N2);
            return FV_ERR_INVALID;
        }
        m.E2 = flush ? m.N2 : std::max<long long>(E, std::min(m.Er2, m.N2));
        m.k = m.E2 - E;
        m.keep = std::max(0LL, std::min(m.k, std::min(m.Er2, m.N2) - E));
        if (m.dA < 0 || m.dS < 0 || m.dY < 0 || m.k < 0 || E != std::min(m.Er, m.N) || m.dA > r.maxA || m.dS > r.maxS || m.dY > r.maxY ||
            m.Er2 - m.Er > r.maxR || m.k > r.max_out) {
            set_error("%s: internal: item %d (session %d): %lld frames, %lld stretched frames, %lld stretched samples, %lld resampled, %lld outputs in "
                      "one step from N = %lld, E = %lld; the pool was sized for %lld, %lld, %lld, %lld, %lld", fn, i, s, m.dA, m.dS, m.dY,
                      m.Er2 - m.Er, m.k, m.N, (long long)E, r.maxA, r.maxS, r.maxY, r.maxR, r.max_out);
            return FV_ERR_INVALID;
        }
        m.active = flush || m.dA > 0 || m.dS > 0 || m.dY > 0;
    }
    return FV_OK;
}

// the pool's own range check, once the bounds of `max_chunk` are known: what a step's tensors and the inner resample pool can hold
static fv_status pvpool_range(const char* fn, int max_chunk, const PvPoolRule& r) {
    if (!r.identity() && (r.maxY > (1 << 28) || r.maxR > (1LL << 30) || (long long)r.pl.N * r.maxS >= (1LL << 31))) {
        set_error("%s: max_chunk = %d gives %lld stretched frames of %d samples in one step, more than 2^31 elements per row or 2^28 stretched "
                  "samples; push smaller chunks", fn, max_chunk, r.maxS, r.pl.N);
        return FV_ERR_UNSUPPORTED;
    }
    return FV_OK;
}

struct fv_pvpool : SamplePool {
    fv_pitch_shift* p = nullptr;
    fv_respool* rs = nullptr;            // NULL for the pass-through
    PvPoolRule rule;
    int G = 0;
    float* pol[2] = {nullptr, nullptr};  // one allocation: per half [mag (S, nb) | theta (S, nb) | phi (S, nb)]
    float* fr[2] = {nullptr, nullptr};   // one allocation: (S, n_fft, G) each
    std::vector<unsigned char> pbit, fbit;
    ~fv_pvpool() {
        fv_respool_destroy(rs);
        if (pol[0]) (void)hipFree(pol[0]);
        if (fr[0]) (void)hipFree(fr[0]);
    }
    fv_pitch_shift::Parts carve(float* ws) const {
        return p->carve(ws, S, (size_t)rule.maxA, (size_t)rule.maxS, (size_t)rule.maxY, (size_t)rule.maxR);
    }
    size_t ws_bytes() const { return rule.identity() ? 0 : align_up(carve(nullptr).elems * sizeof(float), 256); }
};

extern "C" {

FV_API fv_status fv_pvpool_create(fv_pitch_shift* p, int32_t sessions, int32_t max_chunk, fv_pvpool** out) {
    const char* fn = "fv_pvpool_create";
    if (out) *out = nullptr;
    if (!p || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (const fv_status rs = sample_pool_range(fn, sessions, max_chunk)) return rs;
    std::unique_ptr<fv_pvpool> q(new fv_pvpool());
    q->p = p;
    q->rule.pl = p->plan, q->rule.rs = p->identity() ? nullptr : p->rs, q->rule.max_chunk = max_chunk;
    pvpool_bounds(q->rule);
    if (const fv_status rs = pvpool_range(fn, max_chunk, q->rule)) return rs;
    q->pbit.assign((size_t)sessions, 0), q->fbit.assign((size_t)sessions, 0);
    if (p->identity()) {   // the pass-through carries nothing
        q->init(sessions, max_chunk, 0);
        *out = q.release();
        return FV_OK;
    }
    const int F = p->plan.N;
    if (const fv_status rs = q->create(fn, sessions, max_chunk, F)) return rs;
    q->G = F / p->plan.hop;   // (fv_pv_stream_create's note on G)
    const size_t pol = 3 * (size_t)sessions * p->nb, frm = (size_t)sessions * F * q->G;
    FV_HIP_CHECK(hipMalloc((void**)&q->pol[0], 2 * pol * sizeof(float)));
    q->pol[1] = q->pol[0] + pol;
    FV_HIP_CHECK(hipMemset(q->pol[0], 0, 2 * pol * sizeof(float)));
    FV_HIP_CHECK(hipMalloc((void**)&q->fr[0], 2 * frm * sizeof(float)));
    q->fr[1] = q->fr[0] + frm;
    FV_HIP_CHECK(hipMemset(q->fr[0], 0, 2 * frm * sizeof(float)));
    if (const fv_status rs = fv_respool_create(p->rs, sessions, (int32_t)q->rule.maxY, &q->rs)) return rs;
    *out = q.release();
    return FV_OK;
}

FV_API size_t fv_pvpool_workspace_bytes(const fv_pvpool* p) { return p ? p->ws_bytes() : 0; }

FV_API int64_t fv_pvpool_max_outputs(const fv_pvpool* p) { return p ? p->rule.max_out : 0; }

FV_API int64_t fv_pvpool_received(const fv_pvpool* p, int32_t s) { return sample_pool_received(p, s); }

FV_API int64_t fv_pvpool_emitted(const fv_pvpool* p, int32_t s) { return sample_pool_emitted(p, s); }

FV_API int64_t fv_pvpool_pending(const fv_pvpool* p, int32_t s) { return p && s >= 0 && s < p->S ? p->N[(size_t)s] - p->E[(size_t)s] : 0; }

struct RuleHold {
    fv_resample* r = nullptr;
    ~RuleHold() { fv_resample_destroy(r); }
};
// the host rule of a config: the plan, the resampler's rule (owned by `hold`) and the bounds
static fv_status pvpool_rule(const fv_pitch_shift_config* cfg, const char* fn, int max_chunk, PvPoolRule& r, RuleHold& hold) {
    if (const fv_status st = make_plan(cfg, fn, r.pl)) return st;
    r.max_chunk = max_chunk;
    const fv_resample_config rc = resample_config(*cfg, r.pl);
    fv_resample* rs = nullptr;
    if (const fv_status st = resample_rule_create(&rc, fn, &rs)) return st;
    hold.r = rs;
    r.rs = r.pl.orig_freq == cfg->sample_rate ? nullptr : rs;
    pvpool_bounds(r);
    return FV_OK;
}

FV_API fv_status fv_pvpool_bounds(const fv_pitch_shift_config* cfg, int32_t max_chunk, int64_t* bounds) {
    const char* fn = "fv_pvpool_bounds";
    if (!bounds) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = sample_pool_range(fn, 1, max_chunk)) return st;
    PvPoolRule r;
    RuleHold hold;
    if (const fv_status st = pvpool_rule(cfg, fn, max_chunk, r, hold)) return st;
    if (const fv_status st = pvpool_range(fn, max_chunk, r)) return st;
    bounds[0] = r.maxA, bounds[1] = r.maxS, bounds[2] = r.maxY, bounds[3] = r.maxR, bounds[4] = r.max_out;
    return FV_OK;
}

FV_API int64_t fv_pvpool_plan(const fv_pitch_shift_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received,
                              const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                              int64_t* outputs_out) {
    const char* fn = "fv_pvpool_plan";
    if (const fv_status st = sample_pool_range(fn, sessions, max_chunk)) return st;
    PvPoolRule r;
    RuleHold hold;
    if (const fv_status st = pvpool_rule(cfg, fn, max_chunk, r, hold)) return st;
    if (const fv_status st = pvpool_range(fn, max_chunk, r)) return st;
    return sample_pool_plan(fn, sessions, max_chunk, received, emitted, flushed, items, count, outputs_out,
                            [&](const long long* N2, long long* E2) -> fv_status {
                                std::vector<PvPoolMove> mv;
                                if (const fv_status rs = pvpool_moves(r, fn, received, emitted, items, count, N2, mv)) return rs;
                                for (int i = 0; i < count; ++i) E2[i] = emitted[items[i].session] + mv[(size_t)i].k;   // the counts are the moves' k
                                return FV_OK;
                            });
}

FV_API fv_status fv_pvpool_step(fv_pvpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                float* d_out, int64_t out_stride, int32_t out_cols, int64_t* outputs_out, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    const char* fn = "fv_pvpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    for (int i = 0; outputs_out && i < count; ++i) outputs_out[i] = 0;
    // the whole step on the host first: the core's refusals, the pool's own plan, the inner pool's state, the output and the workspace
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status rs = p->admit(fn, "fv_pvpool_reset", items, count, d_chunks, chunk_stride, N2.data())) return rs;
    std::vector<PvPoolMove> mv;
    if (const fv_status rs = pvpool_moves(p->rule, fn, p->N.data(), p->E.data(), items, count, N2.data(), mv)) return rs;
    int nact = 0;
    for (int i = 0; i < count; ++i) {
        const PvPoolMove& m = mv[(size_t)i];
        E2[(size_t)i] = m.E2;
        if (!m.active) continue;
        ++nact;
        const int s = items[i].session;
        if (fv_respool_received(p->rs, s) != m.r1.Y || fv_respool_emitted(p->rs, s) != m.Er) {
            set_error("%s: internal: item %d (session %d): the inner resample pool stands at (%lld, %lld) where the rule says (%lld, %lld)", fn, i, s,
                      (long long)fv_respool_received(p->rs, s), (long long)fv_respool_emitted(p->rs, s), m.r1.Y, m.Er);
            return FV_ERR_INVALID;
        }
    }
    if (const fv_status rs = sample_pool_output(fn, "outputs", items, count, p->E.data(), E2.data(), 1, d_out != nullptr, out_stride, out_cols))
        return rs;
    if (nact > 0 && (!d_workspace || workspace_bytes < p->ws_bytes())) {
        int a = 0;
        while (!mv[(size_t)a].active) ++a;
        set_error("%s: workspace too small (%zu < %zu bytes, fv_pvpool_workspace_bytes) for item %d (session %d)", fn,
                  d_workspace ? workspace_bytes : (size_t)0, p->ws_bytes(), a, items[a].session);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const auto done = [&]() {
        for (int i = 0; outputs_out && i < count; ++i) outputs_out[i] = mv[(size_t)i].k;
        for (int i = 0; i < count; ++i) {
            const PvPoolMove& m = mv[(size_t)i];
            const size_t sl = (size_t)items[i].session;
            if (m.dA > 0 || m.dS > 0) p->pbit[sl] ^= 1;
            if (m.dS > 0) p->fbit[sl] ^= 1;
        }
        p->commit(items, count, N2.data(), E2.data());
        return FV_OK;
    };
    std::vector<PoolCropEntry> crop((size_t)count);
    if (p->rule.identity()) {   // rate 1: every item's samples back bit for bit, zeros behind them
        for (int i = 0; i < count; ++i) crop[(size_t)i] = PoolCropEntry{i, items[i].samples > 0 ? i : -1, 0, items[i].samples};
        if (d_out && out_cols > 0)
            if (const fv_status rs = launch_pool_crop(d_chunks, d_out, crop.data(), count, 1, chunk_stride, out_cols, 1, s, out_stride)) return rs;
        return done();
    }
    // the step's tables: one row of the workspace tensors per active item, in item order
    const fv_pitch_shift* ps = p->p;
    const Plan& pl = ps->plan;
    const int hop = pl.hop, F = pl.N, nb = ps->nb, H = p->H;
    std::vector<SamplePoolEntry> win, carry;
    std::vector<PvScanEntry> scan;
    std::vector<PvOlaEntry> ola;
    std::vector<fv_wavpool_item> inner;
    long long dA_max = 0, dS_max = 0, ki_max = 0;
    bool any_scan = false;
    for (int i = 0; i < count; ++i) {
        const PvPoolMove& m = mv[(size_t)i];
        const int sl = items[i].session;
        const SamplePoolEntry en{i, sl, (int)p->cur[(size_t)sl], (int)m.dA, m.N - H, m.N, items[i].flush ? m.N2 : -1, m.N2, m.r1.A};
        if (items[i].samples > 0) carry.push_back(en);
        crop[(size_t)i] = PoolCropEntry{i, m.active && m.keep > 0 ? (int)win.size() : -1, 0, m.keep};
        if (!m.active) continue;
        win.push_back(en);
        scan.push_back(PvScanEntry{sl, (int)p->pbit[(size_t)sl], (int)m.dA, (int)m.dS, m.r1.A, m.r1.S});
        ola.push_back(PvOlaEntry{sl, (int)p->fbit[(size_t)sl], (int)m.dS, 0, m.r1.S, m.r2.S, m.r1.Y, m.r2.Y});
        inner.push_back(fv_wavpool_item{sl, (int32_t)m.dY, items[i].flush});
        dA_max = std::max(dA_max, m.dA), dS_max = std::max(dS_max, m.dS), ki_max = std::max(ki_max, m.Er2 - m.Er);
        any_scan = any_scan || m.dA > 0 || m.dS > 0;
    }
    if (nact > 0) {
        const fv_pitch_shift::Parts w = p->carve((float*)d_workspace);
        const int T = (int)dA_max, ld = (int)dS_max;
        {
            const AlgoScope scope(FV_CONV_ALGO_AUTO, true);   // every column one fixed-order sum, whatever the launch holds
            if (T > 0) {
                const int TP = T + ps->taps - 1;
                if (const fv_status rs = launch_pv_frame_pool_window(p->buf[0], p->buf[1], H, d_chunks, chunk_stride, win.data(), nact, w.Yp, hop, TP,
                                                                     ps->taps, F / 2, s))
                    return rs;
                ConvRun r;
                r.batch = nact, r.t_in = TP, r.x = w.Yp, r.y = w.Sp;
                if (const fv_status rs = conv_layer_run(ps->stft, r, s)) return rs;
            }
            if (any_scan) {
                const long long per = (long long)nb * (T + 2), sn = (long long)p->S * nb;
                const fv_status rs = for_each_launch_table<PvScanBlock>(nact, scan.data(), [&](const PvScanBlock& blk, int k0, int nz) {
                    hipLaunchKernelGGL(pv_polar_pool_kernel, dim3((unsigned)((per + 255) / 256), nz), dim3(256), 0, s, w.Sp, w.Mg, w.Th, blk, nb, T, k0);
                    hipLaunchKernelGGL(pv_scan_synth_pool_kernel, dim3((nb + 3) / 4, nz), dim3(256), 0, s, w.Mg, w.Th, p->pol[0], p->pol[1], w.S2, blk,
                                       sn, nb, T, ld, pl.o, pl.n, k0);
                    return FV_OK;
                });
                if (rs) return rs;
                set_last_kernel("pv_scan_synth_pool_kernel");
            }
            if (ld > 0) {
                ConvRun r;
                r.batch = nact, r.t_in = ld, r.x = w.S2, r.y = w.Fr;
                if (const fv_status rs = conv_layer_run(ps->idft, r, s)) return rs;
            }
        }
        if (const fv_status rs = launch_pv_pool_ola(w.Fr, p->fr[0], p->fr[1], ps->d_win2, w.St, ola.data(), nact, F, hop, F / 2, p->G, std::max(ld, 1),
                                                    p->rule.maxY, s))
            return rs;
        // the resampler: the inner pool takes this step's stretched samples and writes Rs; a flush's surplus past N' is cut by the crop below
        if (const fv_status rs = fv_respool_step(p->rs, inner.data(), nact, w.St, p->rule.maxY, w.Rs, p->rule.maxR, (int32_t)ki_max, nullptr, stream))
            return rs;
        for (int i = 0; i < count; ++i)   // an item flushed at N' > 0 leaves its inner slot flushed too; fv_pvpool_reset resets both
            if (mv[(size_t)i].active && fv_respool_emitted(p->rs, items[i].session) != mv[(size_t)i].Er2) {
                set_error("%s: internal: the inner resample pool emitted up to %lld for session %d where the rule says %lld", fn,
                          (long long)fv_respool_emitted(p->rs, items[i].session), items[i].session, mv[(size_t)i].Er2);
                return FV_ERR_INVALID;
            }
    }
    if (const fv_status rs = launch_sample_pool_carry(p->buf[0], p->buf[1], H, d_chunks, chunk_stride, carry.data(), (int)carry.size(), s)) return rs;
    if (d_out && out_cols > 0)
        if (const fv_status rs = launch_pool_crop(nact > 0 ? p->carve((float*)d_workspace).Rs : nullptr, d_out, crop.data(), count, 1, p->rule.maxR,
                                                  out_cols, 1, s, out_stride))
            return rs;
    return done();
}

FV_API fv_status fv_pvpool_reset(fv_pvpool* p, int32_t session) {
    if (const fv_status rs = sample_pool_reset(p, "fv_pvpool_reset", session)) return rs;
    return p->rs ? fv_respool_reset(p->rs, session) : FV_OK;
}

FV_API void fv_pvpool_destroy(fv_pvpool* p) { delete p; }

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

FV_API fv_status fv_pv_stream_ready(const fv_pitch_shift_config* cfg, int64_t N, int64_t* frames, int64_t* stretched_frames,
                                    int64_t* stretched_samples) {
    Plan p;
    if (const fv_status st = make_plan(cfg, "fv_pv_stream_ready", p)) return st;
    if (N < 0 || N > kPvMaxLen) {
        set_error("fv_pv_stream_ready: N = %lld must lie in [0, 2^30]", (long long)N);
        return FV_ERR_INVALID;
    }
    const Ready r = stream_ready(p, N);
    if (frames) *frames = r.A;
    if (stretched_frames) *stretched_frames = r.S;
    if (stretched_samples) *stretched_samples = r.Y;
    return FV_OK;
}

FV_API fv_status fv_pv_set_batch_invariant(fv_pitch_shift* p, int32_t enable) {
    if (!p) {
        set_error("fv_pv_set_batch_invariant: null pitch shifter");
        return FV_ERR_INVALID;
    }
    p->invariant = enable != 0;
    return FV_OK;
}

FV_API fv_status fv_pv_stream_create(fv_pitch_shift* p, int32_t batch, int32_t max_chunk, fv_pv_stream** out) {
    const char* fn = "fv_pv_stream_create";
    if (!p || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_pv_stream> st(new fv_pv_stream());
    st->p = p;
    if (p->identity()) {   // the pass-through carries nothing
        if (const fv_status rs = st->create(fn, batch, max_chunk, 0, 1)) return rs;
        *out = st.release();
        return FV_OK;
    }
    const Plan& pl = p->plan;
    const long long F = pl.N, h = pl.hop, o = pl.o, n = pl.n;
    // One call's most: a push analyses at most c / h + 1 frames, the flush T - A <= F / (2 h) + 1; S moves by at most (dA + 1) o / n + 1; Y by at most
    // dS h, and up to Ls < T' h + F / 2 at the flush; the resampler then still owes the outputs whose bands had not ended
    const int kp = resample_band_taps(p->rs);
    const long long maxA = std::max<long long>((long long)max_chunk / h + 1, F / (2 * h) + 2);
    const long long maxS = ((maxA + 1) * o + n - 1) / n + 2;
    const long long maxY = maxS * h + F;
    const long long maxR = ((maxY + 2LL * kp + 2) * n + o - 1) / o + 8;
    if (batch >= 1 && max_chunk >= 1 && (maxY > (1 << 28) || maxR > (1LL << 30) || F * maxS >= (1LL << 31))) {
        set_error("%s: max_chunk = %d gives %lld stretched frames of %lld samples in one push, more than 2^31 elements per row or 2^28 stretched "
                  "samples; push smaller chunks", fn, max_chunk, maxS, F);
        return FV_ERR_UNSUPPORTED;
    }
    if (const fv_status rs = st->create(fn, batch, max_chunk, (int)F, F)) return rs;
    st->G = (int)(F / h);   // one more than the overlap: where Ls(N) binds (h = F only), Y lies up to h samples below S h - F / 2
    st->maxA = (int)maxA, st->maxS = (int)maxS, st->maxY = (int)maxY, st->maxR = (int)maxR;
    const size_t pol = 3 * (size_t)batch * p->nb, frm = (size_t)batch * F * st->G;
    FV_HIP_CHECK(hipMalloc((void**)&st->pol[0], 2 * pol * sizeof(float)));
    st->pol[1] = st->pol[0] + pol;
    FV_HIP_CHECK(hipMemset(st->pol[0], 0, 2 * pol * sizeof(float)));
    FV_HIP_CHECK(hipMalloc((void**)&st->fr[0], 2 * frm * sizeof(float)));
    st->fr[1] = st->fr[0] + frm;
    FV_HIP_CHECK(hipMemset(st->fr[0], 0, 2 * frm * sizeof(float)));
    if (const fv_status rs = fv_resample_stream_create(p->rs, batch, (int32_t)maxY, &st->rs)) return rs;
    *out = st.release();
    return FV_OK;
}

FV_API size_t fv_pv_stream_workspace_bytes(const fv_pv_stream* s) { return s ? s->ws_bytes() : 0; }

FV_API int64_t fv_pv_stream_pending(const fv_pv_stream* s) { return s ? s->N - s->E : 0; }

FV_API fv_status fv_pv_stream_push(fv_pv_stream* s, const float* d_x, int64_t x_row_stride, int32_t c, float* d_y, int64_t y_row_stride,
                                   int64_t* emitted, void* d_workspace, size_t workspace_bytes, void* stream) {
    return pv_stream_step(s, d_x, x_row_stride, c, false, d_y, y_row_stride, emitted, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_pv_stream_flush(fv_pv_stream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
    return pv_stream_step(s, nullptr, 0, 0, true, d_y, y_row_stride, emitted, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_pv_stream_reset(fv_pv_stream* s) {
    if (!s) {
        set_error("fv_pv_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    if (s->rs)
        if (const fv_status rs = fv_resample_stream_reset(s->rs)) return rs;
    s->reset();
    s->Er = 0;
    return FV_OK;
}

FV_API void fv_pv_stream_destroy(fv_pv_stream* s) { delete s; }

}  // extern "C"
