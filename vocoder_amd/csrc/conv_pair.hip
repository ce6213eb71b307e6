// Host side of the fused ResBlock (c1, c2) pairs: which kernel family takes a pair, its launch parameters, the launch bookkeeping.
#include <algorithm>
#include <cstring>

#include "fv_internal.h"
#include "pair_f16x3_params.h"

namespace fv {

// What every fused-pair launch checks and records.  A launcher that declined: the refused LDS opt-in keeps its own error text, otherwise "no <what>
// for (C, k, d)".  Then the kernel's name "<family><k d C>" for fv_last_kernel (set_last_kernel copies it) and — under fv_profile_begin — one profiler
// row: grid = batch x tiles of tt output columns, the ALGORITHMIC (direct-sum) MACs of the two convs, `tensors` tensors of (C, t) moved per item (+ the
// accumulate operand) and the two layers' folded weights once.
static fv_status finish_pair_launch(bool launched, const char* family, const char* what, int tt, double tensors, const ConvLayer& c1, int t,
                                    int batch, int out_mode, hipStream_t stream, int prof_idx) {
    const int C = c1.c_in;
    if (!launched) {
        if (dynamic_lds_refused()) return FV_ERR_HIP;   // error text already names the refused attribute
        set_error("conv_pair_run: no %s for (C=%d k=%d d=%d)", what, C, c1.k, c1.dil);
        return FV_ERR_UNSUPPORTED;
    }
    char name[96];
    std::snprintf(name, sizeof(name), "%s<k=%d d=%d C=%d>", family, c1.k, c1.dil, C);
    set_last_kernel(name);
    if (prof_idx >= 0) {
        char lbl[128];
        std::snprintf(lbl, sizeof(lbl), "%s grid=%d", name, batch * ((t + tt - 1) / tt));
        const double macs = 2.0 * C * C * c1.k * (double)t * batch;
        const double elems = (out_mode == OUT_ACCUM ? tensors + 1.0 : tensors) * C * (double)t * batch;
        prof_end(stream, prof_idx, lbl, 2.0 * macs, elems * 4.0 + 2.0 * C * C * c1.k * 4.0);
    }
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
}

// the fields every fp32 pair kernel reads; w1 / w2: the two layers' weights in the family's fragment order
static PairParams pair_params(const ConvLayer& c1, const ConvLayer& c2, const float4* w1, const float4* w2, const float* x, float* y, int t,
                              int out_mode, float out_scale) {
    PairParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x;
    p.y = y;
    p.w1 = w1;
    p.w2 = w2;
    p.b1 = c1.d_bias;
    p.b2 = c2.d_bias;
    p.T = t;
    p.out_mode = out_mode;
    p.out_scale = out_scale;
    return p;
}

// ... and the f16x3 pair kernels'; w1h / w2h: the layers' d_wph (nch16 = C / 16) or d_wph16 (nch16 = 1) planes
static PairF16Params pair_f16_params(const ConvLayer& c1, const ConvLayer& c2, const void* w1h, const void* w2h, int nch16, const float* x, float* y,
                                     int t, int out_mode, float out_scale) {
    PairF16Params p;
    std::memset(&p, 0, sizeof(p));
    p.x = x;
    p.y = y;
    p.w1h = w1h;
    p.w2h = w2h;
    p.b1 = c1.d_bias;
    p.b2 = c2.d_bias;
    p.s1 = 1.0f / c1.w_scale;
    p.s2 = 1.0f / c2.w_scale;
    p.T = t;
    p.nch16 = nch16;
    p.out_mode = out_mode;
    p.out_scale = out_scale;
    return p;
}

// f16x3 precision mode: wide (C = 128 / 64) SiLU pairs on the fused split-fp16 kernel (pair_f16x3_impl.h)
bool pair_f16x3_supported(const ConvLayer& c1, const ConvLayer& c2) {
    const int C = c1.c_in;
    return c1.precision == FV_PRECISION_F16X3 && c2.precision == FV_PRECISION_F16X3 && c1.d_wph && c2.d_wph &&
           !c1.transposed && !c2.transposed && (C == 256 || C == 128 || C == 64 || C == 32) && c1.c_out == C && c2.c_in == C && c2.c_out == C &&
           c1.k == c2.k && (c1.k == 3 || c1.k == 7 || c1.k == 11) && (c1.dil == 1 || c1.dil == 3 || c1.dil == 5) && c2.dil == 1 &&
           c1.padding == (c1.k - 1) / 2 * c1.dil && c2.padding == (c2.k - 1) / 2 && !knobs().no_f16x3_pairs;
}

static fv_status conv_pair_run_f16x3(const ConvLayer& c1, const ConvLayer& c2, const float* x, float* y, int batch, int t,
                                     int out_mode, float out_scale, hipStream_t stream) {
    if (x == y) {
        set_error("conv_pair_run: output must not alias the input (halo reads)");
        return FV_ERR_INVALID;
    }
    const int C = c1.c_in;
    if ((long long)C * t >= (1LL << 30)) {
        set_error("conv_pair_run: a batch item of %lld elements exceeds the 4 GiB buffer-addressing span", (long long)C * t);
        return FV_ERR_UNSUPPORTED;
    }
    const PairF16Params p = pair_f16_params(c1, c2, c1.d_wph, c2.d_wph, C / 16, x, y, t, out_mode, out_scale);
    const int prof_idx = prof_begin(stream);
    bool ok = false;
    switch (c1.k) {
        case 3: ok = launch_pair_f16x3_k3(p, C, c1.dil, batch, stream); break;
        case 7: ok = launch_pair_f16x3_k7(p, C, c1.dil, batch, stream); break;
        case 11: ok = launch_pair_f16x3_k11(p, C, c1.dil, batch, stream); break;
        default: break;
    }
    const int tt = (C == 32 ? kPairF16ColsC32 : C == 64 ? 128 : 96) - (c1.k - 1);
    return finish_pair_launch(ok, "pair_f16x3", "f16x3 pair kernel", tt, 3.0, c1, t, batch, out_mode, stream, prof_idx);   // x, residual, y (+ accumulate)
}

// C = 16 in f16x3 mode (pair16_f16x3.hip): needs an even T and 8-byte aligned tensors (paired loads / stores); anything else
// keeps the exact-fp32 pair kernel
static bool pair16_f16x3_usable(const ConvLayer& c1, const ConvLayer& c2, const float* x, const float* y, int t) {
    return c1.precision == FV_PRECISION_F16X3 && c2.precision == FV_PRECISION_F16X3 && c1.d_wph16 && c2.d_wph16 &&
           c1.k == c2.k && (c1.dil == 1 || c1.dil == 3 || c1.dil == 5) && c2.dil == 1 &&
           c1.padding == (c1.k - 1) / 2 * c1.dil && c2.padding == (c2.k - 1) / 2 && t % 2 == 0 &&
           (((uintptr_t)x | (uintptr_t)y) & 7) == 0 && x != y && (long long)16 * t < (1LL << 30) &&
           !knobs().no_f16x3_pairs;
}

static fv_status conv_pair16_run_f16x3(const ConvLayer& c1, const ConvLayer& c2, const float* x, float* y, int batch, int t,
                                       int out_mode, float out_scale, hipStream_t stream) {
    const PairF16Params p = pair_f16_params(c1, c2, c1.d_wph16, c2.d_wph16, 1, x, y, t, out_mode, out_scale);
    const int prof_idx = prof_begin(stream);
    const bool ok = launch_pair16_f16x3(p, c1.k, c1.dil, batch, stream);
    return finish_pair_launch(ok, "pair_f16x3", "f16x3 pair kernel", pair16_f16x3_tile(c1.k, c1.dil), 3.0, c1, t, batch, out_mode, stream, prof_idx);
}

bool pair_wino_supported(int C, int ks, int dil) {
    if (dil != 1 && dil != 3 && dil != 5) return false;
    if (C == 16 || C == 32) return ks == 3 || ks == 7 || ks == 11;
    return (C == 64 || C == 128) && ks == 3;   // (wider pairs fuse at k = 3 only: resblock_pair.hip)
}

fv_status conv_pair_run(const ConvLayer& c1, const ConvLayer& c2, const float* x, float* y, int batch, int t, int out_mode,
                        float out_scale, hipStream_t stream, bool quad) {
    const int C = c1.c_in;
    if (pair_f16x3_supported(c1, c2)) return conv_pair_run_f16x3(c1, c2, x, y, batch, t, out_mode, out_scale, stream);
    if (pair16_f16x3_usable(c1, c2, x, y, t)) return conv_pair16_run_f16x3(c1, c2, x, y, batch, t, out_mode, out_scale, stream);
    const bool shape_ok = !c1.transposed && !c2.transposed && c1.c_out == C && c2.c_in == C && c2.c_out == C &&
                          c1.k == c2.k && c2.dil == 1 && c1.padding == (c1.k - 1) / 2 * c1.dil && c2.padding == (c2.k - 1) / 2;
    if (!shape_ok || !pair_supported(C, c1.k, c1.dil)) {
        set_error("conv_pair_run: unsupported pair (C=%d k=%d d=%d)", C, c1.k, c1.dil);
        return FV_ERR_UNSUPPORTED;
    }
    if (x == y) {
        set_error("conv_pair_run: output must not alias the input (halo reads)");
        return FV_ERR_INVALID;
    }
    // the narrow stages at k = 7 / 11: F(4,4) tap groups in both convs (pair_wino44_impl.h; round 5) — 20 / 13 products per four outputs against F(2,3)'s 32 / 20
    if (knobs().pair_wino && knobs().pair_wino44 && effective_algo() != FV_CONV_ALGO_DIRECT && c1.d_wpq16 && c2.d_wpq16 && (C == 16 || C == 32) &&
        (c1.k == 7 || c1.k == 11)) {
        const PairParams p = pair_params(c1, c2, c1.d_wpq16, c2.d_wpq16, x, y, t, out_mode, out_scale);
        const int prof_idx = prof_begin(stream);
        const bool ok = c1.k == 7 ? launch_pair_wino44_k7(p, C, c1.dil, batch, stream) : launch_pair_wino44_k11(p, C, c1.dil, batch, stream);
        const int nbq = 16 * (4 / (C / 16));
        const int tt = 4 * (nbq / c1.dil * c1.dil) - (c1.k - 1);   // PQGeom::TT
        return finish_pair_launch(ok, "pair_wino44", "F(4,4) pair kernel", tt, 2.0, c1, t, batch, out_mode, stream, prof_idx);
    }
    // the wide stages at k = 3: ONE F(4,3) tap group in both convs (pair_wino4_impl.h; round 26) — 6 products per four outputs against F(2,3)'s 8.  Only where
    // the caller asks (the engine's pair branches, on launches that fill the chip) or FV_PAIR_WINO4=2, and never in batch-invariant mode: a clip's bits
    // must not depend on the size of the launch it is part of, so everything below that gate, and every direct call, keeps F(2,3)
    if (knobs().pair_wino && knobs().pair_wino4 != 0 && (quad || knobs().pair_wino4 == 2) && !cur_invariant() && effective_algo() != FV_CONV_ALGO_DIRECT &&
        c1.precision == FV_PRECISION_F32 && c2.precision == FV_PRECISION_F32 && c1.d_wpq3 && c2.d_wpq3 && (C == 64 || C == 128) && c1.k == 3 && (long long)C * t < (1LL << 30)) {
        const PairParams p = pair_params(c1, c2, c1.d_wpq3, c2.d_wpq3, x, y, t, out_mode, out_scale);
        const int prof_idx = prof_begin(stream);
        const bool ok = launch_pair_wino4_k3(p, C, c1.dil, batch, stream);
        return finish_pair_launch(ok, "pair_wino4", "F(4,3) pair kernel", pair_wino4_tile(c1.dil, C), 2.0, c1, t, batch, out_mode, stream, prof_idx);
    }
    const bool wide = C >= 64;   // 32x32x2 kernels on the layers' d_wpw; C <= 32: 16x16x4 kernels on d_wpw16
    if (knobs().pair_wino && effective_algo() != FV_CONV_ALGO_DIRECT && (wide ? (c1.d_wpw && c2.d_wpw) : (c1.d_wpw16 && c2.d_wpw16)) &&
        pair_wino_supported(C, c1.k, c1.dil)) {
        // Winograd F(2,3) tap groups in both convs (pair_wino_impl.h)
        PairParams p = pair_params(c1, c2, wide ? c1.d_wpw : c1.d_wpw16, wide ? c2.d_wpw : c2.d_wpw16, x, y, t, out_mode, out_scale);
        p.n_frag = c1.nchunk * c1.nv;
        p.b1n = c1.d_bias + c1.m_pad;
        p.b2n = c2.d_bias + c2.m_pad;
        const int prof_idx = prof_begin(stream);
        const bool ok = c1.k == 3 ? launch_pair_wino_k3(p, C, c1.dil, batch, stream)
                        : c1.k == 7 ? launch_pair_wino_k7(p, C, c1.dil, batch, stream) : launch_pair_wino_k11(p, C, c1.dil, batch, stream);
        const int nbp = C == 128 ? 32 : 64;
        const int tt = 2 * (nbp / c1.dil * c1.dil) - (c1.k - 1);   // PWGeom::TT / PW32Geom::TT
        return finish_pair_launch(ok, "pair_wino", "Winograd pair kernel", tt, 2.0, c1, t, batch, out_mode, stream, prof_idx);
    }
    const PairParams p = pair_params(c1, c2, C == 16 ? c1.d_wp16 : c1.d_wp, C == 16 ? c2.d_wp16 : c2.d_wp, x, y, t, out_mode, out_scale);
    const int prof_idx = prof_begin(stream);
    const bool ok = launch_resblock_pair(p, C, c1.k, c1.dil, batch, stream);
    const int tt = std::max(128, kPairCols / C) - (c1.k - 1);   // PairGeom::TT
    // algorithmic work: the two convs' MACs; bytes: x once + output once (+ accumulate operand)
    return finish_pair_launch(ok, "resblock_pair", "kernel", tt, 2.0, c1, t, batch, out_mode, stream, prof_idx);
}

}  // namespace fv
