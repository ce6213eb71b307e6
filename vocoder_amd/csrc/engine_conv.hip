// The single-layer ABI (fv_conv_*): one conv, or one fused (c1, c2) pair, outside any model — what the per-layer tests and probes drive.
#include "engine_internal.h"

extern "C" {

// ---- single conv layer ----
struct fv_conv {
    ConvLayer L;
    fv_conv_desc desc;
};

FV_API fv_status fv_conv_create(const fv_conv_desc* d, const float* host_weight, const float* host_bias, fv_conv** out) {
    if (!d || !host_weight || !out) {
        set_error("fv_conv_create: null argument");
        return FV_ERR_INVALID;
    }
    fv_conv* c = new (std::nothrow) fv_conv();
    if (!c) {
        set_error("out of host memory");
        return FV_ERR_INVALID;
    }
    c->desc = *d;
    fv_status st = conv_layer_create(c->L, d->transposed != 0, d->c_in, d->c_out, d->kernel_size,
                                     d->transposed ? 1 : d->dilation, d->padding, d->transposed ? d->stride : 1,
                                     host_weight, host_bias, /*with_f16x3=*/true);
    if (st) {
        conv_layer_destroy(c->L);
        delete c;
        return st;
    }
    *out = c;
    return FV_OK;
}

FV_API int64_t fv_conv_output_length(const fv_conv* c, int32_t t_in) { return c ? c->L.out_len(t_in) : 0; }

FV_API fv_status fv_conv_forward(fv_conv* c, const float* d_x, float* d_y, const float* d_residual, int32_t batch, int32_t t_in,
                          void* stream) {
    if (!c || !d_x || !d_y) {
        set_error("fv_conv_forward: null argument");
        return FV_ERR_INVALID;
    }
    ConvRun r;
    r.x = d_x;
    r.y = d_y;
    r.res = d_residual;
    r.batch = batch;
    r.t_in = t_in;
    r.pre_act = c->desc.pre_act;
    r.post_act = c->desc.post_act;
    r.slope = c->desc.act_slope;
    const AlgoScope algo_scope(c->L.algo, false);
    return conv_layer_run(c->L, r, (hipStream_t)stream);
}

/* y = x + c2(silu(c1(silu(x)))) in one launch (narrow channels only); c1/c2 are fv_conv handles of equal C and k. */
FV_API fv_status fv_conv_pair_forward(fv_conv* c1, fv_conv* c2, const float* d_x, float* d_y, int32_t batch, int32_t t,
                                      void* stream) {
    if (!c1 || !c2 || !d_x || !d_y) {
        set_error("fv_conv_pair_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (batch < 1 || t < 1) {
        set_error("fv_conv_pair_forward: empty input");
        return FV_ERR_INVALID;
    }
    const AlgoScope algo_scope(c1->L.algo, false);
    return conv_pair_run(c1->L, c2->L, d_x, d_y, batch, t, OUT_SET, 1.0f, (hipStream_t)stream);
}

FV_API int32_t fv_pair_wino4_tile(int32_t c, int32_t dilation) {
    return ((c == 64 || c == 128) && (dilation == 1 || dilation == 3 || dilation == 5)) ? pair_wino4_tile(dilation, c) : 0;
}

FV_API int64_t fv_pair_wino4_pack(const float* w, int32_t c, float* out, int64_t cap) {
    if (!w || (c != 64 && c != 128)) return 0;
    const std::vector<float> packed = pack_pair_wino4(std::vector<float>(w, w + (size_t)c * c * 3), c);
    if (out && cap >= (int64_t)packed.size()) std::copy(packed.begin(), packed.end(), out);
    return (int64_t)packed.size();
}

FV_API fv_status fv_conv_set_precision(fv_conv* c, int32_t precision) {
    if (!c || (precision != FV_PRECISION_F32 && precision != FV_PRECISION_F16X3)) {
        set_error("fv_conv_set_precision: invalid argument");
        return FV_ERR_INVALID;
    }
    c->L.precision = precision;
    return FV_OK;
}

FV_API fv_status fv_conv_set_algorithm(fv_conv* c, int32_t algo) {
    if (!c || (algo != FV_CONV_ALGO_AUTO && algo != FV_CONV_ALGO_DIRECT && algo != FV_CONV_ALGO_WINOGRAD)) {
        set_error("fv_conv_set_algorithm: invalid argument");
        return FV_ERR_INVALID;
    }
    c->L.algo = algo;
    return FV_OK;
}

FV_API void fv_conv_destroy(fv_conv* c) {
    if (!c) return;
    conv_layer_destroy(c->L);
    delete c;
}

// ---- single helper ops ----
}  // extern "C"

namespace {
// [a, a + na) and [b, b + nb) floats share a byte
bool floats_overlap(const float* a, long long na, const float* b, long long nb) {
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}
constexpr long long kHelperMaxT = 2147483647LL - 4096;   // the kernels' 32-bit column arithmetic reaches a tile and a halo past T
constexpr long long kHelperMaxGrid = 2147483647LL - 8;
}  // namespace

extern "C" {

FV_API fv_status fv_aa_snake_forward(const float* d_x, const float* d_x2, const float* d_x3, float* d_y, const float* d_alpha,
                                     const float* d_inv_beta, const float* d_up_taps, const float* d_down_taps, int32_t batch,
                                     int32_t channels, int64_t T, void* stream) {
    const char* fn = "fv_aa_snake_forward";
    if (batch < 0) {
        set_error("%s: batch = %d must be >= 0", fn, batch);
        return FV_ERR_INVALID;
    }
    if (channels < 1) {
        set_error("%s: channels = %d must be >= 1", fn, channels);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kHelperMaxT) {
        set_error("%s: T = %lld must lie in [0, %lld]", fn, (long long)T, kHelperMaxT);
        return FV_ERR_INVALID;
    }
    const long long rows = (long long)batch * channels, wg_per_row = (T + 2047) / 2048;   // a workgroup owns two 1024-column tiles
    if (wg_per_row && rows > kHelperMaxGrid / wg_per_row) {
        set_error("%s: batch * channels = %lld rows of T = %lld are more workgroups than one launch holds", fn, rows, (long long)T);
        return FV_ERR_INVALID;
    }
    if ((d_x2 == nullptr) != (d_x3 == nullptr)) {
        set_error("%s: d_x2 and d_x3 go together (%s is NULL)", fn, d_x2 ? "d_x3" : "d_x2");
        return FV_ERR_INVALID;
    }
    if (batch == 0 || T == 0) return FV_OK;
    const float* req[] = {d_x, d_y, d_alpha, d_inv_beta, d_up_taps, d_down_taps};
    const char* req_name[] = {"d_x", "d_y", "d_alpha", "d_inv_beta", "d_up_taps", "d_down_taps"};
    for (int i = 0; i < 6; ++i)
        if (!req[i]) {
            set_error("%s: null argument (%s)", fn, req_name[i]);
            return FV_ERR_INVALID;
        }
    const long long n = rows * T;
    const float* in[] = {d_x, d_x2, d_x3, d_alpha, d_inv_beta, d_up_taps, d_down_taps};
    const long long in_n[] = {n, n, n, channels, channels, 12, 12};
    const char* in_name[] = {"d_x", "d_x2", "d_x3", "d_alpha", "d_inv_beta", "d_up_taps", "d_down_taps"};
    for (int i = 0; i < 7; ++i)
        if (floats_overlap(d_y, n, in[i], in_n[i])) {
            set_error("%s: d_y overlaps %s (workgroups read their neighbours' halo)", fn, in_name[i]);
            return FV_ERR_INVALID;
        }
    const AaSnakeForm form = aa_snake_form(d_x, d_y, d_x2, (int)T);
    const fv_status st = launch_aa_snake(d_x, d_y, d_alpha, d_inv_beta, d_up_taps, d_down_taps, batch, channels, (int)T, (hipStream_t)stream,
                                         d_x2, d_x3);
    if (st == FV_OK) set_last_kernel(aa_snake_form_name(form));
    return st;
}

FV_API fv_status fv_dwconv_ln_forward(const float* d_x, const float* d_dw_weight, const float* d_dw_bias, const float* d_ln_weight,
                                      const float* d_ln_bias, float* d_y, int32_t batch, int32_t channels, int64_t T, int32_t kernel_size,
                                      float eps, void* stream) {
    const char* fn = "fv_dwconv_ln_forward";
    if (batch < 0) {
        set_error("%s: batch = %d must be >= 0", fn, batch);
        return FV_ERR_INVALID;
    }
    if (channels < 1) {
        set_error("%s: channels = %d must be >= 1", fn, channels);
        return FV_ERR_INVALID;
    }
    if (T < 0 || T > kHelperMaxT) {
        set_error("%s: T = %lld must lie in [0, %lld]", fn, (long long)T, kHelperMaxT);
        return FV_ERR_INVALID;
    }
    if ((long long)batch * ((T + 15) / 16) > kHelperMaxGrid) {
        set_error("%s: batch = %d rows of T = %lld are more workgroups than one launch holds", fn, batch, (long long)T);
        return FV_ERR_INVALID;
    }
    if (kernel_size < 1 || kernel_size % 2 == 0) {
        set_error("%s: kernel_size = %d must be odd and >= 1", fn, kernel_size);
        return FV_ERR_INVALID;
    }
    if (!d_dw_weight && (kernel_size != 1 || d_dw_bias)) {
        set_error("%s: without d_dw_weight (LayerNorm alone) kernel_size = %d must be 1 and d_dw_bias NULL", fn, kernel_size);
        return FV_ERR_INVALID;
    }
    if (!(eps >= 0.f)) {
        set_error("%s: eps = %g must be >= 0", fn, (double)eps);
        return FV_ERR_INVALID;
    }
    if (batch == 0 || T == 0) return FV_OK;
    if (!d_x || !d_ln_weight || !d_ln_bias || !d_y) {
        set_error("%s: null argument (%s)", fn, !d_x ? "d_x" : !d_ln_weight ? "d_ln_weight" : !d_ln_bias ? "d_ln_bias" : "d_y");
        return FV_ERR_INVALID;
    }
    const long long n = (long long)batch * channels * T;
    const float* in[] = {d_x, d_dw_weight, d_dw_bias, d_ln_weight, d_ln_bias};
    const long long in_n[] = {n, (long long)channels * kernel_size, channels, channels, channels};
    const char* in_name[] = {"d_x", "d_dw_weight", "d_dw_bias", "d_ln_weight", "d_ln_bias"};
    for (int i = 0; i < 5; ++i)
        if (floats_overlap(d_y, n, in[i], in_n[i])) {
            set_error("%s: d_y overlaps %s (workgroups read their neighbours' halo)", fn, in_name[i]);
            return FV_ERR_INVALID;
        }
    const DwlnForm form = dwln_form(d_dw_weight != nullptr, channels, (int)T, kernel_size);
    const fv_status st = launch_dwconv_ln(d_x, d_dw_weight, d_dw_bias, d_ln_weight, d_ln_bias, d_y, batch, channels, (int)T, kernel_size, eps,
                                          (hipStream_t)stream);
    if (st == FV_OK) {
        char name[64];
        dwln_form_name(form, name, sizeof name);
        set_last_kernel(name);
    }
    return st;
}

}  // extern "C"
