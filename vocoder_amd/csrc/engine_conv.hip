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

}  // extern "C"
