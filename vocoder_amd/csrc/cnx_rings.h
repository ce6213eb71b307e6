// What the ConvNeXt layer stream (engine_cnxstream.hip) and layer pool (engine_cnxpool.hip) state the same way, as WnRings does for the
// posterior stream and pool (wavenet.hip): the checks of the engine a create attaches to, the one allocation that holds the rings and a
// call's scratch for `rows` rows (a stream's batch rows, a pool's slots), and the two launch pairs both level loops contain — a block's
// pointwise half and the stage transition — over (B, n) linear columns or (1, Pn) packed ones.  The level loops themselves differ (a linear
// buffer with an offset, a table with packed offsets) and stay in their files.
#pragma once

#include "cnx_stream_plan.h"
#include "engine_internal.h"

namespace fv {

struct CnxRings {
    int L = 0, R = 0, step = 0, cap = 0;    // blocks, reach, the most frames one call adds to a frontier, slots of a ring
    float* slab = nullptr;
    size_t bytes = 0;
    float* in_ring = nullptr;               // (rows, C_in, cap)
    std::vector<float*> ring;               // per block, (rows, dim, cap): the block's input
    float* win = nullptr;                   // (rows, C_in, win_w): the stem's window
    float *A = nullptr, *Bf = nullptr;      // max_dim x act floats each: the running activation and the LayerNorm output / residual
    float *Hb = nullptr, *G = nullptr;      // max_dim x cols, 4 max_dim x cols
    ~CnxRings() {
        if (slab) (void)hipFree(slab);
    }

    // The checks of `fn` (a *_create of a `noun`: "stream" / "pool") on its engine, which is not NULL, and on its `rows_name` = rows and
    // max_chunk; sets L and R and gives the widest stage
    fv_status attach(const char* fn, const char* noun, const fv_engine* e, const char* rows_name, int rows, int max_chunk,
                     int* widest) {
        if (!e->finalized) {
            set_error("%s: the engine has not been finalized (fv_finalize)", fn);
            return FV_ERR_STATE;
        }
        if (e->cfg.model != FV_MODEL_CONVNEXT) {
            set_error("%s: the layer %s serves FV_MODEL_CONVNEXT engines only (this engine's model is %d)", fn, noun, (int)e->cfg.model);
            return FV_ERR_INVALID;
        }
        const ConvNeXtModel& m = e->cnx;
        if (m.cfg.kernel_size != 7) {
            set_error("%s: kernel_size = %d: the %s form of the depthwise kernel exists for kernel_size = 7 only", fn, m.cfg.kernel_size, noun);
            return FV_ERR_INVALID;
        }
        int dmax = 0;
        for (int i = 0; i < m.cfg.num_stages; ++i) dmax = std::max(dmax, m.cfg.dims[i]);
        if (dmax > 1024) {
            set_error("%s: a stage of %d channels is outside the depthwise tile kernel (1024 at the most)", fn, dmax);
            return FV_ERR_INVALID;
        }
        if (e->precision != FV_PRECISION_F32) {
            set_error("%s: precision f16x3 is not streamed by layers (the claim is the fp32 forward's bits)", fn);
            return FV_ERR_STATE;
        }
        if (rows < 1 || rows > 65535) {
            set_error("%s: %s = %d must lie in [1, 65535]", fn, rows_name, rows);
            return FV_ERR_INVALID;
        }
        if (max_chunk < 1 || max_chunk > (1 << 16)) {
            set_error("%s: max_chunk = %d must lie in [1, 2^16]", fn, max_chunk);
            return FV_ERR_INVALID;
        }
        L = 0;
        for (int i = 0; i < m.cfg.num_stages; ++i) L += m.cfg.depths[i];
        R = cnx_reach(L);
        // fv_reach_frames is this reach plus the 2 frames of margin every engine window keeps
        if (R + 2 != e->reach_frames()) {
            set_error("%s: the %s's reach %d + 2 is not the engine's %d", fn, noun, R, e->reach_frames());
            return FV_ERR_STATE;
        }
        *widest = dmax;
        return FV_OK;
    }

    // Two passes over one carving: the sizes, then the pointers (every buffer starts on a 256-byte boundary).  The rings and the window have
    // `rows` rows of `cap` and `win_w` columns; A and Bf hold `act` columns of the widest stage, Hb `cols` and G four times that.
    fv_status carve(const ConvNeXtModel& m, int dmax, size_t rows, size_t win_w, size_t act, size_t cols) {
        const size_t Cin = (size_t)m.cfg.input_channels;
        size_t used = 0;
        auto take = [&](size_t n) {
            float* p = slab ? slab + used : nullptr;
            used += (n + 63) / 64 * 64;
            return p;
        };
        for (int pass = 0; pass < 2; ++pass) {
            used = 0;
            ring.clear();
            in_ring = take(rows * Cin * cap);
            for (int i = 0; i < m.cfg.num_stages; ++i)
                for (int j = 0; j < m.cfg.depths[i]; ++j) ring.push_back(take(rows * m.cfg.dims[i] * cap));
            win = take(rows * Cin * win_w);
            A = take(dmax * act), Bf = take(dmax * act);
            Hb = take(dmax * cols), G = take(4 * dmax * cols);
            if (pass == 0) {
                bytes = used * sizeof(float);
                FV_HIP_CHECK(hipMalloc(&slab, bytes));
            }
        }
        return FV_OK;
    }
};

inline ConvRun cnx_run(int B, int T, const float* x, float* y) {
    ConvRun r;
    r.batch = B, r.t_in = T, r.x = x, r.y = y;
    return r;
}

// The pointwise half of a block over (B, n) columns: pwconv1 + GELU, H -> G, then pwconv2 * gamma + residual, G -> Y, which holds the residual
inline fv_status cnx_block_pointwise(CnxBlock& blk, int B, int n, const float* H, float* G, float* Y, hipStream_t st) {
    ConvRun p1 = cnx_run(B, n, H, G);
    p1.post_act = FV_ACT_GELU;
    if (const fv_status rc = conv_layer_run(blk.pw1, p1, st)) return rc;
    ConvRun p2 = cnx_run(B, n, G, Y);
    p2.res = Y, p2.gamma = blk.d_gamma;
    return conv_layer_run(blk.pw2, p2, st);
}

// The transition into stage `stg` over (B, n) columns of the stage below: LayerNorm X -> Y, then the 1 x 1 conv Y -> X
inline fv_status cnx_stage_transition(CnxStage& stg, int B, int n, float* X, float* Y, hipStream_t st) {
    if (const fv_status rc = launch_dwconv_ln(X, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, Y, B, stg.ln_dim, n, 1, 1e-6f, st)) return rc;
    return conv_layer_run(stg.conv, cnx_run(B, n, Y, X), st);
}

}  // namespace fv
