// The ConvNeXt layer stream (fv_cnxstream_*): the backbone chunk by chunk with the bits of the whole-row forward in batch-invariant mode.
// A block is a 7-tap depthwise conv and per-frame operations, so it needs no window: it needs the last 6 columns of its input, which live
// in a ring per block (cnx_stream_plan.h states which frames every level computes in a call and which slots it reads and writes).  A call
// runs, per level, over the columns that are new at that level:
//   stem    the window kernel (input ring ++ chunk -> 6 + c linear columns), the unchanged conv_layer_run over them, the unchanged
//           channels-first LayerNorm; the conv's edge columns are computed and never read, except where the zero padding is the true one
//   block   dwconv_ln_stream_kernel (H and the residual, linear), then pwconv1 + GELU and pwconv2 * gamma + residual as in run_convnext
//   between stages and at the end: the unchanged LayerNorm (+ 1 x 1 conv) on linear buffers
// Every launch runs under AlgoScope(FV_CONV_ALGO_DIRECT, invariant = true): kernel choices from the layer shape alone, no split-K, and
// direct sums for a stem that is a C -> C conv (the one ConvNeXt layer with a Winograd form; no other layer has an algorithm to choose).
#include "cnx_stream_plan.h"
#include "engine_internal.h"

struct fv_cnxstream {
    fv_engine* eng = nullptr;
    int batch = 0, max_chunk = 0;
    int L = 0, R = 0, step = 0, cap = 0;
    long long N = 0, E = 0;
    bool flushed = false;
    float* slab = nullptr;
    size_t bytes = 0;
    float* in_ring = nullptr;             // (batch, C_in, cap)
    std::vector<float*> ring;             // per block, (batch, dim, cap): the block's input
    float *win = nullptr;                 // (batch, C_in, 6 + step)
    float *A = nullptr, *Bf = nullptr;    // (batch, max_dim, 6 + step) each: the running activation and the LayerNorm output / residual
    float *Hb = nullptr, *G = nullptr;    // (batch, max_dim, step), (batch, 4 max_dim, step)
    ~fv_cnxstream() {
        if (slab) (void)hipFree(slab);
    }
};

namespace {

ConvRun cnx_run(int B, int T, const float* x, float* y) {
    ConvRun r;
    r.batch = B, r.t_in = T, r.x = x, r.y = y;
    return r;
}

fv_status cnx_stream_advance(const char* fn, fv_cnxstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c,
                             bool flush, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream) {
    if (!s) {
        set_error("%s: null stream", fn);
        return FV_ERR_INVALID;
    }
    if (s->flushed) {
        set_error("%s: the stream was flushed at %lld frames: fv_cnxstream_reset starts the next utterance", fn, s->N);
        return FV_ERR_STATE;
    }
    if (c < 0 || c > s->max_chunk) {
        set_error("%s: c = %d must lie in [0, max_chunk = %d]", fn, c, s->max_chunk);
        return FV_ERR_INVALID;
    }
    if (s->N + c > (1LL << 30)) {
        set_error("%s: %lld + %d frames are more than the 2^30 a stream counts", fn, s->N, c);
        return FV_ERR_INVALID;
    }
    if (c > 0 && !d_x) {
        set_error("%s: null d_x with c = %d", fn, c);
        return FV_ERR_INVALID;
    }
    if (c > 0 && (x_row_stride < c || x_batch_stride < 0)) {
        set_error("%s: x_row_stride = %lld (the stride between channels) is shorter than a chunk of c = %d frames, or x_batch_stride = %lld is "
                  "negative", fn, (long long)x_row_stride, c, (long long)x_batch_stride);
        return FV_ERR_INVALID;
    }
    fv_engine* e = s->eng;
    ConvNeXtModel& m = e->cnx;
    const int B = s->batch;
    const long long N0 = s->N, N1 = N0 + c, E0 = s->E, E1 = flush ? N1 : std::max(E0, N1 - s->R);
    const long long k = E1 - E0;
    if (k > 0 && !d_y) {
        set_error("%s: null d_y for the %lld frames this call emits", fn, k);
        return FV_ERR_INVALID;
    }
    if (k > 0 && y_row_stride < k) {
        set_error("%s: y_row_stride = %lld is shorter than the %lld frames this call emits", fn, (long long)y_row_stride, k);
        return FV_ERR_INVALID;
    }
    // everything is validated: enqueue

    hipStream_t st = (hipStream_t)stream;
    // Every column one fixed-order sum, whatever the launch holds.  Direct sums: a stem with input_channels == dims[0] is a C -> C k = 7 conv,
    // which conv_layer_create marks for the Winograd forms; their outputs come in pairs / quads whose sums take in the whole group's inputs, so a
    // column's bits depend on where the window begins and ends.  The direct-sum kernel has no such dependence.
    const AlgoScope scope(FV_CONV_ALGO_DIRECT, true);
    const ProfScope prof(e);
    fv_status rc;
    // X: the level's output of this call, linear (B, dim, Xw), its new columns from column Xoff on
    float *X = s->A, *Y = s->Bf;
    int Xw = 0, Xoff = 0;
    const CnxStemPlan sp = cnx_stem_plan(N0, N1, flush);
    if (c > 0 || sp.out1 > sp.out0) {
        CnxStage& stg = *m.stages[0];
        if ((rc = launch_cnx_stem_window(d_x, x_batch_stride, x_row_stride, s->in_ring, s->win, B, m.cfg.input_channels, s->cap, N0, c, st)))
            return rc;
        if (sp.out1 > sp.out0) {
            if ((rc = conv_layer_run(stg.conv, cnx_run(B, sp.W, s->win, Y), st))) return rc;
            if ((rc = launch_dwconv_ln(Y, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, X, B, m.cfg.dims[0], sp.W, 1, 1e-6f, st))) return rc;
            Xw = sp.W, Xoff = sp.off;
        }
    }
    int level = 0;
    for (int i = 0; i < m.cfg.num_stages; ++i) {
        CnxStage& stg = *m.stages[i];
        const int dim = m.cfg.dims[i];
        if (i > 0) {
            // LayerNorm + 1 x 1 conv on the columns the last block of the stage below produced in this call
            const int n = (int)(cnx_front(N1, level, flush) - cnx_front(N0, level, false));
            if (n > 0) {   // X is linear (B, ln_dim, n) here: a block's output
                if ((rc = launch_dwconv_ln(X, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, Y, B, stg.ln_dim, n, 1, 1e-6f, st))) return rc;
                if ((rc = conv_layer_run(stg.conv, cnx_run(B, n, Y, X), st))) return rc;
            }
        }
        for (auto& bp : stg.blocks) {
            CnxBlock& blk = *bp;
            ++level;
            const CnxLevelPlan q = cnx_level_plan(N0, N1, flush, level);
            if (q.tiles == 0) continue;   // nothing new at this level (and so at none above it)
            const int n = (int)(q.out1 - q.out0);
            DwStreamRun r;
            r.ring = s->ring[level - 1], r.cap = s->cap;
            r.chunk = X, r.chunk_stride = Xw, r.chunk_off = Xoff;
            r.h = s->Hb, r.xres = Y;
            r.in0 = (int)q.in0, r.in1 = (int)q.in1, r.out0 = (int)q.out0, r.out1 = (int)q.out1, r.tiles = q.tiles;
            if (r.chunk_stride == 0) r.chunk_stride = 1;   // no chunk frames (in0 == in1): nothing of it is addressed
            if ((rc = launch_dwconv_ln_stream(r, blk.d_dw_w, blk.d_dw_b, blk.d_ln_w, blk.d_ln_b, B, dim, 1e-6f, st))) return rc;
            if (n > 0) {
                ConvRun p1 = cnx_run(B, n, s->Hb, s->G);
                p1.post_act = FV_ACT_GELU;
                if ((rc = conv_layer_run(blk.pw1, p1, st))) return rc;
                ConvRun p2 = cnx_run(B, n, s->G, Y);
                p2.res = Y, p2.gamma = blk.d_gamma;
                if ((rc = conv_layer_run(blk.pw2, p2, st))) return rc;
            }
            std::swap(X, Y);        // the block's output, linear (B, dim, n)
            Xw = n, Xoff = 0;
        }
    }
    if (k > 0) {
        const int Co = m.out_dim();
        if (y_row_stride == k) {
            if ((rc = launch_dwconv_ln(X, nullptr, nullptr, m.d_norm_w, m.d_norm_b, d_y, B, Co, (int)k, 1, 1e-6f, st))) return rc;
        } else {
            if ((rc = launch_dwconv_ln(X, nullptr, nullptr, m.d_norm_w, m.d_norm_b, Y, B, Co, (int)k, 1, 1e-6f, st))) return rc;
            FV_HIP_CHECK(hipMemcpy2DAsync(d_y, (size_t)y_row_stride * 4, Y, (size_t)k * 4, (size_t)k * 4, (size_t)B * Co, hipMemcpyDeviceToDevice, st));
        }
    }
    s->N = N1, s->E = E1, s->flushed = flush;
    if (emitted) *emitted = k;
    return FV_OK;
}

}  // namespace

extern "C" {

FV_API fv_status fv_cnxstream_create(fv_engine* e, int32_t batch, int32_t max_chunk, fv_cnxstream** out) {
    const char* fn = "fv_cnxstream_create";
    if (!out || !e) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!e->finalized) {
        set_error("%s: the engine has not been finalized (fv_finalize)", fn);
        return FV_ERR_STATE;
    }
    if (e->cfg.model != FV_MODEL_CONVNEXT) {
        set_error("%s: the layer stream serves FV_MODEL_CONVNEXT engines only (this engine's model is %d)", fn, (int)e->cfg.model);
        return FV_ERR_INVALID;
    }
    const ConvNeXtModel& m = e->cnx;
    if (m.cfg.kernel_size != 7) {
        set_error("%s: kernel_size = %d: the stream form of the depthwise kernel exists for kernel_size = 7 only", fn, m.cfg.kernel_size);
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
    if (batch < 1 || batch > 65535) {
        set_error("%s: batch = %d must lie in [1, 65535]", fn, batch);
        return FV_ERR_INVALID;
    }
    if (max_chunk < 1 || max_chunk > (1 << 16)) {
        set_error("%s: max_chunk = %d must lie in [1, 2^16]", fn, max_chunk);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_cnxstream> s(new fv_cnxstream());
    s->eng = e, s->batch = batch, s->max_chunk = max_chunk;
    for (int i = 0; i < m.cfg.num_stages; ++i) s->L += m.cfg.depths[i];
    s->R = cnx_reach(s->L);
    // fv_reach_frames is this reach plus the 2 frames of margin every engine window keeps
    if (s->R + 2 != e->reach_frames()) {
        set_error("%s: the stream's reach %d + 2 is not the engine's %d", fn, s->R, e->reach_frames());
        return FV_ERR_STATE;
    }
    s->step = cnx_step(max_chunk, s->L), s->cap = cnx_ring_cap(s->step);
    const int Cin = m.cfg.input_channels;
    const size_t Bz = (size_t)batch, lin = (size_t)(kCnxHalo + s->step);
    if ((long long)std::max(dmax, Cin) * (long long)std::max<size_t>(s->cap, lin) >= (1LL << 28) || Bz * 4 * dmax * s->step >= (1ULL << 31)) {
        set_error("%s: batch = %d x max_chunk = %d is more than the stream's 32-bit addressing holds", fn, batch, max_chunk);
        return FV_ERR_INVALID;
    }
    // two passes over one carving: the sizes, then the pointers (every buffer starts on a 256-byte boundary)
    size_t used = 0;
    auto take = [&](size_t n) {
        float* p = s->slab ? s->slab + used : nullptr;
        used += (n + 63) / 64 * 64;
        return p;
    };
    for (int pass = 0; pass < 2; ++pass) {
        used = 0;
        s->ring.clear();
        s->in_ring = take(Bz * Cin * s->cap);
        for (int i = 0; i < m.cfg.num_stages; ++i)
            for (int j = 0; j < m.cfg.depths[i]; ++j) s->ring.push_back(take(Bz * m.cfg.dims[i] * s->cap));
        s->win = take(Bz * Cin * lin);
        s->A = take(Bz * dmax * lin), s->Bf = take(Bz * dmax * lin);
        s->Hb = take(Bz * dmax * s->step), s->G = take(Bz * 4 * dmax * s->step);
        if (pass == 0) {
            s->bytes = used * sizeof(float);
            FV_HIP_CHECK(hipMalloc(&s->slab, s->bytes));
        }
    }
    *out = s.release();
    return FV_OK;
}

FV_API fv_status fv_cnxstream_push(fv_cnxstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c, float* d_y,
                                   int64_t y_row_stride, int64_t* emitted, void* stream) {
    return cnx_stream_advance("fv_cnxstream_push", s, d_x, x_batch_stride, x_row_stride, c, false, d_y, y_row_stride, emitted, stream);
}

FV_API fv_status fv_cnxstream_flush(fv_cnxstream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream) {
    return cnx_stream_advance("fv_cnxstream_flush", s, nullptr, 0, 0, 0, true, d_y, y_row_stride, emitted, stream);
}

FV_API fv_status fv_cnxstream_reset(fv_cnxstream* s) {
    if (!s) {
        set_error("fv_cnxstream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->N = s->E = 0, s->flushed = false;        // the rings keep their frames: nothing at or past a frontier, or before frame 0, is ever read
    return FV_OK;
}

FV_API int64_t fv_cnxstream_pending(const fv_cnxstream* s) { return s ? s->N - s->E : -1; }

FV_API int32_t fv_cnxstream_lookahead(const fv_cnxstream* s) { return s ? s->R : -1; }

FV_API int64_t fv_cnxstream_state_bytes(const fv_cnxstream* s) { return s ? (int64_t)s->bytes : -1; }

FV_API void fv_cnxstream_destroy(fv_cnxstream* s) { delete s; }

FV_API int32_t fv_cnxstream_plan(int64_t N0, int64_t N1, int32_t flush, int32_t level, int32_t max_chunk, int32_t levels, int64_t* out) {
    if (!out || N0 < 0 || N1 < N0 || level < 0 || levels < level || max_chunk < 1) return -1;
    if (level == 0) {
        const CnxStemPlan sp = cnx_stem_plan(N0, N1, flush != 0);
        out[0] = N0, out[1] = N1, out[2] = sp.out0, out[3] = sp.out1, out[4] = sp.W, out[5] = sp.off;
    } else {
        const CnxLevelPlan q = cnx_level_plan(N0, N1, flush != 0, level);
        out[0] = q.in0, out[1] = q.in1, out[2] = q.out0, out[3] = q.out1, out[4] = q.tiles, out[5] = q.tiles > 1 ? cnx_file_from(q, 1) : -1;
    }
    return cnx_ring_cap(cnx_step(max_chunk, levels));
}

}  // extern "C"
