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
// The counters, the refusals of a push or flush and the emission rule are frame_pool.h's (FrameStream); the engine checks of the create, the
// allocation and the launch pairs the pool states too (a block's pointwise half, the stage transition) are cnx_rings.h's.
#include "cnx_rings.h"
#include "frame_pool.h"

// The rings and a call's scratch for `batch` rows: win (batch, C_in, 6 + step), A and Bf (batch, max_dim, 6 + step), Hb (batch, max_dim, step),
// G (batch, 4 max_dim, step)
struct fv_cnxstream : CnxRings {
    fv_engine* eng = nullptr;
    int batch = 0;
    FrameStream count;
};

namespace {

fv_status cnx_stream_advance(const char* fn, fv_cnxstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c,
                             bool flush, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream) {
    if (const fv_status rs = frame_stream_chunk(fn, "fv_cnxstream_reset", s ? &s->count : nullptr, c)) return rs;
    if (const fv_status rs = s->count.input(fn, d_x, x_batch_stride, x_row_stride, c)) return rs;
    long long N1, E1;
    if (const fv_status rs = s->count.output(fn, "d_y", c, flush, d_y != nullptr, y_row_stride, &N1, &E1)) return rs;
    fv_engine* e = s->eng;
    ConvNeXtModel& m = e->cnx;
    const int B = s->batch;
    const long long N0 = s->count.N, k = E1 - s->count.E;
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
            // X is linear (B, ln_dim, n) here: a block's output
            if (n > 0 && (rc = cnx_stage_transition(stg, B, n, X, Y, st))) return rc;
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
            if (n > 0 && (rc = cnx_block_pointwise(blk, B, n, s->Hb, s->G, Y, st))) return rc;
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
    s->count.commit(N1, E1, flush, emitted);
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
    std::unique_ptr<fv_cnxstream> s(new fv_cnxstream());
    int dmax = 0;
    if (const fv_status rs = s->attach(fn, "stream", e, "batch", batch, max_chunk, &dmax)) return rs;
    const ConvNeXtModel& m = e->cnx;
    s->eng = e, s->batch = batch;
    s->count.max_chunk = max_chunk, s->count.R = s->R;
    s->step = cnx_step(max_chunk, s->L), s->cap = cnx_ring_cap(s->step);
    const int Cin = m.cfg.input_channels;
    const size_t Bz = (size_t)batch, lin = (size_t)(kCnxHalo + s->step);
    if ((long long)std::max(dmax, Cin) * (long long)std::max<size_t>(s->cap, lin) >= (1LL << 28) || Bz * 4 * dmax * s->step >= (1ULL << 31)) {
        set_error("%s: batch = %d x max_chunk = %d is more than the stream's 32-bit addressing holds", fn, batch, max_chunk);
        return FV_ERR_INVALID;
    }
    if (const fv_status rs = s->carve(m, dmax, Bz, lin, Bz * lin, Bz * s->step)) return rs;
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
    return frame_stream_reset("fv_cnxstream_reset", s ? &s->count : nullptr);
}

FV_API int64_t fv_cnxstream_pending(const fv_cnxstream* s) { return s ? s->count.pending() : -1; }

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
