// The ConvNeXt layer session pool (fv_cnxpool_*): what fv_cnxstream_* is to rows in lockstep, for `sessions` slots that advance independently.
// A slot's state is its own row of every ring — the input ring and one ring per block, (sessions, dim, cap) — and its counters N, E and
// flushed.  A step plans every item at every level on the host (cnx_stream_plan.h, per item its slot's (N0, N1, flush)) and then runs, per
// level, one launch per table of kCnxPoolBlock entries:
//   stem    cnx_stem_pool_window_kernel (slot ring ++ chunk row -> win (count, C_in, Wmax), exact zeros past an item's frames), the unchanged
//           conv_layer_run over win, the unchanged channels-first LayerNorm; level 1 reads row i from column off_i on
//   block   dwconv_ln_pool_kernel (H and the residual, PACKED (dim, P): item i's new columns from the prefix sum pk(i) on), then pwconv1 +
//           GELU and pwconv2 * gamma + residual over the packed buffer as one row of P columns
//   between stages and at the end: the unchanged LayerNorm (+ 1 x 1 conv) over the packed buffer; launch_pool_crop hands every item its columns
// Pointwise work is thereby proportional to the columns that are new, not to count x the longest item.  Every launch runs under
// AlgoScope(FV_CONV_ALGO_DIRECT, invariant = true), as the stream's do: a column's bits do not depend on what else the launch holds.
// The slots' counters, the refusals of a step, the plan entry and the emission rule are frame_pool.h's (FramePool); the engine checks of the
// create, the allocation and the launch pairs the stream states too (a block's pointwise half, the stage transition) are cnx_rings.h's.
#include "cnx_rings.h"
#include "frame_pool.h"

// The rings and a step's scratch for `sessions` slots: win (sessions, C_in, 6 + max_chunk); A, Bf and Hb (max_dim, Pmax) and G (4 max_dim,
// Pmax), Pmax = sessions (max_chunk + R) packed columns
struct fv_cnxpool : CnxRings {
    fv_engine* eng = nullptr;
    FramePool count;
    // a step's tables, kept between steps so that a step allocates nothing once they have grown to `sessions` entries
    std::vector<long long> N2, E2;
    std::vector<CnxPoolEntry> tab;
    std::vector<PoolCropEntry> crop;
};

extern "C" {

FV_API int32_t fv_cnxpool_table_size(void) { return kCnxPoolBlock; }

FV_API fv_status fv_cnxpool_create(fv_engine* e, int32_t sessions, int32_t max_chunk, fv_cnxpool** out) {
    const char* fn = "fv_cnxpool_create";
    if (!out || !e) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<fv_cnxpool> s(new fv_cnxpool());
    int dmax = 0;
    if (const fv_status rs = s->attach(fn, "pool", e, "sessions", sessions, max_chunk, &dmax)) return rs;
    const ConvNeXtModel& m = e->cnx;
    s->eng = e;
    s->step = cnx_pool_step(max_chunk, s->L), s->cap = cnx_ring_cap(s->step);
    const int Cin = m.cfg.input_channels;
    const size_t Sz = (size_t)sessions, Pmax = Sz * (size_t)s->step, Wmax = (size_t)(kCnxHalo + max_chunk);
    // The packed buffers are addressed as one row of Pmax columns with 32-bit byte offsets, G being the widest (4 max(dims) channels); a
    // ring and win are addressed per slot row with int element offsets.  dmax * Pmax < 2^27 also keeps every packed LayerNorm in the tile kernel.
    if (4ULL * dmax * Pmax >= (1ULL << 29)) {
        set_error("%s: 4 x %d channels x sessions = %d x (max_chunk = %d + %d) packed columns are more than the pool's 32-bit addressing holds",
                  fn, dmax, sessions, max_chunk, s->R);
        return FV_ERR_INVALID;
    }
    if ((unsigned long long)std::max(dmax, Cin) * (unsigned long long)s->cap >= (1ULL << 28) || Sz * Cin * Wmax >= (1ULL << 29)) {
        set_error("%s: a ring of %d x %d floats per slot, or the stem window of sessions = %d x %d x %zu floats, is more than the pool's 32-bit "
                  "addressing holds", fn, std::max(dmax, Cin), s->cap, sessions, Cin, Wmax);
        return FV_ERR_INVALID;
    }
    s->count.init(sessions, max_chunk, s->R);
    s->N2.reserve(Sz), s->E2.reserve(Sz), s->tab.reserve(Sz), s->crop.reserve(Sz);
    if (const fv_status rs = s->carve(m, dmax, Sz, Wmax, Pmax, Pmax)) return rs;
    *out = s.release();
    return FV_OK;
}

FV_API int64_t fv_cnxpool_plan(int32_t reach, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                               const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out) {
    return FramePool::plan("fv_cnxpool_plan", "fv_cnxpool_reset", reach, sessions, max_chunk, received, emitted, flushed, items, count, frames_out);
}

FV_API fv_status fv_cnxpool_step(fv_cnxpool* p, const fv_wavpool_item* items, int32_t count, const float* d_x, int64_t x_item_stride,
                                 int64_t x_row_stride, float* d_y, int32_t out_cols, int64_t* frames_out, void* stream) {
    const char* fn = "fv_cnxpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    const size_t cz = (size_t)std::max(count, 0);
    p->N2.resize(cz), p->E2.resize(cz);
    long long *N2 = p->N2.data(), *E2 = p->E2.data();
    const FramePool& fc = p->count;
    if (const fv_status st = fc.admit(fn, "fv_cnxpool_reset", items, count, d_x, x_row_stride, N2, E2)) return st;
    if (const fv_status st = fc.output(fn, "d_y", items, count, d_x, x_item_stride, E2, d_y != nullptr, out_cols)) return st;
    // everything is validated: enqueue

    fv_engine* e = p->eng;
    ConvNeXtModel& m = e->cnx;
    hipStream_t st = (hipStream_t)stream;
    const AlgoScope scope(FV_CONV_ALGO_DIRECT, true);   // as the stream: every column one fixed-order sum, direct sums in a C -> C stem
    const ProfScope prof(e);
    fv_status rc;
    int launches = 0;
    p->tab.resize(cz);
    CnxPoolEntry* tab = p->tab.data();
    auto slot_N0 = [&](int i) { return (long long)fc.N[(size_t)items[i].session]; };

    // the stem: every item's window; row i of its output holds the new columns [out0, out1) from column off_i on
    int longest = 0;
    bool stem_work = false, stem_out = false;
    for (int i = 0; i < count; ++i) {
        const long long N0 = slot_N0(i);
        const CnxStemPlan sp = cnx_stem_plan(N0, N2[i], items[i].flush != 0);
        longest = std::max(longest, items[i].samples);
        stem_work = stem_work || items[i].samples > 0 || sp.out1 > sp.out0;
        stem_out = stem_out || sp.out1 > sp.out0;
        tab[i] = CnxPoolEntry{items[i].session, (int)N0, (int)N2[i], (int)sp.out0, (int)sp.out1, 0, 0, 0};
    }
    const int Wmax = kCnxHalo + longest;
    float *X = p->A, *Y = p->Bf;
    if (stem_work) {
        CnxStage& stg = *m.stages[0];
        if ((rc = launch_cnx_stem_pool_window(d_x, x_item_stride, x_row_stride, p->in_ring, p->win, tab, count, m.cfg.input_channels, p->cap, Wmax,
                                              st, &launches)))
            return rc;
        if (stem_out) {
            if ((rc = conv_layer_run(stg.conv, cnx_run(count, Wmax, p->win, Y), st))) return rc;
            if ((rc = launch_dwconv_ln(Y, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, X, count, m.cfg.dims[0], Wmax, 1, 1e-6f, st))) return rc;
            launches += 2;
        }
    }
    // P: the packed columns of the level below (its buffer's row stride); level 0's output is padded rows instead
    int level = 0, P = 0;
    for (int si = 0; si < m.cfg.num_stages; ++si) {
        CnxStage& stg = *m.stages[si];
        const int dim = m.cfg.dims[si];
        if (si > 0 && P > 0) {
            // LayerNorm + 1 x 1 conv on the packed columns the last block of the stage below produced in this step
            if ((rc = cnx_stage_transition(stg, 1, P, X, Y, st))) return rc;
            launches += 2;
        }
        for (auto& bp : stg.blocks) {
            CnxBlock& blk = *bp;
            ++level;
            int Pn = 0, tiles = 0;
            for (int i = 0; i < count; ++i) {
                const long long N0 = slot_N0(i);
                const bool flush = items[i].flush != 0;
                const CnxLevelPlan q = cnx_level_plan(N0, N2[i], flush, level);
                // where frame in0 lies: row i of the stem's padded output, or the item's columns of the packed level below
                const int base = level == 1 ? i * m.cfg.dims[0] * Wmax + cnx_stem_plan(N0, N2[i], flush).off : tab[i].out_col;
                tab[i] = CnxPoolEntry{items[i].session, (int)q.in0, (int)q.in1, (int)q.out0, (int)q.out1, q.tiles, base, Pn};
                Pn += (int)(q.out1 - q.out0);
                tiles = std::max(tiles, q.tiles);
            }
            if (tiles > 0) {
                DwPoolRun r;
                r.ring = p->ring[(size_t)level - 1], r.cap = p->cap;
                r.chunk = X, r.chunk_stride = level == 1 ? Wmax : P;
                r.h = p->Hb, r.xres = Y, r.ostride = Pn;
                if ((rc = launch_dwconv_ln_pool(r, tab, count, blk.d_dw_w, blk.d_dw_b, blk.d_ln_w, blk.d_ln_b, dim, 1e-6f, st, &launches))) return rc;
                if (Pn > 0) {
                    if ((rc = cnx_block_pointwise(blk, 1, Pn, p->Hb, p->G, Y, st))) return rc;
                    launches += 2;
                }
                std::swap(X, Y);        // the block's output, packed (dim, Pn)
            }
            P = Pn;                     // nothing new at this level: nothing new at any above it either
        }
    }
    // the last level's packed columns are the step's emission: item i's k_i frames at tab[i].out_col
    if (count > 0 && out_cols > 0) {
        const int Co = m.out_dim();
        if (P > 0) {
            if ((rc = launch_dwconv_ln(X, nullptr, nullptr, m.d_norm_w, m.d_norm_b, Y, 1, Co, P, 1, 1e-6f, st))) return rc;
            ++launches;
        }
        p->crop.resize(cz);
        for (int i = 0; i < count; ++i) {
            const long long k = E2[i] - fc.E[(size_t)items[i].session];
            p->crop[(size_t)i] = PoolCropEntry{i, k > 0 ? 0 : -1, tab[i].out_col, k};
        }
        if ((rc = launch_pool_crop(Y, d_y, p->crop.data(), count, Co, std::max(P, 1), out_cols, 1, st))) return rc;
        launches += (count + kPoolBlock - 1) / kPoolBlock;
    }
    if (launches) set_last_kernel("dwconv_ln_pool_kernel");
    p->count.commit(items, count, N2, E2, frames_out, launches);
    return FV_OK;
}

FV_API fv_status fv_cnxpool_reset(fv_cnxpool* p, int32_t session) {
    return frame_pool_reset("fv_cnxpool_reset", p ? &p->count : nullptr, session);
}

FV_API int64_t fv_cnxpool_received(const fv_cnxpool* p, int32_t session) { return p ? p->count.received(session) : -1; }

FV_API int64_t fv_cnxpool_emitted(const fv_cnxpool* p, int32_t session) { return p ? p->count.emitted(session) : -1; }

FV_API int64_t fv_cnxpool_pending(const fv_cnxpool* p, int32_t session) { return p ? p->count.pending(session) : -1; }

FV_API int32_t fv_cnxpool_lookahead(const fv_cnxpool* p) { return p ? p->R : -1; }

FV_API int64_t fv_cnxpool_max_frames(const fv_cnxpool* p) { return p ? p->count.max_frames() : -1; }

FV_API int32_t fv_cnxpool_launches(const fv_cnxpool* p) { return p ? p->count.launches : -1; }

FV_API int64_t fv_cnxpool_state_bytes(const fv_cnxpool* p) { return p ? (int64_t)p->bytes : -1; }

FV_API void fv_cnxpool_destroy(fv_cnxpool* p) { delete p; }

}  // extern "C"
