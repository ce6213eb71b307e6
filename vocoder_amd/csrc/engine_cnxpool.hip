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
#include "cnx_stream_plan.h"
#include "engine_internal.h"
#include "sample_pool.h"

struct fv_cnxpool {
    fv_engine* eng = nullptr;
    int S = 0, max_chunk = 0;
    int L = 0, R = 0, step = 0, cap = 0;
    std::vector<int64_t> N, E;
    std::vector<int32_t> flushed;
    int launches = 0;
    float* slab = nullptr;
    size_t bytes = 0;
    float* in_ring = nullptr;             // (sessions, C_in, cap)
    std::vector<float*> ring;             // per block, (sessions, dim, cap): the block's input
    float* win = nullptr;                 // (sessions, C_in, 6 + max_chunk)
    float *A = nullptr, *Bf = nullptr;    // (max_dim, Pmax) each, Pmax = sessions (max_chunk + R): the running activation and the residual
    float *Hb = nullptr, *G = nullptr;    // (max_dim, Pmax), (4 max_dim, Pmax)
    // a step's tables, kept between steps so that a step allocates nothing once they have grown to `sessions` entries
    std::vector<long long> N2, E2;
    std::vector<CnxPoolEntry> tab;
    std::vector<PoolCropEntry> crop;
    ~fv_cnxpool() {
        if (slab) (void)hipFree(slab);
    }
};

namespace {

constexpr long long kCnxMaxFrames = 1LL << 30;

ConvRun cnx_pool_run(int T, const float* x, float* y) {
    ConvRun r;
    r.batch = 1, r.t_in = T, r.x = x, r.y = y;
    return r;
}

// The refusals of a pool step's items (sample_pool_admit, counting frames, 2^30 of them) and the emission rule: N2 and E2 per item
fv_status cnx_pool_admit(const char* fn, int R, int S, int max_chunk, const int64_t* received, const int64_t* emitted, const int32_t* flushed,
                         const fv_wavpool_item* items, int count, bool buffers, const float* d_x, long long x_row_stride, long long* N2,
                         long long* E2) {
    if (const fv_status st = sample_pool_admit(fn, "fv_cnxpool_reset", S, max_chunk, received, flushed, items, count, buffers, d_x, x_row_stride, N2,
                                               "frames", kCnxMaxFrames, "2^30"))
        return st;
    for (int i = 0; i < count; ++i) E2[i] = items[i].flush ? N2[i] : std::max((long long)emitted[items[i].session], N2[i] - R);
    return FV_OK;
}

fv_status cnx_pool_range(const char* fn, int sessions, int max_chunk) {
    if (sessions < 1 || sessions > 65535 || max_chunk < 1 || max_chunk > (1 << 20)) {
        set_error("%s: sessions (%d) must lie in [1, 65535] and max_chunk (%d) in [1, 2^20]", fn, sessions, max_chunk);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

bool valid_slot(const fv_cnxpool* p, int s) { return p && s >= 0 && s < p->S; }

}  // namespace

extern "C" {

FV_API int32_t fv_cnxpool_table_size(void) { return kCnxPoolBlock; }

FV_API fv_status fv_cnxpool_create(fv_engine* e, int32_t sessions, int32_t max_chunk, fv_cnxpool** out) {
    const char* fn = "fv_cnxpool_create";
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
        set_error("%s: the layer pool serves FV_MODEL_CONVNEXT engines only (this engine's model is %d)", fn, (int)e->cfg.model);
        return FV_ERR_INVALID;
    }
    const ConvNeXtModel& m = e->cnx;
    if (m.cfg.kernel_size != 7) {
        set_error("%s: kernel_size = %d: the pool form of the depthwise kernel exists for kernel_size = 7 only", fn, m.cfg.kernel_size);
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
    if (sessions < 1 || sessions > 65535) {
        set_error("%s: sessions = %d must lie in [1, 65535]", fn, sessions);
        return FV_ERR_INVALID;
    }
    if (max_chunk < 1 || max_chunk > (1 << 16)) {
        set_error("%s: max_chunk = %d must lie in [1, 2^16]", fn, max_chunk);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_cnxpool> s(new fv_cnxpool());
    s->eng = e, s->S = sessions, s->max_chunk = max_chunk;
    for (int i = 0; i < m.cfg.num_stages; ++i) s->L += m.cfg.depths[i];
    s->R = cnx_reach(s->L);
    // fv_reach_frames is this reach plus the 2 frames of margin every engine window keeps
    if (s->R + 2 != e->reach_frames()) {
        set_error("%s: the pool's reach %d + 2 is not the engine's %d", fn, s->R, e->reach_frames());
        return FV_ERR_STATE;
    }
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
    s->N.assign(Sz, 0), s->E.assign(Sz, 0), s->flushed.assign(Sz, 0);
    s->N2.reserve(Sz), s->E2.reserve(Sz), s->tab.reserve(Sz), s->crop.reserve(Sz);
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
        s->in_ring = take(Sz * Cin * s->cap);
        for (int i = 0; i < m.cfg.num_stages; ++i)
            for (int j = 0; j < m.cfg.depths[i]; ++j) s->ring.push_back(take(Sz * m.cfg.dims[i] * s->cap));
        s->win = take(Sz * Cin * Wmax);
        s->A = take(dmax * Pmax), s->Bf = take(dmax * Pmax);
        s->Hb = take(dmax * Pmax), s->G = take(4 * dmax * Pmax);
        if (pass == 0) {
            s->bytes = used * sizeof(float);
            FV_HIP_CHECK(hipMalloc(&s->slab, s->bytes));
        }
    }
    *out = s.release();
    return FV_OK;
}

FV_API int64_t fv_cnxpool_plan(int32_t reach, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                               const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out) {
    const char* fn = "fv_cnxpool_plan";
    if (reach < 0) {
        set_error("%s: reach = %d must be >= 0", fn, reach);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = cnx_pool_range(fn, sessions, max_chunk)) return st;
    if (!received || !emitted || (count > 0 && !frames_out)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status st = cnx_pool_admit(fn, reach, sessions, max_chunk, received, emitted, flushed, items, count, false, nullptr, 0, N2.data(),
                                            E2.data()))
        return st;
    return sample_pool_counts(emitted, items, count, E2.data(), frames_out);
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
    if (const fv_status st = cnx_pool_admit(fn, p->R, p->S, p->max_chunk, p->N.data(), p->E.data(), p->flushed.data(), items, count, true, d_x,
                                            x_row_stride, N2, E2))
        return st;
    if (d_x && x_item_stride < 0) {
        set_error("%s: x_item_stride = %lld is negative", fn, (long long)x_item_stride);
        return FV_ERR_INVALID;
    }
    if (out_cols > kCnxMaxFrames) {
        set_error("%s: out_cols = %d is more than 2^30", fn, out_cols);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = sample_pool_output(fn, "frames", items, count, p->E.data(), E2, 1, d_y != nullptr, out_cols, out_cols)) return st;
    if (count > 0 && out_cols > 0 && !d_y) {
        set_error("%s: null d_y although every row's first out_cols = %d columns are written", fn, out_cols);
        return FV_ERR_INVALID;
    }
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
    auto slot_N0 = [&](int i) { return (long long)p->N[(size_t)items[i].session]; };

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
            ConvRun r = cnx_pool_run(Wmax, p->win, Y);
            r.batch = count;
            if ((rc = conv_layer_run(stg.conv, r, st))) return rc;
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
            if ((rc = launch_dwconv_ln(X, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, Y, 1, stg.ln_dim, P, 1, 1e-6f, st))) return rc;
            if ((rc = conv_layer_run(stg.conv, cnx_pool_run(P, Y, X), st))) return rc;
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
                    ConvRun p1 = cnx_pool_run(Pn, p->Hb, p->G);
                    p1.post_act = FV_ACT_GELU;
                    if ((rc = conv_layer_run(blk.pw1, p1, st))) return rc;
                    ConvRun p2 = cnx_pool_run(Pn, p->G, Y);
                    p2.res = Y, p2.gamma = blk.d_gamma;
                    if ((rc = conv_layer_run(blk.pw2, p2, st))) return rc;
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
            const long long k = E2[i] - p->E[(size_t)items[i].session];
            p->crop[(size_t)i] = PoolCropEntry{i, k > 0 ? 0 : -1, tab[i].out_col, k};
        }
        if ((rc = launch_pool_crop(Y, d_y, p->crop.data(), count, Co, std::max(P, 1), out_cols, 1, st))) return rc;
        launches += (count + kPoolBlock - 1) / kPoolBlock;
    }
    if (launches) set_last_kernel("dwconv_ln_pool_kernel");
    for (int i = 0; i < count; ++i) {
        const size_t s = (size_t)items[i].session;
        if (frames_out) frames_out[i] = E2[i] - p->E[s];
        p->N[s] = N2[i], p->E[s] = E2[i];
        if (items[i].flush) p->flushed[s] = 1;
    }
    p->launches = launches;
    return FV_OK;
}

FV_API fv_status fv_cnxpool_reset(fv_cnxpool* p, int32_t session) {
    const char* fn = "fv_cnxpool_reset";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    if (session < 0 || session >= p->S) {
        set_error("%s: session %d lies outside [0, %d)", fn, session, p->S);
        return FV_ERR_INVALID;
    }
    // the slot's ring rows keep their frames: nothing at or past a frontier, or before frame 0, is ever read
    p->N[(size_t)session] = p->E[(size_t)session] = 0, p->flushed[(size_t)session] = 0;
    return FV_OK;
}

FV_API int64_t fv_cnxpool_received(const fv_cnxpool* p, int32_t session) { return valid_slot(p, session) ? p->N[(size_t)session] : -1; }

FV_API int64_t fv_cnxpool_emitted(const fv_cnxpool* p, int32_t session) { return valid_slot(p, session) ? p->E[(size_t)session] : -1; }

FV_API int64_t fv_cnxpool_pending(const fv_cnxpool* p, int32_t session) {
    return valid_slot(p, session) ? p->N[(size_t)session] - p->E[(size_t)session] : -1;
}

FV_API int32_t fv_cnxpool_lookahead(const fv_cnxpool* p) { return p ? p->R : -1; }

FV_API int64_t fv_cnxpool_max_frames(const fv_cnxpool* p) { return p ? (int64_t)p->max_chunk + p->R : -1; }

FV_API int32_t fv_cnxpool_launches(const fv_cnxpool* p) { return p ? p->launches : -1; }

FV_API int64_t fv_cnxpool_state_bytes(const fv_cnxpool* p) { return p ? (int64_t)p->bytes : -1; }

FV_API void fv_cnxpool_destroy(fv_cnxpool* p) { delete p; }

}  // extern "C"
