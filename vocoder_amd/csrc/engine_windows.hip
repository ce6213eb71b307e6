// Windowed forwards: the unchanged model run on windows of frames under the reach rule, keeping only the frames that lie a reach inside each
// window edge.  The reach and the frame-alignment test, and the four callers that share them and the window workspace: the time tiles of a
// long clip (run_model), streams (fv_stream_*), ragged batches (fv_ragged_*, planner included) and session pools (fv_pool_*, planner included).
// The copy kernels they launch: window_kernels.hip.
#include "engine_internal.h"

// ---- long clips as a batch of time tiles -------------------------------------------------------------------------
// One-sided reach of the generator in INPUT frames: an output sample depends on input frames no further away than this (an upper
// bound, walked backwards through the layers: every conv adds (k - 1) / 2 * dilation at its own rate, a transposed conv divides by
// its stride; the anti-aliased activations of BigVGAN add their two 12-tap filters at the doubled rate).
static int64_t ups_reach(const UpsamplerModel& m) {
    const fv_upsampler_config& c = m.cfg;
    const int aa = m.bigvgan ? 7 : 0;   // Activation1d: replicate-pad 5 + 6-tap polyphase up, 12-tap low-pass at 2x: <= 6.5 samples
    int64_t R = (c.post_conv_kernel_size - 1) / 2 + aa;
    for (int i = c.num_upsamples - 1; i >= 0; --i) {
        int64_t br = 0;
        for (int j = 0; j < c.num_kernels; ++j) {
            const int k = c.resblock_kernel_sizes[j];
            int64_t r = 0;
            for (int n = 0; n < FV_MAX_DILATIONS; ++n) r += (int64_t)(k - 1) / 2 * (c.resblock_dilation_sizes[j][n] + 1) + 2 * aa;
            br = std::max(br, r);
        }
        R += br + (c.use_template ? 2 : 0);   // noise_convs[i]: one stage sample either side of the strided template conv
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        R = (R + k - 1) / u + 1;
    }
    return R + (c.pre_conv_kernel_size - 1) / 2;
}
static int64_t cnx_reach(const ConvNeXtModel& m) {
    int64_t R = m.cfg.kernel_size / 2;   // stem
    for (int i = 0; i < m.cfg.num_stages; ++i) R += (int64_t)m.cfg.depths[i] * (m.cfg.kernel_size / 2);
    return R;
}
int fv_engine::reach_frames() const {
    int64_t R = 0;
    switch (cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: R = ups_reach(ups); break;
        case FV_MODEL_CONVNEXT: R = cnx_reach(cnx); break;
        case FV_MODEL_ISTFT_HEAD: R = (cfg.head.n_fft + cfg.head.hop_length - 1) / cfg.head.hop_length; break;
        case FV_MODEL_VOCOS: R = cnx_reach(cnx) + (cfg.head.n_fft + cfg.head.hop_length - 1) / cfg.head.hop_length; break;
        case FV_MODEL_FIREFLY: R = cnx_reach(cnx) + ups_reach(ups); break;
        case FV_MODEL_REFINEGAN:
            if (!noise_seeded) return -1;   // its AdaIN noise exists per call only: no window can reproduce it
            R = refine_reach(refine);
            break;
        default: return -1;   // LOGMEL: not tiled
    }
    return (int)std::min<int64_t>(R + 2, 1 << 20);
}
// The frame-aligned models, the ones a window of frames [a, b) can stand in for: a finite reach, no "center" ISTFT trim, and exactly hop output
// samples per input frame at both t_a and t_b frames — the gather / scatter of the time tiles and the window / crop of a stream address rows at
// frames x hop.  Returns hop, or 0 with the reason in *why (may be NULL).  Used by tile_plan and fv_stream_create.
int fv_engine::frame_hop(int t_a, int t_b, const char** why) const {
    const char* r = nullptr;
    if (cfg.model == FV_MODEL_LOGMEL)
        r = "the log-mel front-end (wave -> mel) is not frame-windowed";
    else if (cfg.model == FV_MODEL_REFINEGAN && !noise_seeded)
        r = "RefineGAN cannot be windowed without a noise seed (its AdaIN noise is drawn per call: fv_refinegan_set_noise_seed)";
    else if (reach_frames() < 0)
        r = "the model has no finite reach";
    else if ((cfg.model == FV_MODEL_VOCOS || cfg.model == FV_MODEL_ISTFT_HEAD) && head.center())
        r = "ISTFT head with padding=\"center\": the output is (T - 1) * hop samples, trimmed at both ends";
    if (!r && t_a >= 1 && t_b >= 1) {
        // A transposed conv with odd (kernel - rate) yields T u + 1 samples per stage (ConvLayer::out_len): not frames x hop
        const int64_t la = fv_output_length(this, t_a), lb = fv_output_length(this, t_b);
        const int64_t hop = la / t_a;
        if (hop >= 1 && la == hop * t_a && lb == hop * (int64_t)t_b) return (int)hop;
        r = "the output is not hop x frames samples (a transposed conv with odd kernel - rate adds a sample per stage)";
    }
    if (why) *why = r ? r : "empty input";
    return 0;
}
// Longest tile (frames) whose largest per-item tensor stays under HALF the 4 GiB addressing span of the conv kernels
int fv_engine::tile_frame_limit() const {
    int64_t per_frame = 1;
    switch (cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: per_frame = ups.max_elems(1 << 10) >> 10; break;
        case FV_MODEL_CONVNEXT: per_frame = 4LL * cnx.max_dim(); break;
        case FV_MODEL_ISTFT_HEAD: per_frame = std::max<int64_t>(2 * head.nb, cfg.head.n_fft); break;
        case FV_MODEL_VOCOS: per_frame = std::max<int64_t>(4LL * cnx.max_dim(), std::max<int64_t>(2 * head.nb, cfg.head.n_fft)); break;
        case FV_MODEL_FIREFLY: per_frame = std::max<int64_t>(4LL * cnx.max_dim(), ups.max_elems(1 << 10) >> 10); break;
        case FV_MODEL_REFINEGAN:   // tiled only with seeded noise (reach_frames); cat([x, skip]) at the output rate is the largest tensor
            per_frame = noise_seeded ? refine_max_elems_per_frame(refine) : 0;
            if (per_frame < 1) return 0;
            break;
        default: return 0;
    }
    return (int)std::min<int64_t>((1LL << 29) / std::max<int64_t>(per_frame, 1), 1 << 30);
}
fv_engine::TilePlan fv_engine::tile_plan(int t_in) const {
    TilePlan p;
    const int reach = reach_frames();
    int limit = tile_frame_limit();   // 0 for the models that are never tiled (LOGMEL, RefineGAN without a noise seed)
    if (opt.tile_frames_override > 0) limit = std::min(limit, std::max(opt.tile_frames_override, 4 * reach));
    if (limit <= 0 || t_in <= limit) return p;
    if (limit < 4 * reach) return p;   // (a model whose reach does not fit the span: the per-layer check reports it)
    // The gather / scatter address tiles and clips at exactly frames x hop samples: a model that is not frame-aligned (frame_hop: e.g. a "center"
    // ISTFT head, or odd (kernel - rate) upsamplers) runs whole, and past the addressing span the per-layer check refuses it by name.
    if (frame_hop(limit, t_in, nullptr) < 1) return p;
    p.halo = reach;
    p.L = limit;
    p.stride = p.L - 2 * p.halo;
    // n tiles cover [0, T): the last one is pulled back to end at T
    p.n = (int)(((int64_t)t_in - 2 * p.halo + p.stride - 1) / p.stride);
    if (p.n < 2) p.n = 2;
    return p;
}

// The workspace of a windowed forward: [window input | window template | window output | the model's own workspace], for `item_frames`
// = windows x frames of input at `hop` samples per frame; each of the first three parts is rounded to 64 floats (256 bytes).  Sized and
// carved here only: the tiles build one per call, a stream, a ragged plan and a session pool hold theirs.
struct WindowWorkspace {
    size_t n_in = 0, n_tmpl = 0, n_out = 0;   // floats
    size_t model_bytes = 0;
    WindowWorkspace() = default;
    WindowWorkspace(size_t item_frames, int cin, int cout, int hop, bool tmpl, size_t model_bytes_)
        : n_in(align_up(item_frames * cin, 64)), n_tmpl(tmpl ? align_up(item_frames * hop, 64) : 0), n_out(align_up(item_frames * cout * hop, 64)),
          model_bytes(model_bytes_) {}
    size_t bytes() const { return (n_in + n_tmpl + n_out) * sizeof(float) + model_bytes; }
    struct Parts {
        float *in, *tmpl, *out, *model;   // tmpl: NULL when the generator takes no template
    };
    Parts carve(void* ws) const {
        float* in = (float*)ws;
        float* out = in + n_in + n_tmpl;
        return {in, n_tmpl ? in + n_in : nullptr, out, out + n_out};
    }
    // what `fn` refuses when the caller's workspace is shorter than its `getter` said
    fv_status check(const char* fn, const char* getter, const void* ws, size_t ws_bytes) const {
        if (ws && ws_bytes >= bytes()) return FV_OK;
        set_error("%s: workspace too small (%zu < %zu bytes, %s)", fn, ws ? ws_bytes : (size_t)0, bytes(), getter);
        return FV_ERR_INVALID;
    }
};

// What fv_stream_create, fv_ragged_create and fv_pool_create (`fn`, which wants to `verb`) check first: their arguments, a finalized engine, a
// frame-aligned model.  Clears *out; *hop: the model's samples per frame.
template <class Handle>
static fv_status create_preamble(const fv_engine* e, const void* arg, Handle** out, const char* fn, const char* verb, int* hop) {
    if (!e || !arg || !out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!e->finalized) {
        set_error("%s: call fv_finalize first", fn);
        return FV_ERR_STATE;
    }
    const char* why = nullptr;
    *hop = e->frame_hop(1, 2, &why);
    if (*hop < 1) {
        set_error("%s: this model cannot %s: %s", fn, verb, why);
        return FV_ERR_UNSUPPORTED;
    }
    return FV_OK;
}

// One window length a windowed caller (`fn`, which wants to `verb`) can form: frame-aligned with this hop, and a forward of batch x frames
// fits.  Raises *model_bytes to that forward's workspace (fv_workspace_bytes need not be monotone in t_in: the tile plan switches in at the
// addressing span, so the caller passes every length it can form).
static fv_status admit_window(const fv_engine* e, const char* fn, const char* verb, int hop, int batch, int frames, size_t* model_bytes) {
    const char* why = nullptr;
    if (e->frame_hop(1, frames, &why) != hop) {
        set_error("%s: this model cannot %s: %s (%d-frame window)", fn, verb, why, frames);
        return FV_ERR_UNSUPPORTED;
    }
    const size_t b = fv_workspace_bytes(e, batch, frames);
    if (b == 0) {
        set_error("%s: no forward of %d x %d frames fits (split the batch)", fn, batch, frames);
        return FV_ERR_UNSUPPORTED;
    }
    *model_bytes = std::max(*model_bytes, b);
    return FV_OK;
}

// [input tiles | template tiles | output tiles | the model's own workspace for (batch * n) items of L frames]
static WindowWorkspace tile_workspace(const fv_engine* e, int batch, const fv_engine::TilePlan& tp) {
    const int bn = batch * tp.n;
    const int hop = (int)(fv_output_length(e, tp.L) / tp.L);   // (tile_plan: exactly hop samples per frame)
    return WindowWorkspace((size_t)bn * tp.L, fv_input_channels(e), fv_output_channels(e), hop, e->wants_template(), fv_workspace_bytes(e, bn, tp.L));
}
size_t fv_engine::tile_workspace_bytes(int batch, const TilePlan& tp) const { return tile_workspace(this, batch, tp).bytes(); }

fv_status fv_engine::run_model(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s) {
    const TilePlan tp = tile_plan(t_in);
    if (tp.n <= 1) return run_model_whole(d_in, d_out, batch, t_in, ws, s);
    const int cin = fv_input_channels(this), cout = fv_output_channels(this);
    const int64_t lout = fv_output_length(this, tp.L), clip_out = fv_output_length(this, t_in);
    const int hop = (int)(lout / tp.L);
    const int bn = batch * tp.n;
    const WindowWorkspace::Parts w = tile_workspace(this, batch, tp).carve(ws);
    fv_status st;
    FV_PROF(s, "gather_tiles", 0.0, 8.0 * bn * cin * tp.L, launch_gather_tiles(d_in, w.in, batch, cin, t_in, tp.n, tp.L, tp.stride, 1, s));
    const float* clip_template = cur_template;
    if (cur_template) {
        FV_PROF(s, "gather_tiles", 0.0, 8.0 * bn * lout, launch_gather_tiles(cur_template, w.tmpl, batch, 1, t_in, tp.n, tp.L, tp.stride, hop, s));
        cur_template = w.tmpl;
    }
    // seeded RefineGAN: tile i of a clip draws the clip's noise row at the tile's own start (TilePlan::start), not at a plain multiple
    cur_tile_n = tp.n;
    cur_tile_stride = tp.stride;
    cur_tile_last = t_in - tp.L;
    st = run_model_whole(w.in, w.out, bn, tp.L, w.model, s);
    cur_tile_n = 1;
    cur_tile_stride = cur_tile_last = 0;
    cur_template = clip_template;
    if (st) return st;
    FV_PROF(s, "scatter_tiles", 0.0, 8.0 * batch * cout * clip_out,
            launch_scatter_tiles(w.out, d_out, batch, cout, t_in, tp.n, tp.L, tp.stride, tp.halo, hop, s));
    return FV_OK;
}

// ---- rings: what streams and session pools share ---------------------------------------------------------------------
// What a stream and a session pool share: `rows` sessions (the stream's batch, advancing in lockstep; the pool's slots, each on its own) that
// keep their last `cap` frames in a ring and form windows of at most `cap` frames in the caller's workspace.
struct RingWindows {
    fv_engine* e = nullptr;
    int rows = 0, max_chunk = 0, K = 0, A = 0, cin = 0, cout = 0, hop = 0;
    int64_t cap = 0;              // ring length in frames: K + A + max_chunk, >= every window a session forms
    bool tmpl = false;            // use_template generator: a template ring at the hop rate beside the mel ring
    float* ring = nullptr;        // (rows, C_in, cap), then (rows, 1, cap * hop) for the template: the only device allocation
    float* ring_tmpl = nullptr;
    // The code form (fv_stream_create_codes / fv_codepool_create): the ring holds (rows, n_q, cap) int32 codes in place of the C_in floats
    // per frame, and the window-forming launch decodes them with `vq`'s codebooks (vq.hip); everything else is the float form's.
    const fv_vq* vq = nullptr;
    int n_q = 0;
    size_t ring_bytes = 0;        // of the rings' contents (the allocation rounds the first ring up to 256 bytes)
    int32_t* ring_codes() const { return (int32_t*)ring; }
    WindowWorkspace ws;           // sized for rows x cap frames, and the forward's own workspace for the largest window at batch `rows`
    ~RingWindows() {
        if (ring) (void)hipFree(ring);
    }
    // For `fn`, which calls its rows `rows_name`, past its create_preamble (`hop` is set); context / lookahead: -1 = the reach
    fv_status create(fv_engine* e_, const char* fn, const char* rows_name, int rows_, int max_chunk_, int context, int lookahead,
                     const fv_vq* vq_ = nullptr, int n_q_ = 0) {
        const int R = e_->reach_frames();
        if (rows_ < 1 || max_chunk_ < 1 || context < -1 || lookahead < -1) {
            set_error("%s: %s (%d) and max_chunk_frames (%d) must be >= 1, context_frames (%d) and lookahead_frames (%d) >= 0 "
                      "(-1: the reach, %d frames)", fn, rows_name, rows_, max_chunk_, context, lookahead, R);
            return FV_ERR_INVALID;
        }
        e = e_;
        rows = rows_;
        max_chunk = max_chunk_;
        K = context < 0 ? R : context;
        A = lookahead < 0 ? R : lookahead;
        cin = fv_input_channels(e);
        cout = fv_output_channels(e);
        cap = (int64_t)K + A + max_chunk;
        tmpl = e->wants_template();
        if (cap > (1 << 20)) {
            set_error("%s: context + lookahead + max_chunk_frames = %lld frames, more than 2^20", fn, (long long)cap);
            return FV_ERR_INVALID;
        }
        // Every window length a session can form (1 ... cap frames) must be frame-aligned; the forward's workspace is the largest over them
        size_t model_bytes = 0;
        for (int W = 1; W <= cap; ++W)
            if (const fv_status r = admit_window(e, fn, "stream", hop, rows, W, &model_bytes)) return r;
        const size_t n = (size_t)rows * (size_t)cap;
        ws = WindowWorkspace(n, cin, cout, hop, tmpl, model_bytes);
        vq = vq_;
        n_q = n_q_;
        const size_t ring_ch = vq ? (size_t)n_q : (size_t)cin;   // 4-byte entries per frame of the ring
        const size_t n_ring = align_up(n * ring_ch, 64), n_ring_tmpl = tmpl ? n * hop : 0;
        ring_bytes = (n * ring_ch + n_ring_tmpl) * sizeof(float);
        FV_HIP_CHECK(hipMalloc((void**)&ring, (n_ring + n_ring_tmpl) * sizeof(float)));
        ring_tmpl = tmpl ? ring + n_ring : nullptr;
        return FV_OK;
    }
};

// What fv_stream_create_codes / fv_codepool_create (`fn`) check past their create_preamble: the quantiser, and that it decodes to the
// engine's input channels.
static fv_status admit_vq(const fv_engine* e, const char* fn, const fv_vq* vq, int* n_q) {
    int dim = 0;
    if (const fv_status r = vq_describe(fn, vq, &dim, n_q)) return r;
    if (dim != fv_input_channels(e)) {
        set_error("%s: vq decodes to dim = %d channels, but the engine takes %d input channels", fn, dim, fv_input_channels(e));
        return FV_ERR_INVALID;
    }
    return FV_OK;
}
// A call of the wrong kind on a handle (`fn` on a ring of codes, or its _codes twin on a ring of floats): refused before anything moves
static fv_status check_ring_kind(const RingWindows* h, bool codes_call, const char* fn, const char* float_fn, const char* codes_fn) {
    if ((h->vq != nullptr) == codes_call) return FV_OK;
    if (h->vq)
        set_error("%s: this handle keeps a ring of codes (it was made by a _create_codes entry point): call %s", fn, codes_fn);
    else
        set_error("%s: this handle keeps a ring of floats, not of codes: call %s", fn, float_fn);
    return FV_ERR_STATE;
}

// The emission rule, of a stream and of each session of a pool alike: n more frames arrive at the counters (F, E); the frames [E, E2) are
// emitted out of one forward over the window [w, F2) (vocoder_amd/streaming.py restates it in Python).
struct Emission {
    int64_t F2, E2, w;
};
static inline Emission emission(int64_t F, int64_t E, int64_t n, int K, int A, bool flush) {
    const int64_t F2 = F + n;
    return {F2, flush ? F2 : std::max(E, F2 - A), std::max<int64_t>(0, E - K)};
}

// ---- streaming synthesis ---------------------------------------------------------------------------------------------
// B sessions advance in lockstep.  Host counters: F frames received, E emitted.  A push of n frames appends them (F += n) and emits the frames
// [E, E'), E' = max(E, F - A), out of ONE forward over the window [w, F), w = max(0, E - K); a flush does the same with E' = F.  With K and A
// >= the reach every emitted frame lies >= R frames inside each window edge that is not the utterance's own, so the window reproduces the whole
// utterance's samples there (the rule of the time tiles, tile_plan).  The window is assembled in the caller's workspace at fixed addresses: a
// steady-state push (fixed n: W = K + A + n frames) hands forward_common the same (buffers, batch, frames, stream) as the one before and
// replays its captured graph.
struct fv_stream : RingWindows {
    int64_t F = 0, E = 0;
    bool flushed = false;
    // RefineGAN: the noise seed the stream was created under — its reach, ring and workspace were sized for a seeded engine, and every window
    // draws the noise of its own position in the utterance
    bool seeded = false;
    uint64_t seed = 0;
    int32_t first_row = 0;
};

// d_in: the chunk — (B, C_in, n) floats, or with `codes` (n_q, B, n) int32 codes for a stream that keeps a ring of codes
static fv_status stream_step(fv_stream* st, const void* d_in, bool codes, const float* d_template, int32_t n, bool flush, float* d_out,
                             int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = flush ? "fv_stream_flush" : codes ? "fv_stream_push_codes" : "fv_stream_push";
    if (frames_out) *frames_out = 0;
    if (!st || !frames_out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (!flush)
        if (const fv_status r = check_ring_kind(st, codes, fn, "fv_stream_push", "fv_stream_push_codes")) return r;
    if (st->flushed) {
        set_error("%s: the stream was flushed; fv_stream_reset it before the next utterance", fn);
        return FV_ERR_STATE;
    }
    if (!flush) {
        if (n < 0 || n > st->max_chunk) {
            set_error("%s: %d frames, more than max_chunk_frames = %d of this stream", fn, n, st->max_chunk);
            return FV_ERR_INVALID;
        }
        if (n == 0) return FV_OK;
        if (!d_in) {
            set_error("%s: null %s chunk", fn, codes ? "code" : "mel");
            return FV_ERR_INVALID;
        }
        if (st->tmpl && !d_template) {
            set_error("%s: the generator was built with use_template=True and every push needs a template chunk (B, 1, n*hop)", fn);
            return FV_ERR_INVALID;
        }
        if (!st->tmpl && d_template) {
            set_error("%s: template given but the generator was built with use_template=False", fn);
            return FV_ERR_INVALID;
        }
    }
    if (st->seeded && !(st->e->noise_seeded && st->e->noise_seed == st->seed && st->e->noise_first_row == st->first_row)) {
        set_error("%s: the engine's noise seed was cleared or changed since this RefineGAN stream was created: create a new stream", fn);
        return FV_ERR_STATE;
    }
    if (const fv_status r = st->ws.check(fn, "fv_stream_workspace_bytes", d_workspace, workspace_bytes)) return r;
    const Emission em = emission(st->F, st->E, flush ? 0 : n, st->K, st->A, flush);
    const int64_t F = em.F2, E2 = em.E2;
    const bool emit = E2 > st->E;
    if (emit && !d_out) {
        set_error("%s: null output (this call emits %lld frames)", fn, (long long)(E2 - st->E));
        return FV_ERR_INVALID;
    }
    fv_engine* e = st->e;
    const int B = st->rows, hop = st->hop;
    const int64_t w = emit ? em.w : st->F;   // no emission: the chunk only goes into the ring
    hipStream_t s = (hipStream_t)stream;
    const WindowWorkspace::Parts win = st->ws.carve(d_workspace);
    const ProfScope prof(e);
    if (!flush || emit) {
        // the chunk into the ring at F mod cap, and the window [w, F) beside it; a flush has no chunk (n = 0: the window comes from the ring alone)
        const int64_t nc = flush ? 0 : n, W = F - w;
        if (st->vq)   // the ring holds codes: the window is decoded from them on the way (W x n_q codes in, W x C_in floats out)
            FV_PROF(s, "stream_window_codes", 0.0, 4.0 * B * (st->n_q * (2.0 * nc + (emit ? 1.0 * W : 0.0)) + (emit ? 1.0 * W * st->cin * (1 + st->n_q) : 0.0)),
                    launch_stream_window_codes(st->vq, (const int*)d_in, st->ring_codes(), emit ? win.in : nullptr, B, st->cap, st->F, nc, w, s));
        else
            FV_PROF(s, "stream_window", 0.0, 4.0 * B * st->cin * (2.0 * nc + (emit ? 2.0 * W : 0.0)),
                    launch_stream_window((const float*)d_in, st->ring, emit ? win.in : nullptr, B, st->cin, st->cap, st->F, nc, w, s));
        if (st->tmpl)
            FV_PROF(s, "stream_window", 0.0, 4.0 * B * hop * (2.0 * nc + (emit ? 2.0 * W : 0.0)),
                    launch_stream_window(d_template, st->ring_tmpl, emit ? win.tmpl : nullptr, B, 1, st->cap * hop, st->F * hop, nc * hop, w * hop, s));
    }
    if (emit) {
        const int W = (int)(F - w);
        // seeded RefineGAN: the window [w, F) draws the utterance's noise at w (the key of a captured graph holds w: steady-state pushes run eagerly)
        const fv_status r = forward_common(e, win.in, win.tmpl, nullptr, win.out, B, W, win.model, st->ws.model_bytes, stream, st->seeded, w);
        if (r) return r;
        const int64_t len = (E2 - st->E) * hop;
        FV_PROF(s, "stream_crop", 0.0, 8.0 * B * st->cout * len,
                launch_stream_crop(win.out, d_out, B, st->cout, (int64_t)W * hop, (st->E - w) * hop, len, s));
    }
    *frames_out = E2 - st->E;
    st->F = F;
    st->E = E2;
    if (flush) st->flushed = true;
    return FV_OK;
}

extern "C" {

FV_API int32_t fv_reach_frames(const fv_engine* e) {
    if (!e || !e->finalized || e->frame_hop(1, 2, nullptr) < 1) return -1;
    return e->reach_frames();
}

static fv_status stream_create(fv_engine* e, const fv_vq* vq, bool codes, const fv_stream_config* cfg, fv_stream** out) {
    const char* fn = codes ? "fv_stream_create_codes" : "fv_stream_create";
    std::unique_ptr<fv_stream> st(new fv_stream());
    if (const fv_status r = create_preamble(e, cfg, out, fn, "stream", &st->hop)) return r;
    int n_q = 0;
    if (codes)
        if (const fv_status r = admit_vq(e, fn, vq, &n_q)) return r;
    if (const fv_status r = st->create(e, fn, "batch", cfg->batch, cfg->max_chunk_frames, cfg->context_frames, cfg->lookahead_frames, vq, n_q))
        return r;
    if (e->cfg.model == FV_MODEL_REFINEGAN) {
        st->seeded = true;
        st->seed = e->noise_seed;
        st->first_row = e->noise_first_row;
    }
    *out = st.release();
    return FV_OK;
}

FV_API fv_status fv_stream_create(fv_engine* e, const fv_stream_config* cfg, fv_stream** out) { return stream_create(e, nullptr, false, cfg, out); }

FV_API fv_status fv_stream_create_codes(fv_engine* e, const fv_vq* vq, const fv_stream_config* cfg, fv_stream** out) {
    return stream_create(e, vq, true, cfg, out);
}

FV_API size_t fv_stream_ring_bytes(const fv_stream* s) { return s ? s->ring_bytes : 0; }

FV_API size_t fv_stream_workspace_bytes(const fv_stream* s) { return s ? s->ws.bytes() : 0; }

FV_API int64_t fv_stream_pending_frames(const fv_stream* s) { return s ? s->F - s->E : 0; }

FV_API fv_status fv_stream_push(fv_stream* s, const float* d_mel, const float* d_template, int32_t n, float* d_out, int64_t* frames_out,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    return stream_step(s, d_mel, false, d_template, n, false, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_stream_push_codes(fv_stream* s, const int32_t* d_codes, const float* d_template, int32_t n, float* d_out,
                                      int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    return stream_step(s, d_codes, true, d_template, n, false, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_stream_flush(fv_stream* s, float* d_out, int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    return stream_step(s, nullptr, false, nullptr, 0, true, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_stream_reset(fv_stream* s) {
    if (!s) {
        set_error("fv_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->F = s->E = 0;
    s->flushed = false;
    return FV_OK;
}

FV_API void fv_stream_destroy(fv_stream* s) { delete s; }

}  // extern "C"

// ---- ragged batches ----------------------------------------------------------------------------------------------------
// The plan (include/fishvoc.h states it; vocoder_amd/ragged.py restates it in Python, and the tests compare the two window for window).
static constexpr int kRaggedLaunchFrames = 192, kRaggedMaxGroups = 8;

static fv_status ragged_plan(int reach, const int32_t* lengths, int batch, int launch_frames, int max_groups, std::vector<fv_ragged_window>& out) {
    out.clear();
    if (reach < 1 || reach > (1 << 20) || !lengths || batch < 1) {
        set_error("fv_ragged_plan: reach (%d) and batch (%d) must be >= 1 and the lengths given", reach, batch);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 0) {
            set_error("fv_ragged_plan: negative length %d of clip %d", lengths[b], b);
            return FV_ERR_INVALID;
        }
    if (launch_frames <= 0) launch_frames = kRaggedLaunchFrames;
    if (max_groups <= 0) max_groups = kRaggedMaxGroups;
    const int R2 = 2 * reach;
    std::vector<std::pair<int, int>> lng;   // (T, b) of the long clips, ascending
    for (int b = 0; b < batch; ++b)
        if (lengths[b] > R2) lng.emplace_back(lengths[b], b);
    std::sort(lng.begin(), lng.end());
    const int m = (int)lng.size();
    struct Item {
        int n, b, a, lo, hi;
    };
    std::vector<Item> items;
    if (m > 0) {
        // f[k][j]: the least cost of the first j clips in exactly k runs; a run [i, j) costs (j - i) Tg + 2R #{T < Tg} + launch_frames
        const int K = std::min(max_groups, m);
        const int64_t INF = (int64_t)1 << 62;
        std::vector<int> first_eq(m);   // first index of the block of equal lengths that clip j belongs to
        for (int j = 0; j < m; ++j) first_eq[j] = (j > 0 && lng[j].first == lng[j - 1].first) ? first_eq[j - 1] : j;
        std::vector<std::vector<int64_t>> f(K + 1, std::vector<int64_t>(m + 1, INF));
        std::vector<std::vector<int>> arg(K + 1, std::vector<int>(m + 1, -1));
        f[0][0] = 0;
        for (int k = 1; k <= K; ++k)
            for (int j = k; j <= m; ++j) {
                if (j < m && lng[j].first == lng[j - 1].first) continue;   // no cut between two clips of one length
                for (int i = k - 1; i < j; ++i) {
                    if (f[k - 1][i] >= INF) continue;
                    const int64_t c = f[k - 1][i] + (int64_t)(j - i) * lng[j - 1].first + (int64_t)R2 * std::max(0, first_eq[j - 1] - i) + launch_frames;
                    if (c < f[k][j]) {   // strict: the earliest start wins a tie
                        f[k][j] = c;
                        arg[k][j] = i;
                    }
                }
            }
        int best = 1;
        for (int k = 2; k <= K; ++k)
            if (f[k][m] < f[best][m]) best = k;   // strict: the fewest runs win a tie
        for (int k = best, j = m; k >= 1; --k) {
            const int i = arg[k][j], tg = lng[j - 1].first;
            for (int t = i; t < j; ++t) {
                const int T = lng[t].first, b = lng[t].second;
                if (T == tg) {
                    items.push_back({tg, b, 0, 0, T});
                } else {
                    items.push_back({tg, b, 0, 0, T - reach});
                    items.push_back({R2, b, T - R2, T - reach, T});
                }
            }
            j = i;
        }
    }
    for (int b = 0; b < batch; ++b)
        if (lengths[b] >= 1 && lengths[b] <= R2) items.push_back({lengths[b], b, 0, 0, lengths[b]});
    std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.n != y.n ? x.n > y.n : x.b < y.b; });
    int group = -1, prev = -1;
    for (const Item& it : items) {
        if (it.n != prev) {
            ++group;
            prev = it.n;
        }
        out.push_back({it.b, it.a, it.n, it.lo, it.hi, group});
    }
    return FV_OK;
}

struct fv_ragged {
    fv_engine* e = nullptr;
    int B = 0, t_max = 0, cin = 0, cout = 0, hop = 0, min_len = 0;
    bool tmpl = false;
    std::vector<fv_ragged_window> win;
    struct Group {
        int first, count, frames;
    };
    std::vector<Group> groups;
    fv_ragged_window* d_win = nullptr;   // the window table, then the lengths: the plan's only device allocation
    int32_t* d_len = nullptr;
    WindowWorkspace ws;                  // sized for the largest group, and the largest group's own workspace
    ~fv_ragged() {
        if (d_win) (void)hipFree(d_win);
    }
};

static int32_t copy_windows(const std::vector<fv_ragged_window>& w, fv_ragged_window* out, int32_t cap) {
    if (out && cap > 0) std::copy(w.begin(), w.begin() + std::min<size_t>(w.size(), (size_t)cap), out);
    return (int32_t)w.size();
}

extern "C" {

FV_API int32_t fv_ragged_plan(int32_t reach, const int32_t* host_lengths, int32_t batch, int32_t launch_frames, int32_t max_groups,
                              fv_ragged_window* out, int32_t cap) {
    std::vector<fv_ragged_window> w;
    if (const fv_status st = ragged_plan(reach, host_lengths, batch, launch_frames, max_groups, w)) return st;
    if (cap < 0 || (cap > 0 && !out)) {
        set_error("fv_ragged_plan: cap = %d without room for it", cap);
        return FV_ERR_INVALID;
    }
    return copy_windows(w, out, cap);
}

FV_API fv_status fv_ragged_create(fv_engine* e, const int32_t* host_lengths, int32_t batch, int32_t t_max, int32_t launch_frames,
                                  int32_t max_groups, fv_ragged** out) {
    int hop = 0;
    if (const fv_status st = create_preamble(e, host_lengths, out, "fv_ragged_create", "run ragged batches", &hop)) return st;
    if (e->cfg.model == FV_MODEL_REFINEGAN) {
        set_error("fv_ragged_create: this model cannot run ragged batches: the windows of a RefineGAN batch start at per-row origins, and its "
                  "seeded AdaIN noise takes one (origin, stride) per launch");
        return FV_ERR_UNSUPPORTED;
    }
    if (batch < 1 || t_max < 1) {
        set_error("fv_ragged_create: batch (%d) and t_max (%d) must be >= 1", batch, t_max);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > t_max) {
            set_error("fv_ragged_create: length %d of clip %d is outside [0, t_max = %d]", host_lengths[b], b, t_max);
            return FV_ERR_INVALID;
        }
    std::unique_ptr<fv_ragged> p(new fv_ragged());
    p->e = e;
    p->B = batch;
    p->t_max = t_max;
    p->cin = fv_input_channels(e);
    p->cout = fv_output_channels(e);
    p->hop = hop;
    p->tmpl = e->wants_template();
    p->min_len = *std::min_element(host_lengths, host_lengths + batch);
    if (const fv_status st = ragged_plan(e->reach_frames(), host_lengths, batch, launch_frames, max_groups, p->win)) return st;
    size_t max_items = 0, model_bytes = 0;
    for (int i = 0; i < (int)p->win.size(); ++i) {
        const fv_ragged_window& w = p->win[i];
        // what the kernels rely on: the window starts inside the clip and its kept frames lie inside the window and the clip
        if (w.start < 0 || w.start >= host_lengths[w.clip] || w.keep_lo < w.start || w.keep_hi > std::min(w.start + w.frames, host_lengths[w.clip]) ||
            w.keep_lo >= w.keep_hi) {
            set_error("fv_ragged_create: internal error, window %d of the plan is malformed", i);
            return FV_ERR_STATE;
        }
        if (p->groups.empty() || w.group != (int)p->groups.size() - 1) p->groups.push_back({i, 0, w.frames});
        p->groups.back().count++;
    }
    for (const auto& g : p->groups) {
        if (const fv_status st = admit_window(e, "fv_ragged_create", "run ragged batches", hop, g.count, g.frames, &model_bytes)) return st;
        max_items = std::max(max_items, (size_t)g.count * g.frames);
    }
    p->ws = WindowWorkspace(max_items, p->cin, p->cout, hop, p->tmpl, model_bytes);
    const size_t wbytes = align_up(p->win.size() * sizeof(fv_ragged_window), 256);
    FV_HIP_CHECK(hipMalloc((void**)&p->d_win, wbytes + (size_t)batch * sizeof(int32_t)));
    p->d_len = (int32_t*)((char*)p->d_win + wbytes);
    if (!p->win.empty()) FV_HIP_CHECK(hipMemcpy(p->d_win, p->win.data(), p->win.size() * sizeof(fv_ragged_window), hipMemcpyHostToDevice));
    FV_HIP_CHECK(hipMemcpy(p->d_len, host_lengths, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = p.release();
    return FV_OK;
}

FV_API size_t fv_ragged_workspace_bytes(const fv_ragged* p) { return p ? p->ws.bytes() : 0; }

FV_API int32_t fv_ragged_num_groups(const fv_ragged* p) { return p ? (int32_t)p->groups.size() : 0; }

FV_API int32_t fv_ragged_group(const fv_ragged* p, int32_t g, int32_t* batch, int32_t* frames) {
    if (!p || g < 0 || g >= (int32_t)p->groups.size()) {
        set_error("fv_ragged_group: no group %d", g);
        return FV_ERR_INVALID;
    }
    if (batch) *batch = p->groups[g].count;
    if (frames) *frames = p->groups[g].frames;
    return FV_OK;
}

FV_API int32_t fv_ragged_windows(const fv_ragged* p, fv_ragged_window* out, int32_t cap) {
    if (!p || cap < 0 || (cap > 0 && !out)) {
        set_error("fv_ragged_windows: null argument");
        return FV_ERR_INVALID;
    }
    return copy_windows(p->win, out, cap);
}

FV_API fv_status fv_ragged_forward(fv_ragged* p, const float* d_in, const float* d_template, float* d_out, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!p || !d_in || !d_out) {
        set_error("fv_ragged_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (const fv_status st = p->ws.check("fv_ragged_forward", "fv_ragged_workspace_bytes", d_workspace, workspace_bytes)) return st;
    fv_engine* e = p->e;
    if (const fv_status st = check_template(e, d_template)) return st;   // (up front: a batch of empty clips runs no forward that would check it)
    const WindowWorkspace::Parts win = p->ws.carve(d_workspace);
    for (const auto& g : p->groups)   // everything is checked before anything is enqueued
        if (const fv_status st = check_forward(e, win.in, win.tmpl, win.out, g.count, g.frames, win.model, p->ws.model_bytes)) return st;
    hipStream_t s = (hipStream_t)stream;
    const int hop = p->hop;
    const long long T = p->t_max;
    const ForwardScope scope(e, nullptr, nullptr);
    for (const auto& g : p->groups) {
        const long long n = g.frames;
        FV_PROF(s, "ragged_gather", 0.0, 8.0 * g.count * p->cin * n,
                launch_ragged_gather(d_in, win.in, p->d_win, p->d_len, g.first, g.count, p->cin, T, n, 1, s));
        if (p->tmpl)
            FV_PROF(s, "ragged_gather", 0.0, 8.0 * g.count * n * hop,
                    launch_ragged_gather(d_template, win.tmpl, p->d_win, p->d_len, g.first, g.count, 1, T * hop, n * hop, hop, s));
        e->cur_template = win.tmpl;
        // eagerly, past forward_common's graph bookkeeping: a ragged call neither evicts a captured graph nor resets the last key
        const fv_status st = e->run_model(win.in, win.out, g.count, g.frames, win.model, s);
        if (st) return st;
        FV_PROF(s, "ragged_scatter", 0.0, 8.0 * g.count * p->cout * n * hop,
                launch_ragged_scatter(win.out, d_out, p->d_win, g.first, g.count, p->cout, T * hop, n * hop, hop, s));
    }
    FV_PROF(s, "ragged_zero_tail", 0.0, 4.0 * p->B * p->cout * (double)(p->t_max - p->min_len) * hop,
            launch_ragged_zero_tail(d_out, p->d_len, p->B, p->cout, T * hop, (long long)(p->t_max - p->min_len) * hop, hop, s));
    return FV_OK;
}

FV_API void fv_ragged_destroy(fv_ragged* p) { delete p; }

}  // extern "C"

// ---- session pool: streaming sessions that advance independently ---------------------------------------------------------
// The plan (include/fishvoc.h states it; vocoder_amd/sessions.py restates it in Python, and the tests compare the two row for row).  Per
// item the counters move as stream_step moves them; the rows are then placed in groups: group 0 aligns every row against the tensor edge it
// owns, the whole short utterances that would not fill it run in groups of their own length.
struct PoolPlan {
    std::vector<fv_pool_row> rows;               // by group, then by item
    std::vector<int32_t> group_rows, group_frames;
    std::vector<int64_t> F2, E2;                 // per item: the session's counters after the step
    std::vector<char> seen;                      // per session (scratch of the duplicate check)
    std::vector<fv_pool_row> cand;               // scratch: the rows in item order
};

static fv_status pool_plan(const char* fn, int S, int max_chunk, int K, int A, const int64_t* F, const int64_t* E, const int32_t* flushed,
                           const fv_pool_item* items, int count, int in_frames, int out_frames, PoolPlan& p) {
    p.rows.clear();
    p.group_rows.clear();
    p.group_frames.clear();
    p.cand.clear();
    if (S < 1 || max_chunk < 1 || K < 0 || A < 0 || (int64_t)K + A + max_chunk > (1 << 20)) {
        set_error("%s: sessions (%d) and max_chunk_frames (%d) must be >= 1, context_frames (%d) and lookahead_frames (%d) >= 0, and their "
                  "sum with max_chunk_frames at most 2^20", fn, S, max_chunk, K, A);
        return FV_ERR_INVALID;
    }
    if (count < 0 || !F || !E || (count > 0 && !items)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    p.seen.assign((size_t)S, 0);
    p.F2.assign((size_t)count, 0);
    p.E2.assign((size_t)count, 0);
    int max_n = 0;
    int64_t max_emit = 0, Wg = 0;
    for (int i = 0; i < count; ++i) {
        const fv_pool_item& it = items[i];
        if (it.session < 0 || it.session >= S) {
            set_error("%s: item %d names session %d, outside [0, %d)", fn, i, it.session, S);
            return FV_ERR_INVALID;
        }
        if (p.seen[(size_t)it.session]) {
            set_error("%s: duplicate session %d (item %d): a session appears at most once per step", fn, it.session, i);
            return FV_ERR_INVALID;
        }
        p.seen[(size_t)it.session] = 1;
        if (it.frames < 0 || it.frames > max_chunk) {
            set_error("%s: item %d has %d frames, outside [0, max_chunk_frames = %d]", fn, i, it.frames, max_chunk);
            return FV_ERR_INVALID;
        }
        const int64_t f = F[it.session], e = E[it.session];
        if (f < 0 || e < 0 || e > f) {
            set_error("%s: invalid counters of session %d (F = %lld, E = %lld)", fn, it.session, (long long)f, (long long)e);
            return FV_ERR_INVALID;
        }
        if (flushed && flushed[it.session]) {
            set_error("%s: session %d was flushed (item %d); fv_pool_reset it before the next utterance", fn, it.session, i);
            return FV_ERR_STATE;
        }
        const Emission em = emission(f, e, it.frames, K, A, it.flush != 0);
        const int64_t f2 = em.F2, e2 = em.E2;
        p.F2[(size_t)i] = f2;
        p.E2[(size_t)i] = e2;
        max_n = std::max(max_n, it.frames);
        max_emit = std::max(max_emit, e2 - e);
        if (e2 > e) {
            p.cand.push_back({i, 0, 0, (int32_t)(f2 - em.w), em.w, e, e2});
            Wg = std::max(Wg, f2 - em.w);
        }
    }
    if (in_frames >= 0 && in_frames < max_n) {
        set_error("%s: in_frames = %d, but an item of this step has %d frames", fn, in_frames, max_n);
        return FV_ERR_INVALID;
    }
    if (out_frames >= 0 && out_frames < max_emit) {
        set_error("%s: out_frames = %d, but an item of this step emits %lld frames", fn, out_frames, (long long)max_emit);
        return FV_ERR_INVALID;
    }
    if (p.cand.empty()) return FV_OK;
    // group 0: every row but the whole utterances shorter than Wg; a row that does not own its left edge is right-aligned
    auto whole_short = [&](const fv_pool_row& r) { return r.w == 0 && items[r.item].flush && r.frames < Wg; };
    for (fv_pool_row r : p.cand)
        if (!whole_short(r)) {
            r.col0 = r.w == 0 ? 0 : (int32_t)(Wg - r.frames);
            p.rows.push_back(r);
        }
    p.group_rows.push_back((int32_t)p.rows.size());
    p.group_frames.push_back((int32_t)Wg);
    // the rest by exact length, descending; item order within a length
    const size_t first_short = p.rows.size();
    for (const fv_pool_row& r : p.cand)
        if (whole_short(r)) p.rows.push_back(r);
    std::stable_sort(p.rows.begin() + (ptrdiff_t)first_short, p.rows.end(),
                     [](const fv_pool_row& a, const fv_pool_row& b) { return a.frames > b.frames; });
    for (size_t i = first_short; i < p.rows.size(); ++i) {
        if (i == first_short || p.rows[i].frames != p.rows[i - 1].frames) {
            p.group_rows.push_back(0);
            p.group_frames.push_back(p.rows[i].frames);
        }
        p.rows[i].group = (int32_t)p.group_rows.size() - 1;
        p.group_rows.back()++;
    }
    return FV_OK;
}

struct fv_pool : RingWindows {
    std::vector<int64_t> F, E;    // per session
    std::vector<int32_t> flushed;
    PoolPlan plan;                // the step's plan and launch tables: host vectors that keep their capacity from step to step
    std::vector<PoolGatherEntry> gather;
    std::vector<PoolCropEntry> crop;
};

extern "C" {

FV_API int32_t fv_pool_plan(const fv_pool_config* cfg, const int64_t* received, const int64_t* emitted, const int32_t* flushed,
                            const fv_pool_item* items, int32_t count, int32_t in_frames, int32_t out_frames, fv_pool_row* rows,
                            int32_t row_cap, int32_t* group_rows, int32_t* group_frames, int32_t group_cap, int32_t* num_groups) {
    if (num_groups) *num_groups = 0;
    if (!cfg || row_cap < 0 || group_cap < 0 || (row_cap > 0 && !rows) || (group_cap > 0 && (!group_rows || !group_frames))) {
        set_error("fv_pool_plan: null argument, or a capacity without room for it");
        return FV_ERR_INVALID;
    }
    PoolPlan p;
    if (const fv_status st = pool_plan("fv_pool_plan", cfg->sessions, cfg->max_chunk_frames, cfg->context_frames, cfg->lookahead_frames, received,
                                       emitted, flushed, items, count, in_frames, out_frames, p))
        return st;
    std::copy(p.rows.begin(), p.rows.begin() + (ptrdiff_t)std::min<size_t>(p.rows.size(), (size_t)row_cap), rows);
    const ptrdiff_t ng = (ptrdiff_t)std::min<size_t>(p.group_rows.size(), (size_t)group_cap);
    std::copy(p.group_rows.begin(), p.group_rows.begin() + ng, group_rows);
    std::copy(p.group_frames.begin(), p.group_frames.begin() + ng, group_frames);
    if (num_groups) *num_groups = (int32_t)p.group_rows.size();
    return (int32_t)p.rows.size();
}

static fv_status pool_create(fv_engine* e, const fv_vq* vq, bool codes, const fv_pool_config* cfg, fv_pool** out) {
    const char* fn = codes ? "fv_codepool_create" : "fv_pool_create";
    std::unique_ptr<fv_pool> p(new fv_pool());
    if (const fv_status r = create_preamble(e, cfg, out, fn, "stream", &p->hop)) return r;
    if (e->cfg.model == FV_MODEL_REFINEGAN) {
        set_error("%s: this model cannot run session pools: the sessions of a RefineGAN pool advance to per-row origins, and its "
                  "seeded AdaIN noise takes one (origin, stride) per launch", fn);
        return FV_ERR_UNSUPPORTED;
    }
    int n_q = 0;
    if (codes)
        if (const fv_status r = admit_vq(e, fn, vq, &n_q)) return r;
    if (const fv_status r = p->create(e, fn, "sessions", cfg->sessions, cfg->max_chunk_frames, cfg->context_frames, cfg->lookahead_frames, vq, n_q))
        return r;
    const size_t S = (size_t)p->rows;
    p->F.assign(S, 0);
    p->E.assign(S, 0);
    p->flushed.assign(S, 0);
    p->gather.reserve(S);
    p->crop.reserve(S);
    *out = p.release();
    return FV_OK;
}

FV_API fv_status fv_pool_create(fv_engine* e, const fv_pool_config* cfg, fv_pool** out) { return pool_create(e, nullptr, false, cfg, out); }

FV_API fv_status fv_codepool_create(fv_engine* e, const fv_vq* vq, const fv_pool_config* cfg, fv_pool** out) {
    return pool_create(e, vq, true, cfg, out);
}

FV_API size_t fv_codepool_ring_bytes(const fv_pool* p) { return p ? p->ring_bytes : 0; }

FV_API size_t fv_pool_workspace_bytes(const fv_pool* p) { return p ? p->ws.bytes() : 0; }

FV_API int64_t fv_pool_pending_frames(const fv_pool* p, int32_t session) {
    return p && session >= 0 && session < p->rows ? p->F[(size_t)session] - p->E[(size_t)session] : 0;
}

// d_chunks: (count, C_in, in_frames) floats, or with `codes` (n_q, count, in_frames) int32 codes for a pool that keeps rings of codes
static fv_status pool_step(fv_pool* p, const fv_pool_item* items, int32_t count, const void* d_chunks, bool codes, const float* d_templates,
                           int32_t in_frames, float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
    const char* fn = codes ? "fv_codepool_step" : "fv_pool_step";
    if (!p || count < 0 || (count > 0 && !items) || in_frames < 0 || out_frames < 0) {
        set_error("%s: null argument, or a negative count, in_frames or out_frames", fn);
        return FV_ERR_INVALID;
    }
    // ---- the whole step is checked before any counter moves or anything is enqueued ----
    if (const fv_status st = check_ring_kind(p, codes, fn, "fv_pool_step", "fv_codepool_step")) return st;
    PoolPlan& pl = p->plan;
    if (const fv_status st = pool_plan(fn, p->rows, p->max_chunk, p->K, p->A, p->F.data(), p->E.data(), p->flushed.data(), items, count,
                                       in_frames, out_frames, pl))
        return st;
    bool any_frames = false;
    for (int i = 0; i < count; ++i) any_frames |= items[i].frames > 0;
    if (any_frames && !d_chunks) {
        set_error("%s: null chunk buffer, but an item of this step has frames", fn);
        return FV_ERR_INVALID;
    }
    if (any_frames && p->tmpl && !d_templates) {
        set_error("%s: the generator was built with use_template=True and every chunk needs a template chunk (count, 1, in_frames*hop)", fn);
        return FV_ERR_INVALID;
    }
    if (!p->tmpl && d_templates) {
        set_error("%s: template given but the generator was built with use_template=False", fn);
        return FV_ERR_INVALID;
    }
    if (count > 0 && out_frames > 0 && !d_out) {
        set_error("%s: null output (out_frames = %d)", fn, out_frames);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = p->ws.check(fn, "fv_pool_workspace_bytes", d_workspace, workspace_bytes)) return st;
    fv_engine* e = p->e;
    const WindowWorkspace::Parts win = p->ws.carve(d_workspace);
    const int G = (int)pl.group_rows.size();
    for (int g = 0; g < G; ++g)
        if (const fv_status st = check_forward(e, win.in, win.tmpl, win.out, pl.group_rows[g], pl.group_frames[g], win.model, p->ws.model_bytes))
            return st;
    // ---- enqueue: per group gather -> forward -> crop; the first gather also files the chunks of the items that emit nothing, the first crop
    //      also zeroes their output rows (with no group at all, one launch of each does only that) ----
    hipStream_t s = (hipStream_t)stream;
    const int hop = p->hop;
    const ProfScope prof(e);
    std::vector<char>& has_row = pl.seen;   // reused as: item i has a row
    has_row.assign((size_t)count, 0);
    for (const fv_pool_row& r : pl.rows) has_row[(size_t)r.item] = 1;
    size_t r0 = 0;
    for (int g = 0; g < std::max(G, 1); ++g) {
        const int rows = G ? pl.group_rows[g] : 0;
        const long long Wg = G ? pl.group_frames[g] : 0;
        p->gather.clear();
        p->crop.clear();
        for (int k = 0; k < rows; ++k) {
            const fv_pool_row& r = pl.rows[r0 + (size_t)k];
            const fv_pool_item& it = items[r.item];
            p->gather.push_back({r.item, it.session, k, r.col0, r.frames, it.frames, r.w, p->F[(size_t)it.session]});
            p->crop.push_back({r.item, k, r.col0 + (r.emit_lo - r.w), r.emit_hi - r.emit_lo});
        }
        if (g == 0)
            for (int i = 0; i < count; ++i)
                if (!has_row[(size_t)i]) {
                    if (items[i].frames > 0) p->gather.push_back({i, items[i].session, -1, 0, 0, items[i].frames, 0, p->F[(size_t)items[i].session]});
                    p->crop.push_back({i, -1, 0, 0});
                }
        const int ng = (int)p->gather.size(), nc = (int)p->crop.size();
        if (p->vq)   // the rings hold codes: the group's tensor is decoded from them on the way
            FV_PROF(s, "pool_gather_codes", 0.0, 4.0 * rows * Wg * (p->n_q + (double)p->cin * (1 + p->n_q)),
                    launch_pool_gather_codes(p->vq, (const int*)d_chunks, p->ring_codes(), win.in, p->gather.data(), ng, count, p->cap, in_frames, Wg, s));
        else
            FV_PROF(s, "pool_gather", 0.0, 8.0 * rows * p->cin * Wg,
                    launch_pool_gather((const float*)d_chunks, p->ring, win.in, p->gather.data(), ng, p->cin, p->cap, in_frames, Wg, 1, s));
        if (p->tmpl)
            FV_PROF(s, "pool_gather", 0.0, 8.0 * rows * Wg * hop,
                    launch_pool_gather(d_templates, p->ring_tmpl, win.tmpl, p->gather.data(), ng, 1, p->cap, in_frames, Wg, hop, s));
        if (rows > 0) {
            if (g == 0) {
                // fixed addresses: a steady state with the same rows and the same Wg repeats its key and replays the captured graph
                if (const fv_status st = forward_common(e, win.in, win.tmpl, nullptr, win.out, rows, (int)Wg, win.model, p->ws.model_bytes, stream))
                    return st;
            } else {
                // eagerly, past forward_common's graph bookkeeping (as the groups of a ragged batch)
                const ForwardScope scope(e, win.tmpl, nullptr);
                if (const fv_status st = e->run_model(win.in, win.out, rows, (int)Wg, win.model, s)) return st;
            }
        }
        FV_PROF(s, "pool_crop", 0.0, 4.0 * nc * p->cout * (double)out_frames * hop,
                launch_pool_crop(win.out, d_out, p->crop.data(), nc, p->cout, Wg, out_frames, hop, s));
        r0 += (size_t)rows;
    }
    // ---- the counters move ----
    for (int i = 0; i < count; ++i) {
        const size_t sess = (size_t)items[i].session;
        if (frames_out) frames_out[i] = pl.E2[(size_t)i] - p->E[sess];
        p->F[sess] = pl.F2[(size_t)i];
        p->E[sess] = pl.E2[(size_t)i];
        if (items[i].flush) p->flushed[sess] = 1;
    }
    return FV_OK;
}

FV_API fv_status fv_pool_step(fv_pool* p, const fv_pool_item* items, int32_t count, const float* d_chunks, const float* d_templates,
                              int32_t in_frames, float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace,
                              size_t workspace_bytes, void* stream) {
    return pool_step(p, items, count, d_chunks, false, d_templates, in_frames, d_out, out_frames, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_codepool_step(fv_pool* p, const fv_pool_item* items, int32_t count, const int32_t* d_codes, const float* d_templates,
                                    int32_t in_frames, float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
    return pool_step(p, items, count, d_codes, true, d_templates, in_frames, d_out, out_frames, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_pool_reset(fv_pool* p, int32_t session) {
    if (!p || session < 0 || session >= p->rows) {
        set_error("fv_pool_reset: no session %d", (int)session);
        return FV_ERR_INVALID;
    }
    p->F[(size_t)session] = p->E[(size_t)session] = 0;
    p->flushed[(size_t)session] = 0;
    return FV_OK;
}

FV_API void fv_pool_destroy(fv_pool* p) { delete p; }

}  // extern "C"
