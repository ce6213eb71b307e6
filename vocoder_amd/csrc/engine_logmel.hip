// The log-mel front-end on rows of different lengths and on chunks of a stream (fv_logmel_*, include/fishvoc.h): what
// fish_vocoder/data/transforms/spectrogram.py:25-104 computes for whole, equal-length rows and test.py:64-71 calls once per file.
// Only the first step differs from fv_forward on a log-mel engine: logmel_window_kernel (frame_kernels.hip) writes the polyphase signal of
// the frames [f0, f0 + n) with per-row edges; behind it the forward's own tail runs unchanged (fv_engine::run_logmel_tail).  These entries
// enqueue eagerly and leave the engine's captured graphs and their bookkeeping alone.
#include <memory>

#include "engine_internal.h"
#include "sample_stream.h"

static constexpr int64_t kLogmelMaxLen = kSampleStreamMaxLen;   // N hop stays far inside 64 bits

static int64_t logmel_frames(const fv_logmel_config& c, int64_t L) {
    const int64_t pad = c.win_length - c.hop_length;   // pad_l + pad_r
    return L + pad >= c.n_fft ? 1 + (L + pad - c.n_fft) / c.hop_length : 0;
}
static int64_t logmel_frames_ready(const fv_logmel_config& c, int64_t N) {
    const int64_t pad_l = (c.win_length - c.hop_length) / 2;
    return N + pad_l >= c.n_fft ? 1 + (N + pad_l - c.n_fft) / c.hop_length : 0;
}
static bool logmel_config_ok(const fv_logmel_config* c) {
    return c && c->n_fft >= 1 && c->hop_length >= 1 && c->win_length >= c->hop_length;
}
// a row the whole forward would refuse: no frame, or not longer than the reflect padding (run_model_whole)
static bool logmel_row_too_short(const fv_engine* e, int64_t L) {
    return logmel_frames(e->cfg.mel, L) < 1 || L <= std::max(e->mel.pad_l, e->mel.pad_r);
}
static fv_status logmel_engine_check(const fv_engine* e, const char* fn) {
    if (!e) {
        set_error("%s: null engine", fn);
        return FV_ERR_INVALID;
    }
    if (!e->finalized) {
        set_error("%s: call fv_finalize first", fn);
        return FV_ERR_STATE;
    }
    if (e->cfg.model != FV_MODEL_LOGMEL) {
        set_error("%s: the engine is not a log-mel front-end (FV_MODEL_LOGMEL)", fn);
        return FV_ERR_UNSUPPORTED;
    }
    return FV_OK;
}

// the core's buffers are two (B, H) carries: buf[cur] holds the samples [N - H, N), and a push reads its chunk in place
struct fv_logmel_stream : SampleStream {
    fv_engine* e = nullptr;
    int max_frames = 0;                     // the most frames one call emits
    size_t ws_bytes() const { return align_up(e->logmel_ws_elems(B, max_frames) * sizeof(float), 256); }
};

// frames [E, E2) of every row of a stream, or frames [0, T) of a ragged batch: window kernel, then the forward's tail
static fv_status logmel_run_frames(fv_engine* e, const float* carry, long long carry_stride, long long carry_origin, const float* chunk,
                                   long long chunk_stride, long long chunk_origin, const long long* row_len, long long avail, float* d_out,
                                   int B, long long f0, int T, float* ws, hipStream_t s) {
    const int hop = e->cfg.mel.hop_length, TP = T + e->mel.taps - 1;
    const fv_engine::LogmelParts p = e->logmel_carve(ws, B, T);
    FV_PROF(s, "logmel_window", 0.0, 8.0 * B * (double)hop * TP,
            launch_logmel_window(carry, carry_stride, carry_origin, chunk, chunk_stride, chunk_origin, row_len, avail, p.Yp, B, f0, hop, TP,
                                 e->mel.pad_l, e->mel.pad_r, s));
    return e->run_logmel_tail(p, d_out, B, T, s);
}

static fv_status logmel_stream_step(fv_logmel_stream* st, const float* d_wave, int64_t row_stride, int32_t c, bool flush, float* d_out,
                                    int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = flush ? "fv_logmel_stream_flush" : "fv_logmel_stream_push";
    if (frames_out) *frames_out = 0;
    if (!st || !frames_out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    long long N2;
    bool noop;
    if (const fv_status rs = st->admit(fn, "fv_logmel_stream_reset", d_wave, row_stride, c, flush, &N2, &noop)) return rs;
    if (noop) return FV_OK;
    fv_engine* e = st->e;
    const fv_logmel_config& mc = e->cfg.mel;
    if (flush && st->N > 0 && logmel_row_too_short(e, st->N)) {
        set_error("fv_logmel_stream_flush: the utterance has %lld samples: too short for reflect padding %d/%d and one %d-sample frame",
                  (long long)st->N, e->mel.pad_l, e->mel.pad_r, mc.n_fft);
        return FV_ERR_INVALID;
    }
    const int64_t E2 = std::max<int64_t>(st->E, flush ? logmel_frames(mc, N2) : logmel_frames_ready(mc, N2));
    const int64_t k = E2 - st->E;
    if (k > 0) {
        if (!d_out) {
            set_error("%s: null output (this call emits %lld frames per row)", fn, (long long)k);
            return FV_ERR_INVALID;
        }
        if (k > st->max_frames) {   // (cannot happen: max_frames bounds every call's emission)
            set_error("%s: internal: %lld frames in one call, the stream was sized for %d", fn, (long long)k, st->max_frames);
            return FV_ERR_INVALID;
        }
        if (!d_workspace || workspace_bytes < st->ws_bytes()) {
            set_error("%s: workspace too small (%zu < %zu bytes, fv_logmel_stream_workspace_bytes)", fn, d_workspace ? workspace_bytes : (size_t)0,
                      st->ws_bytes());
            return FV_ERR_INVALID;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const ForwardScope scope(e, nullptr, nullptr);
    const float* prev = st->buf[st->cur];
    if (k > 0) {
        std::vector<long long> row_len;   // rows advance in lockstep: a flush gives every row the same end
        if (flush) row_len.assign((size_t)st->B, (long long)N2);
        if (const fv_status rs = logmel_run_frames(e, prev, st->H, st->N - st->H, flush ? nullptr : d_wave, row_stride, st->N,
                                                   flush ? row_len.data() : nullptr, N2, d_out, st->B, st->E, (int)k, (float*)d_workspace, s))
            return rs;
    }
    if (!flush) {
        FV_PROF(s, "logmel_carry", 0.0, 8.0 * st->B * (double)st->H,
                launch_sample_carry(prev, st->buf[st->cur ^ 1], d_wave, st->stride, row_stride, st->B, st->N, N2 - st->H, st->N - st->H, st->H,
                                    s));
    }
    *frames_out = k;
    st->commit(N2, E2, flush, !flush);
    return FV_OK;
}

extern "C" {

FV_API int64_t fv_logmel_frames(const fv_logmel_config* cfg, int64_t L) {
    if (!logmel_config_ok(cfg) || L < 0 || L > kLogmelMaxLen) return 0;
    return logmel_frames(*cfg, L);
}

FV_API int64_t fv_logmel_frames_ready(const fv_logmel_config* cfg, int64_t N) {
    if (!logmel_config_ok(cfg) || N < 0 || N > kLogmelMaxLen) return 0;
    return logmel_frames_ready(*cfg, N);
}

FV_API fv_status fv_logmel_ragged_forward(fv_engine* e, const float* d_wave, int64_t row_stride, const int32_t* host_lengths, int32_t batch,
                                          int32_t L_max, float* d_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fv_logmel_ragged_forward";
    if (const fv_status st = logmel_engine_check(e, fn)) return st;
    if (!host_lengths || batch < 1 || L_max < 1) {
        set_error("%s: null lengths or empty input (batch=%d, L_max=%d)", fn, batch, L_max);
        return FV_ERR_INVALID;
    }
    if (row_stride < L_max) {
        set_error("%s: row_stride %lld is shorter than L_max = %d", fn, (long long)row_stride, L_max);
        return FV_ERR_INVALID;
    }
    bool any = false;
    for (int b = 0; b < batch; ++b) {
        const int32_t L = host_lengths[b];
        if (L < 0 || L > L_max) {
            set_error("%s: lengths[%d] = %d lies outside [0, L_max = %d]", fn, b, L, L_max);
            return FV_ERR_INVALID;
        }
        if (L > 0 && logmel_row_too_short(e, L)) {
            set_error("%s: lengths[%d] = %d samples is too short for reflect padding %d/%d and one %d-sample frame (0 marks an empty row)", fn, b,
                      L, e->mel.pad_l, e->mel.pad_r, e->cfg.mel.n_fft);
            return FV_ERR_INVALID;
        }
        any = any || L > 0;
    }
    const int64_t T = logmel_frames(e->cfg.mel, L_max);
    if (T < 1) return FV_OK;   // (every row is empty then, and the output has no columns)
    if (T > (1 << 30)) {
        set_error("%s: L_max = %d gives %lld frames, more than 2^30", fn, L_max, (long long)T);
        return FV_ERR_UNSUPPORTED;
    }
    if (!d_wave || !d_out) {
        set_error("%s: null %s", fn, d_wave ? "d_out" : "d_wave");
        return FV_ERR_INVALID;
    }
    const size_t need = fv_workspace_bytes(e, batch, L_max);
    if (!d_workspace || workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_workspace_bytes(e, batch, L_max))", fn, d_workspace ? workspace_bytes : (size_t)0,
                  need);
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const ForwardScope scope(e, nullptr, nullptr);
    std::vector<long long> len((size_t)batch), cols((size_t)batch);
    bool ragged = false;
    for (int b = 0; b < batch; ++b) {
        len[(size_t)b] = host_lengths[b];
        cols[(size_t)b] = logmel_frames(e->cfg.mel, host_lengths[b]);
        ragged = ragged || cols[(size_t)b] < T;
    }
    if (any) {
        if (const fv_status st = logmel_run_frames(e, nullptr, 0, 0, d_wave, row_stride, 0, len.data(), 0, d_out, batch, 0, (int)T,
                                                   (float*)d_workspace, s))
            return st;
    }
    if (!ragged) return FV_OK;
    const int C = fv_output_channels(e);
    FV_PROF(s, "zero_columns", 0.0, 4.0 * batch * C * (double)T, launch_zero_columns(d_out, cols.data(), batch, C, T, s));
    return FV_OK;
}

FV_API fv_status fv_logmel_stream_create(fv_engine* e, int32_t batch, int32_t max_chunk_samples, fv_logmel_stream** out) {
    const char* fn = "fv_logmel_stream_create";
    if (out) *out = nullptr;
    if (const fv_status st = logmel_engine_check(e, fn)) return st;
    if (!out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_logmel_stream> st(new fv_logmel_stream());
    st->e = e;
    // A frame not yet emitted starts less than n_fft samples before N (fv_logmel_frames_ready), and the flush reflects pad_r + 1 < n_fft samples back
    const int H = e->cfg.mel.n_fft;
    if (const fv_status rs = st->create(fn, batch, max_chunk_samples, H, H)) return rs;
    // A push emits the frames that became ready: at most (n_fft + max_chunk) / hop + 1 when the first ones come out; the flush at most pad_r / hop + 1
    st->max_frames = (int)(((int64_t)H + max_chunk_samples) / e->cfg.mel.hop_length + 2);
    *out = st.release();
    return FV_OK;
}

FV_API size_t fv_logmel_stream_workspace_bytes(const fv_logmel_stream* s) { return s ? s->ws_bytes() : 0; }

FV_API int64_t fv_logmel_stream_pending_samples(const fv_logmel_stream* s) {
    if (!s) return 0;
    return s->N - std::max<int64_t>(0, s->E * s->e->cfg.mel.hop_length - s->e->mel.pad_l);
}

FV_API fv_status fv_logmel_stream_push(fv_logmel_stream* s, const float* d_wave, int64_t row_stride, int32_t c, float* d_out,
                                       int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    return logmel_stream_step(s, d_wave, row_stride, c, false, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_logmel_stream_flush(fv_logmel_stream* s, float* d_out, int64_t* frames_out, void* d_workspace, size_t workspace_bytes,
                                        void* stream) {
    return logmel_stream_step(s, nullptr, 0, 0, true, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_logmel_stream_reset(fv_logmel_stream* s) {
    if (!s) {
        set_error("fv_logmel_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->reset();
    return FV_OK;
}

FV_API void fv_logmel_stream_destroy(fv_logmel_stream* s) { delete s; }

}  // extern "C"
