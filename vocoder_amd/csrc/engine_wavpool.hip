// The log-mel front-end as a pool of sessions that advance independently (fv_wavpool_*, include/fishvoc.h): what
// fish_vocoder/data/transforms/spectrogram.py:25-104 computes for one whole file (test.py:64-71), per session and chunk by chunk.  The
// counters and the carry are the sample pool's (sample_pool.h); a step is logmel_pool_window_kernel (frame_kernels.hip) over one table entry
// per emitting item, the forward's own tail (fv_engine::run_logmel_tail) on (rows, max k), a crop into the caller's rows and the carry copy
// of the items that pushed samples.  These entries enqueue eagerly and leave the engine's captured graphs and their bookkeeping alone.
#include <memory>

#include "engine_internal.h"
#include "sample_pool.h"

static int64_t wavpool_pad_l(const fv_logmel_config& c) { return (c.win_length - c.hop_length) / 2; }
static int64_t wavpool_pad_r(const fv_logmel_config& c) { return (c.win_length - c.hop_length + 1) / 2; }
// a row the whole forward would refuse: no frame, or not longer than the reflect padding (run_model_whole)
static bool wavpool_too_short(const fv_logmel_config& c, int64_t L) {
    return fv_logmel_frames(&c, L) < 1 || L <= std::max(wavpool_pad_l(c), wavpool_pad_r(c));
}

// The emission rule of one step, after the pool's admit: E2[i] = max(E, flush ? frames(N2) : frames_ready(N2)).  A flush of a non-empty
// utterance that is too short refuses the step and names the session.
static fv_status wavpool_emission(const char* fn, const fv_logmel_config& c, const int64_t* emitted, const fv_wavpool_item* items, int count,
                                  const long long* N2, long long* E2) {
    for (int i = 0; i < count; ++i) {
        const fv_wavpool_item& it = items[i];
        if (it.flush && N2[i] > 0 && wavpool_too_short(c, N2[i])) {
            set_error("%s: session %d (item %d) ends after %lld samples: too short for reflect padding %d/%d and one %d-sample frame", fn,
                      it.session, i, N2[i], (int)wavpool_pad_l(c), (int)wavpool_pad_r(c), c.n_fft);
            return FV_ERR_INVALID;
        }
        const int64_t E = emitted[it.session];
        E2[i] = std::max<int64_t>(E, it.flush ? fv_logmel_frames(&c, N2[i]) : fv_logmel_frames_ready(&c, N2[i]));
    }
    return FV_OK;
}

// the core's buffers are two (S, H) carries: buf[cur[s]] row s holds the samples [N_s - H, N_s) of slot s, and a step reads its chunks in place
struct fv_wavpool : SamplePool {
    fv_engine* e = nullptr;
    int max_frames = 0;                     // the most frames one item emits in one step
    int C = 0;                              // output channels
    size_t front_bytes() const { return align_up(e->logmel_ws_elems(S, max_frames) * sizeof(float), 256); }
    size_t ws_bytes() const { return front_bytes() + align_up((size_t)S * C * max_frames * sizeof(float), 256); }
};

extern "C" {

FV_API fv_status fv_wavpool_create(fv_engine* e, int32_t sessions, int32_t max_chunk_samples, fv_wavpool** out) {
    const char* fn = "fv_wavpool_create";
    if (out) *out = nullptr;
    if (!e || !out) {
        set_error("%s: null argument", fn);
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
    std::unique_ptr<fv_wavpool> p(new fv_wavpool());
    p->e = e;
    p->C = fv_output_channels(e);
    // the carry: a frame not yet emitted starts less than n_fft samples before N, and a flush reflects pad_r + 1 < n_fft samples back (fv_logmel_stream_create)
    const int H = e->cfg.mel.n_fft;
    if (const fv_status rs = p->create(fn, sessions, max_chunk_samples, H)) return rs;
    // An item emits at most (n_fft + max_chunk) / hop + 2 frames: with E >= frames_ready(N) and pad_r < n_fft, frames(N + c) - E stays below
    // (c + pad_r) / hop + 2, the first emission and the flush in one step included
    p->max_frames = (int)(((int64_t)H + max_chunk_samples) / e->cfg.mel.hop_length + 2);
    *out = p.release();
    return FV_OK;
}

FV_API size_t fv_wavpool_workspace_bytes(const fv_wavpool* p) { return p ? p->ws_bytes() : 0; }

FV_API int32_t fv_wavpool_max_frames(const fv_wavpool* p) { return p ? p->max_frames : 0; }

FV_API int64_t fv_wavpool_received_samples(const fv_wavpool* p, int32_t s) { return sample_pool_received(p, s); }

FV_API int64_t fv_wavpool_emitted_frames(const fv_wavpool* p, int32_t s) { return sample_pool_emitted(p, s); }

FV_API int64_t fv_wavpool_pending_samples(const fv_wavpool* p, int32_t s) {
    if (!p || s < 0 || s >= p->S) return 0;
    return p->N[(size_t)s] - std::max<int64_t>(0, p->E[(size_t)s] * p->e->cfg.mel.hop_length - p->e->mel.pad_l);
}

FV_API int32_t fv_wavpool_plan(const fv_logmel_config* cfg, int32_t sessions, int32_t max_chunk_samples, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* frames_out) {
    const char* fn = "fv_wavpool_plan";
    if (!cfg || cfg->n_fft < 1 || cfg->hop_length < 1 || cfg->win_length < cfg->hop_length) {
        set_error("%s: unusable config (need n_fft >= 1, 1 <= hop_length <= win_length)", fn);
        return FV_ERR_INVALID;
    }
    if (const fv_status st = sample_pool_range(fn, sessions, max_chunk_samples)) return st;
    const int64_t k_max = sample_pool_plan(fn, sessions, max_chunk_samples, received, emitted, flushed, items, count, frames_out,
                                           [&](const long long* N2, long long* E2) {
                                               return wavpool_emission(fn, *cfg, emitted, items, count, N2, E2);
                                           });
    return (int32_t)std::min<int64_t>(k_max, INT32_MAX);   // (a refusal is negative and passes as it is)
}

FV_API fv_status fv_wavpool_step(fv_wavpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream) {
    const char* fn = "fv_wavpool_step";
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    for (int i = 0; frames_out && i < count; ++i) frames_out[i] = 0;
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status rs = p->admit(fn, "fv_wavpool_reset", items, count, d_chunks, chunk_stride, N2.data())) return rs;
    fv_engine* e = p->e;
    const fv_logmel_config& mc = e->cfg.mel;
    if (const fv_status rs = wavpool_emission(fn, mc, p->E.data(), items, count, N2.data(), E2.data())) return rs;
    // one table entry per item: `win` the rows that emit, in item order; `carry` the items that push samples
    std::vector<SamplePoolEntry> all, win, carry;
    p->build_entries(items, count, N2.data(), E2.data(), all, carry);
    std::vector<PoolCropEntry> crop((size_t)count);
    long long k_max = 0;
    for (int i = 0; i < count; ++i) {
        const long long k = E2[(size_t)i] - p->E[(size_t)items[i].session];
        if (k > p->max_frames) {   // (cannot happen: max_frames bounds every item's emission)
            set_error("%s: internal: session %d emits %lld frames in one step, the pool was sized for %d", fn, items[i].session, k, p->max_frames);
            return FV_ERR_INVALID;
        }
        crop[(size_t)i] = PoolCropEntry{i, k > 0 ? (int)win.size() : -1, 0, k};
        if (k > 0) win.push_back(all[(size_t)i]);
        k_max = std::max(k_max, k);
    }
    if (out_frames < k_max || out_frames < 0) {
        set_error("%s: out_frames = %d, but an item of this step emits %lld frames", fn, out_frames, k_max);
        return FV_ERR_INVALID;
    }
    if (out_frames > 0 && count > 0 && !d_out) {
        set_error("%s: null output (out_frames = %d)", fn, out_frames);
        return FV_ERR_INVALID;
    }
    if (k_max > 0 && (!d_workspace || workspace_bytes < p->ws_bytes())) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_wavpool_workspace_bytes)", fn, d_workspace ? workspace_bytes : (size_t)0,
                  p->ws_bytes());
        return FV_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const ForwardScope scope(e, nullptr, nullptr);
    const int rows = (int)win.size(), T = (int)k_max, hop = mc.hop_length;
    float* y = (float*)((char*)d_workspace + p->front_bytes());   // (rows, C, T): the tail's result before the crop
    if (rows > 0) {
        const int TP = T + e->mel.taps - 1;
        const fv_engine::LogmelParts parts = e->logmel_carve((float*)d_workspace, rows, T);
        FV_PROF(s, "logmel_pool_window", 0.0, 8.0 * rows * (double)hop * TP,
                launch_logmel_pool_window(p->buf[0], p->buf[1], p->H, d_chunks, chunk_stride, win.data(), rows, parts.Yp, hop, TP, e->mel.taps,
                                          e->mel.pad_l, e->mel.pad_r, s));
        if (const fv_status rs = e->run_logmel_tail(parts, y, rows, T, s)) return rs;
    }
    if (count > 0 && out_frames > 0) {   // every element of d_out: the item's frames, then zeros; a row of zeros for an item that emits nothing
        FV_PROF(s, "wavpool_crop", 0.0, 8.0 * count * p->C * (double)out_frames,
                launch_pool_crop(y, d_out, crop.data(), count, p->C, T, out_frames, 1, s));
    }
    FV_PROF(s, "sample_pool_carry", 0.0, 8.0 * carry.size() * (double)p->H,
            launch_sample_pool_carry(p->buf[0], p->buf[1], p->H, d_chunks, chunk_stride, carry.data(), (int)carry.size(), s));
    for (int i = 0; frames_out && i < count; ++i) frames_out[i] = E2[(size_t)i] - p->E[(size_t)items[i].session];
    p->commit(items, count, N2.data(), E2.data());
    return FV_OK;
}

FV_API fv_status fv_wavpool_reset(fv_wavpool* p, int32_t session) { return sample_pool_reset(p, "fv_wavpool_reset", session); }

FV_API void fv_wavpool_destroy(fv_wavpool* p) { delete p; }

}  // extern "C"
