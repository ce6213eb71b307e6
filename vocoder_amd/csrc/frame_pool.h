// The frame counters of the layer streams and pools (fv_wnstream / fv_cnxstream, fv_wnpool / fv_cnxpool), beside sample_pool.h and built on its
// admit, output and counts.  A layered module emits frame t once the R frames after it have arrived, or at the flush: after N' frames a call
// has emitted up to E' = flush ? N' : max(E, N' - R).  FrameStream is that rule for rows in lockstep, FramePool for S slots that advance
// independently.  Both check a call whole before any counter moves and move the counters only after the call was enqueued; the names of the
// reset entry and of the output pointer are arguments, so every entry's messages are its own.  What a module runs between the refusals and
// commit — its tables, its launches, a refusal of its own — stays with the module.  No HIP runtime call is made here.
#pragma once

#include "sample_pool.h"

namespace fv {

constexpr long long kFrameMaxFrames = 1LL << 30;     // frames in one utterance

struct FrameStream {
    int max_chunk = 0, R = 0;
    long long N = 0, E = 0;
    bool flushed = false;

    // What a push of c frames (the flush: c = 0) refuses given its input, after frame_stream_chunk
    fv_status input(const char* fn, const float* d_x, long long x_batch_stride, long long x_row_stride, int c) const {
        if (c > 0 && !d_x) {
            set_error("%s: null d_x with c = %d", fn, c);
            return FV_ERR_INVALID;
        }
        if (c > 0 && (x_row_stride < c || x_batch_stride < 0)) {
            set_error("%s: x_row_stride = %lld (the stride between channels) is shorter than a chunk of c = %d frames, or x_batch_stride = %lld is "
                      "negative", fn, x_row_stride, c, x_batch_stride);
            return FV_ERR_INVALID;
        }
        return FV_OK;
    }
    // The emission rule and the refusals of the output (`out_name`: d_z / d_y): the call takes the stream to N1 frames received and E1 emitted
    fv_status output(const char* fn, const char* out_name, int c, bool flush, bool have_out, long long y_row_stride, long long* N1,
                     long long* E1) const {
        *N1 = N + c, *E1 = flush ? *N1 : std::max(E, *N1 - R);
        const long long k = *E1 - E;
        if (k > 0 && !have_out) {
            set_error("%s: null %s for the %lld frames this call emits", fn, out_name, k);
            return FV_ERR_INVALID;
        }
        if (k > 0 && y_row_stride < k) {
            set_error("%s: y_row_stride = %lld is shorter than the %lld frames this call emits", fn, y_row_stride, k);
            return FV_ERR_INVALID;
        }
        return FV_OK;
    }
    // the call was enqueued
    void commit(long long N1, long long E1, bool flush, int64_t* emitted) {
        if (emitted) *emitted = E1 - E;
        N = N1, E = E1, flushed = flush;
    }
    // the next utterance; what the module keeps on the device stays: nothing at or past a frontier, or before frame 0, is ever read
    void reset() { N = E = 0, flushed = false; }
    long long pending() const { return N - E; }
};

// The first refusals of a push or flush, on a stream that may be NULL: no stream, a flushed one (`reset_fn` starts the next utterance), c
// outside [0, max_chunk], more than 2^30 frames
inline fv_status frame_stream_chunk(const char* fn, const char* reset_fn, const FrameStream* s, int c) {
    if (!s) {
        set_error("%s: null stream", fn);
        return FV_ERR_INVALID;
    }
    if (s->flushed) {
        set_error("%s: the stream was flushed at %lld frames: %s starts the next utterance", fn, s->N, reset_fn);
        return FV_ERR_STATE;
    }
    if (c < 0 || c > s->max_chunk) {
        set_error("%s: c = %d must lie in [0, max_chunk = %d]", fn, c, s->max_chunk);
        return FV_ERR_INVALID;
    }
    if (s->N + c > kFrameMaxFrames) {
        set_error("%s: %lld + %d frames are more than the 2^30 a stream counts", fn, s->N, c);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

inline fv_status frame_stream_reset(const char* fn, FrameStream* s) {
    if (!s) {
        set_error("%s: null stream", fn);
        return FV_ERR_INVALID;
    }
    s->reset();
    return FV_OK;
}

struct FramePool {
    int S = 0, max_chunk = 0, R = 0;
    std::vector<int64_t> N, E;
    std::vector<int32_t> flushed;
    int launches = 0;                   // of the last accepted step

    static fv_status range(const char* fn, int sessions, int max_chunk) {
        if (sessions < 1 || sessions > 65535 || max_chunk < 1 || max_chunk > (1 << 20)) {
            set_error("%s: sessions (%d) must lie in [1, 65535] and max_chunk (%d) in [1, 2^20]", fn, sessions, max_chunk);
            return FV_ERR_INVALID;
        }
        return FV_OK;
    }
    void init(int sessions, int chunk, int reach) {
        S = sessions, max_chunk = chunk, R = reach;
        N.assign((size_t)S, 0), E.assign((size_t)S, 0), flushed.assign((size_t)S, 0);
    }

    // The refusals of a step's items (sample_pool_admit, counting frames, 2^30 of them) and the emission rule: N2 and E2 per item
    static fv_status admit(const char* fn, const char* reset_fn, int R, int S, int max_chunk, const int64_t* received, const int64_t* emitted,
                           const int32_t* flushed, const SamplePoolItem* items, int count, bool buffers, const float* d_x,
                           long long x_row_stride, long long* N2, long long* E2) {
        if (const fv_status st = sample_pool_admit(fn, reset_fn, S, max_chunk, received, flushed, items, count, buffers, d_x, x_row_stride, N2,
                                                   "frames", kFrameMaxFrames, "2^30"))
            return st;
        for (int i = 0; i < count; ++i) E2[i] = items[i].flush ? N2[i] : std::max((long long)emitted[items[i].session], N2[i] - R);
        return FV_OK;
    }
    fv_status admit(const char* fn, const char* reset_fn, const SamplePoolItem* items, int count, const float* d_x, long long x_row_stride,
                    long long* N2, long long* E2) const {
        return admit(fn, reset_fn, R, S, max_chunk, N.data(), E.data(), flushed.data(), items, count, true, d_x, x_row_stride, N2, E2);
    }
    // A *_plan entry on the caller's counters: a negative fv_status, or the largest count
    static int64_t plan(const char* fn, const char* reset_fn, int reach, int sessions, int max_chunk, const int64_t* received,
                        const int64_t* emitted, const int32_t* flushed, const SamplePoolItem* items, int count, int64_t* frames_out) {
        if (reach < 0) {
            set_error("%s: reach = %d must be >= 0", fn, reach);
            return FV_ERR_INVALID;
        }
        if (const fv_status st = range(fn, sessions, max_chunk)) return st;
        if (!received || !emitted || (count > 0 && !frames_out)) {
            set_error("%s: null argument", fn);
            return FV_ERR_INVALID;
        }
        std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
        if (const fv_status st = admit(fn, reset_fn, reach, sessions, max_chunk, received, emitted, flushed, items, count, false, nullptr, 0,
                                       N2.data(), E2.data()))
            return st;
        return sample_pool_counts(emitted, items, count, E2.data(), frames_out);
    }
    // What a step refuses once its items are admitted (`out_name`: d_z / d_y, contiguous rows of out_cols columns)
    fv_status output(const char* fn, const char* out_name, const SamplePoolItem* items, int count, const float* d_x, long long x_item_stride,
                     const long long* E2, bool have_out, int out_cols) const {
        if (d_x && x_item_stride < 0) {
            set_error("%s: x_item_stride = %lld is negative", fn, x_item_stride);
            return FV_ERR_INVALID;
        }
        if (out_cols > kFrameMaxFrames) {
            set_error("%s: out_cols = %d is more than 2^30", fn, out_cols);
            return FV_ERR_INVALID;
        }
        if (const fv_status st = sample_pool_output(fn, "frames", items, count, E.data(), E2, 1, have_out, out_cols, out_cols)) return st;
        if (count > 0 && out_cols > 0 && !have_out) {
            set_error("%s: null %s although every row's first out_cols = %d columns are written", fn, out_name, out_cols);
            return FV_ERR_INVALID;
        }
        return FV_OK;
    }
    // the step was enqueued, in `step_launches` launches: the items' counters move
    void commit(const SamplePoolItem* items, int count, const long long* N2, const long long* E2, int64_t* frames_out, int step_launches) {
        for (int i = 0; i < count; ++i) {
            const size_t s = (size_t)items[i].session;
            if (frames_out) frames_out[i] = E2[i] - E[s];
            N[s] = N2[i], E[s] = E2[i];
            if (items[i].flush) flushed[s] = 1;
        }
        launches = step_launches;
    }
    // the next utterance of one slot; its ring rows keep their frames: nothing at or past a frontier, or before frame 0, is ever read
    fv_status reset(const char* fn, int s) {
        if (s < 0 || s >= S) {
            set_error("%s: session %d lies outside [0, %d)", fn, s, S);
            return FV_ERR_INVALID;
        }
        N[(size_t)s] = E[(size_t)s] = 0, flushed[(size_t)s] = 0;
        return FV_OK;
    }
    bool valid(int s) const { return s >= 0 && s < S; }
    int64_t received(int s) const { return valid(s) ? N[(size_t)s] : -1; }
    int64_t emitted(int s) const { return valid(s) ? E[(size_t)s] : -1; }
    int64_t pending(int s) const { return valid(s) ? N[(size_t)s] - E[(size_t)s] : -1; }
    int64_t max_frames() const { return (int64_t)max_chunk + R; }
};

inline fv_status frame_pool_reset(const char* fn, FramePool* p, int s) {
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    return p->reset(fn, s);
}

}  // namespace fv
