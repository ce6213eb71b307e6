// The core of the per-session sample-domain front-ends (fv_wavpool in engine_wavpool.hip): `S` slots that advance independently.  Every slot has
// its own N samples received, E outputs emitted, flushed flag and its own ping-pong bit cur[s]: the last H samples of slot s are carried in
// buf[cur[s]] row s, and a step that pushes samples into the slot writes buf[cur[s] ^ 1] row s (launch_sample_pool_carry, window_kernels.hip)
// and then flips that slot's bit alone.  A step touches only some slots; one toggle for all of them (sample_stream.h) would leave the
// untouched slots' carry in the buffer the next step no longer reads.  Per slot the streams' rule holds: no launch reads and writes the same
// buffer.  A step is checked whole before any counter moves (admit), and only its items' counters move (commit).  What a pool emits, and what
// it runs between admit() and commit(), is its own.  admit / commit / reset make no HIP runtime call: a host program can drive them.
#pragma once

#include "sample_stream.h"

namespace fv {

using SamplePoolItem = fv_wavpool_item;   // session, samples, flush: the utterance ends with these samples

// The refusals every step shares, over the counters `received` / `flushed` of `S` slots (flushed may be NULL: none is), in this order per item:
// session out of range, duplicate session, samples outside [0, max_chunk], a flushed slot (FV_ERR_STATE), more than 2^40 samples; then, with
// `buffers`, a NULL chunk buffer although an item has samples and a row stride shorter than the longest chunk.  Each names the item and the
// session.  FV_OK: N2[i] = the samples slot items[i].session has received once the step commits.  Changes nothing.
inline fv_status sample_pool_admit(const char* fn, const char* reset_fn, int S, int max_chunk, const int64_t* received, const int32_t* flushed,
                                   const SamplePoolItem* items, int count, bool buffers, const float* chunks, long long chunk_stride,
                                   long long* N2) {
    if (count < 0 || (count > 0 && (!items || !N2))) {
        set_error("%s: %d items with a null %s", fn, count, items ? "result" : "item list");
        return FV_ERR_INVALID;
    }
    std::vector<unsigned char> seen((size_t)S, 0);
    int longest = 0, longest_item = 0;
    for (int i = 0; i < count; ++i) {
        const SamplePoolItem& it = items[i];
        if (it.session < 0 || it.session >= S) {
            set_error("%s: item %d names session %d, outside [0, %d)", fn, i, it.session, S);
            return FV_ERR_INVALID;
        }
        if (seen[(size_t)it.session]) {
            set_error("%s: duplicate session %d (item %d): a session appears at most once per step", fn, it.session, i);
            return FV_ERR_INVALID;
        }
        seen[(size_t)it.session] = 1;
        if (it.samples < 0 || it.samples > max_chunk) {
            set_error("%s: item %d (session %d) has %d samples, outside [0, max_chunk = %d]", fn, i, it.session, it.samples, max_chunk);
            return FV_ERR_INVALID;
        }
        if (flushed && flushed[it.session]) {
            set_error("%s: session %d was flushed (item %d); %s it before the next utterance", fn, it.session, i, reset_fn);
            return FV_ERR_STATE;
        }
        const long long N = received[it.session];
        if (N < 0 || N + it.samples > kSampleStreamMaxLen) {
            set_error("%s: item %d takes session %d past 2^40 samples in one utterance (%lld + %d)", fn, i, it.session, N, it.samples);
            return FV_ERR_INVALID;
        }
        N2[i] = N + it.samples;
        if (it.samples > longest) longest = it.samples, longest_item = i;
    }
    if (buffers && longest > 0) {
        if (!chunks) {
            set_error("%s: null chunk buffer although item %d (session %d) has %d samples", fn, longest_item, items[longest_item].session,
                      longest);
            return FV_ERR_INVALID;
        }
        if (chunk_stride < longest) {
            set_error("%s: row stride %lld is shorter than the longest chunk, the %d samples of item %d (session %d)", fn, chunk_stride, longest,
                      longest_item, items[longest_item].session);
            return FV_ERR_INVALID;
        }
    }
    return FV_OK;
}

struct SamplePool {
    int S = 0, max_chunk = 0, H = 0;
    float* buf[2] = {nullptr, nullptr};     // two (S, H) buffers of one allocation
    std::vector<int64_t> N, E;
    std::vector<int32_t> flushed;
    std::vector<unsigned char> cur;         // the slot's carried samples are in buf[cur[s]] row s
    ~SamplePool() {
        if (buf[0]) (void)hipFree(buf[0]);
    }

    // the range checks of `fn` (a *_create), then two zeroed (sessions, h) buffers
    fv_status create(const char* fn, int sessions, int chunk, int h) {
        if (sessions < 1 || sessions > 65535 || chunk < 1 || chunk > (1 << 28)) {
            set_error("%s: sessions (%d) must lie in [1, 65535] and max_chunk (%d) in [1, 2^28]", fn, sessions, chunk);
            return FV_ERR_INVALID;
        }
        init(sessions, chunk, h);
        const size_t elems = (size_t)sessions * (size_t)h;
        FV_HIP_CHECK(hipMalloc((void**)&buf[0], 2 * elems * sizeof(float)));
        buf[1] = buf[0] + elems;
        FV_HIP_CHECK(hipMemset(buf[0], 0, 2 * elems * sizeof(float)));
        return FV_OK;
    }
    // the host half of create: the counters of `sessions` fresh slots
    void init(int sessions, int chunk, int h) {
        S = sessions, max_chunk = chunk, H = h;
        N.assign((size_t)S, 0), E.assign((size_t)S, 0), flushed.assign((size_t)S, 0), cur.assign((size_t)S, 0);
    }

    fv_status admit(const char* fn, const char* reset_fn, const SamplePoolItem* items, int count, const float* chunks, long long chunk_stride,
                    long long* N2) const {
        return sample_pool_admit(fn, reset_fn, S, max_chunk, N.data(), flushed.data(), items, count, true, chunks, chunk_stride, N2);
    }

    // the step was enqueued: the items' counters move, and the bit of every slot that pushed samples flips (the step wrote its other buffer)
    void commit(const SamplePoolItem* items, int count, const long long* N2, const long long* E2) {
        for (int i = 0; i < count; ++i) {
            const size_t s = (size_t)items[i].session;
            N[s] = N2[i], E[s] = E2[i];
            if (items[i].flush) flushed[s] = 1;
            if (items[i].samples > 0) cur[s] ^= 1;
        }
    }

    // the next utterance of one slot: samples before 0 are zeros by index, whatever the carried buffer holds
    fv_status reset(const char* fn, int s) {
        if (s < 0 || s >= S) {
            set_error("%s: session %d lies outside [0, %d)", fn, s, S);
            return FV_ERR_INVALID;
        }
        N[(size_t)s] = E[(size_t)s] = 0;
        flushed[(size_t)s] = 0;
        return FV_OK;
    }
};

}  // namespace fv
