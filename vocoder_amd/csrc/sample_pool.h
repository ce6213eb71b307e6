// The core of the per-session sample-domain front-ends (fv_wavpool in engine_wavpool.hip): `S` slots that advance independently.  Every slot has
// its own N samples received, E outputs emitted, flushed flag and its own ping-pong bit cur[s]: the last H samples of slot s are carried in
// buf[cur[s]] row s, and a step that pushes samples into the slot writes buf[cur[s] ^ 1] row s (launch_sample_pool_carry, window_kernels.hip)
// and then flips that slot's bit alone.  A step touches only some slots; one toggle for all of them (sample_stream.h) would leave the
// untouched slots' carry in the buffer the next step no longer reads.  Per slot the streams' rule holds: no launch reads and writes the same
// buffer.  A step is checked whole before any counter moves (admit), and only its items' counters move (commit).  What a pool emits, and what
// it runs between admit() and commit(), is its own.  What the pools state the same way is here too: the range check, the refusals of a step's
// output buffer, the tail of a *_plan and the table entry of an item.  Only create() and the destructor make a HIP runtime call: a host
// program can drive everything else.
#pragma once

#include "sample_stream.h"

namespace fv {

using SamplePoolItem = fv_wavpool_item;   // session, samples, flush: the utterance ends with these samples

// The refusals every step shares, over the counters `received` / `flushed` of `S` slots (flushed may be NULL: none is), in this order per item:
// session out of range, duplicate session, samples outside [0, max_chunk], a flushed slot (FV_ERR_STATE), more than 2^40 samples; then, with
// `buffers`, a NULL chunk buffer although an item has samples and a row stride shorter than the longest chunk.  Each names the item and the
// session.  FV_OK: N2[i] = the samples slot items[i].session has received once the step commits.  Changes nothing.  A pool that counts
// something else (the posterior pool: frames, 2^30 of them) names its unit and its longest utterance.
inline fv_status sample_pool_admit(const char* fn, const char* reset_fn, int S, int max_chunk, const int64_t* received, const int32_t* flushed,
                                   const SamplePoolItem* items, int count, bool buffers, const float* chunks, long long chunk_stride,
                                   long long* N2, const char* unit = "samples", long long max_len = kSampleStreamMaxLen,
                                   const char* max_name = "2^40") {
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
            set_error("%s: item %d (session %d) has %d %s, outside [0, max_chunk = %d]", fn, i, it.session, it.samples, unit, max_chunk);
            return FV_ERR_INVALID;
        }
        if (flushed && flushed[it.session]) {
            set_error("%s: session %d was flushed (item %d); %s it before the next utterance", fn, it.session, i, reset_fn);
            return FV_ERR_STATE;
        }
        const long long N = received[it.session];
        if (N < 0 || N + it.samples > max_len) {
            set_error("%s: item %d takes session %d past %s %s in one utterance (%lld + %d)", fn, i, it.session, max_name, unit, N, it.samples);
            return FV_ERR_INVALID;
        }
        N2[i] = N + it.samples;
        if (it.samples > longest) longest = it.samples, longest_item = i;
    }
    if (buffers && longest > 0) {
        if (!chunks) {
            set_error("%s: null chunk buffer although item %d (session %d) has %d %s", fn, longest_item, items[longest_item].session,
                      longest, unit);
            return FV_ERR_INVALID;
        }
        if (chunk_stride < longest) {
            set_error("%s: row stride %lld is shorter than the longest chunk, the %d %s of item %d (session %d)", fn, chunk_stride, longest,
                      unit, longest_item, items[longest_item].session);
            return FV_ERR_INVALID;
        }
    }
    return FV_OK;
}

// The range check of every *_create and *_plan
inline fv_status sample_pool_range(const char* fn, int sessions, int max_chunk) {
    if (sessions < 1 || sessions > 65535 || max_chunk < 1 || max_chunk > (1 << 28)) {
        set_error("%s: sessions (%d) must lie in [1, 65535] and max_chunk (%d) in [1, 2^28]", fn, sessions, max_chunk);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// The refusals of a step's output buffer: (E2 - E) * per_unit columns for the item that emits most, `what` names a column
inline fv_status sample_pool_output(const char* fn, const char* what, const SamplePoolItem* items, int count, const int64_t* emitted,
                                    const long long* E2, long long per_unit, bool have_out, long long out_stride, int out_cols) {
    long long k_max = 0;
    int k_item = 0;
    for (int i = 0; i < count; ++i) {
        const long long k = (E2[i] - emitted[items[i].session]) * per_unit;
        if (k > k_max) k_max = k, k_item = i;
    }
    const int k_session = count > 0 ? items[k_item].session : -1;
    if (out_cols < k_max || out_cols < 0) {
        set_error("%s: out_cols = %d, but item %d (session %d) emits %lld %s in this step", fn, out_cols, k_item, k_session, k_max, what);
        return FV_ERR_INVALID;
    }
    if (out_stride < out_cols) {
        set_error("%s: out_stride = %lld is shorter than out_cols = %d (item %d, session %d, emits %lld %s)", fn, out_stride, out_cols, k_item,
                  k_session, k_max, what);
        return FV_ERR_INVALID;
    }
    if (k_max > 0 && !have_out) {
        set_error("%s: null output although item %d (session %d) emits %lld %s", fn, k_item, k_session, k_max, what);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// What a plan returns: E' - E per item and the largest of them
inline int64_t sample_pool_counts(const int64_t* emitted, const SamplePoolItem* items, int count, const long long* E2, int64_t* out) {
    int64_t k_max = 0;
    for (int i = 0; i < count; ++i) {
        out[i] = E2[i] - emitted[items[i].session];
        k_max = std::max(k_max, out[i]);
    }
    return k_max;
}

// The tail of a *_plan, after the pool's own checks of its config and sample_pool_range: the null arguments, the admit without buffers, the
// pool's rule `emission(N2, E2) -> fv_status`, which fills E2 and may refuse, and the counts.  A negative fv_status, or the largest count.
template <class Emission>
inline int64_t sample_pool_plan(const char* fn, int sessions, int max_chunk, const int64_t* received, const int64_t* emitted,
                                const int32_t* flushed, const SamplePoolItem* items, int count, int64_t* out, Emission&& emission) {
    if (!received || !emitted || (count > 0 && !out)) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    std::vector<long long> N2((size_t)std::max(count, 0)), E2(N2.size());
    if (const fv_status rs = sample_pool_admit(fn, "reset", sessions, max_chunk, received, flushed, items, count, false, nullptr, 0, N2.data()))
        return rs;
    if (const fv_status rs = emission(N2.data(), E2.data())) return rs;
    return sample_pool_counts(emitted, items, count, E2.data(), out);
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
        if (const fv_status rs = sample_pool_range(fn, sessions, chunk)) return rs;
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

    // The table entry of item i once admit gave N2 and the pool's rule E2: the slot's bit, the E2 - E it emits (its caller bounds that to an
    // int), the carried samples [N - H, N), the chunk up to N2 and, with a flush, the utterance's end there
    SamplePoolEntry entry(int i, const SamplePoolItem& item, long long N2, long long E2) const {
        const size_t s = (size_t)item.session;
        return SamplePoolEntry{i, item.session, (int)cur[s], (int)(E2 - E[s]), N[s] - H, N[s], item.flush ? N2 : -1, N2, E[s]};
    }
    // one entry per item in `rows`, in item order, and in `carry` those of the items that push samples (launch_sample_pool_carry)
    void build_entries(const SamplePoolItem* items, int count, const long long* N2, const long long* E2, std::vector<SamplePoolEntry>& rows,
                       std::vector<SamplePoolEntry>& carry) const {
        rows.resize((size_t)std::max(count, 0)), carry.clear();
        for (int i = 0; i < count; ++i) {
            rows[(size_t)i] = entry(i, items[i], N2[i], E2[i]);
            if (items[i].samples > 0) carry.push_back(rows[(size_t)i]);
        }
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

    int64_t received(int s) const { return s >= 0 && s < S ? N[(size_t)s] : 0; }
    int64_t emitted(int s) const { return s >= 0 && s < S ? E[(size_t)s] : 0; }

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

// fv_*pool_received / _emitted / _reset on a pool that may be NULL
inline int64_t sample_pool_received(const SamplePool* p, int s) { return p ? p->received(s) : 0; }
inline int64_t sample_pool_emitted(const SamplePool* p, int s) { return p ? p->emitted(s) : 0; }
inline fv_status sample_pool_reset(SamplePool* p, const char* fn, int s) {
    if (!p) {
        set_error("%s: null pool", fn);
        return FV_ERR_INVALID;
    }
    return p->reset(fn, s);
}

}  // namespace fv
