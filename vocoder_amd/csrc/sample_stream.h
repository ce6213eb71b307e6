// The core of the sample-domain streams (fv_resample_stream in resample.hip, fv_logmel_stream in engine_logmel.hip): `B` rows advance in
// lockstep, N samples received and E outputs emitted per row, and the last H samples of every row carried from call to call in two ping-pong
// buffers of one allocation — buf[cur] holds the carried samples, a call writes buf[cur ^ 1] (launch_sample_carry, window_kernels.hip) and then
// toggles, so no launch reads and writes the same buffer (include/fishvoc.h).  What a stream emits, and what it runs between admit() and
// commit(), is its own.  admit / commit / reset make no HIP runtime call (as conv_pack.hip makes none): a host program can drive them.
#pragma once

#include "fv_internal.h"

namespace fv {

constexpr long long kSampleStreamMaxLen = 1LL << 40;   // n N and N hop stay far inside 64 bits

struct SampleStream {
    int B = 0, max_chunk = 0, H = 0, cur = 0;
    long long stride = 0;                   // row stride of buf[]
    float* buf[2] = {nullptr, nullptr};     // one allocation
    long long N = 0, E = 0;
    bool flushed = false;
    ~SampleStream() {
        if (buf[0]) (void)hipFree(buf[0]);
    }

    // the range checks of `fn` (a *_create), then two zeroed (batch, row_stride) buffers
    fv_status create(const char* fn, int batch, int chunk, int h, long long row_stride) {
        if (batch < 1 || batch > 65535 || chunk < 1 || chunk > (1 << 28)) {
            set_error("%s: batch (%d) must lie in [1, 65535] and max_chunk (%d) in [1, 2^28]", fn, batch, chunk);
            return FV_ERR_INVALID;
        }
        B = batch, max_chunk = chunk, H = h, stride = row_stride;
        const size_t elems = (size_t)batch * (size_t)row_stride;
        FV_HIP_CHECK(hipMalloc((void**)&buf[0], 2 * elems * sizeof(float)));
        buf[1] = buf[0] + elems;
        FV_HIP_CHECK(hipMemset(buf[0], 0, 2 * elems * sizeof(float)));
        return FV_OK;
    }

    // The refusals every push (`c` samples per row at `chunk`, rows `chunk_stride` apart) and every flush share, in the order the entries have
    // always made them.  FV_OK: *N2 = the samples received once the call commits; *noop: an empty push, which returns FV_OK at once.
    fv_status admit(const char* fn, const char* reset_fn, const float* chunk, long long chunk_stride, int c, bool flush, long long* N2,
                    bool* noop) const {
        *N2 = N, *noop = false;
        if (flushed) {
            set_error("%s: the stream was flushed; %s it before the next utterance", fn, reset_fn);
            return FV_ERR_STATE;
        }
        if (flush) return FV_OK;
        if (c < 0 || c > max_chunk) {
            set_error("%s: %d samples, outside [0, max_chunk = %d] of this stream", fn, c, max_chunk);
            return FV_ERR_INVALID;
        }
        if (c == 0) {
            *noop = true;
            return FV_OK;
        }
        if (!chunk || chunk_stride < c) {
            set_error("%s: %s", fn, chunk ? "the row stride is shorter than the chunk" : "null chunk");
            return FV_ERR_INVALID;
        }
        if (N + c > kSampleStreamMaxLen) {
            set_error("%s: more than 2^40 samples in one utterance", fn);
            return FV_ERR_INVALID;
        }
        *N2 = N + c;
        return FV_OK;
    }

    // the call was enqueued; toggled: it wrote buf[cur ^ 1], which now holds the carried samples
    void commit(long long N2, long long E2, bool flush, bool toggled) {
        N = N2, E = E2;
        if (flush) flushed = true;
        if (toggled) cur ^= 1;
    }

    // the next utterance: samples before 0 are zeros by index, whatever the carried buffer holds
    void reset() {
        N = E = 0;
        flushed = false;
    }
};

}  // namespace fv
