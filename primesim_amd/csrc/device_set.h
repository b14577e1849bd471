// device_set.h — what the device-side ensemble stages (stream_gen.hip, trace_place.hip,
// delay_sum.hip, delay_hist.hip, delay_tail.hip, delay_series.hip, run_results.hip) share on the host: one allocation of device state per set, the
// set's own stream, and the rule that orders the set's calls whatever stream
// each is given.  A stage's handle derives from DeviceSet and adds what is its
// own.  Host code only: the stage files include it, engine.hip does not.
//
// The ordering rule.  The state is the set's, so its calls run one after the
// other: every call records `ev` on its stream when it has launched and becomes
// `last`; a call on another stream than `last` first makes its stream wait for
// `ev`.  Calls that stay on one stream are ordered by the stream and wait for
// nothing.  Reading back and closing wait for `ev` on the host, so only for the
// set's own work.
//
// replica_range is the readers' check of first and n against the set.  What the four
// delay stages share beyond that, the record reader of their kernels and delay_add
// around their launches, is in delay_stage.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <new>
#include <string>

#include "common.h"

namespace pu {

inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// The first / n / out check of a reader `who` ("pu_x_read") of replicas [first, first + n)
// of a set that holds set_count (0: there is no set); have_out: the output is there, which
// only n > 0 needs.  1: nothing to do (n == 0), 0: go on, else PU_E* with the error text.
inline int replica_range(int set_count, int first, int n, bool have_out, const char* who) {
    if (set_count < 1 || first < 0 || n < 0 || (!have_out && n)) return set_error(PU_EINVAL, std::string(who) + ": bad arguments");
    if ((int64_t)first + n > set_count) return set_error(PU_ERANGE, "more replicas than the set holds");
    return n == 0 ? 1 : 0;
}

struct DeviceSet {
    int device = 0;
    hipStream_t stream = nullptr;   // the set's own stream
    hipStream_t last = nullptr;     // the stream of the last call
    hipEvent_t ev = nullptr;        // recorded after every call: the set's outstanding work
    bool ev_recorded = false;
    uint8_t* base = nullptr;
    size_t bytes = 0;

    int use() { return hipSetDevice(device) == hipSuccess ? 0 : set_error(PU_ENODEV, "hipSetDevice failed"); }

    // The device, the set's stream and event, and `nbytes` of device memory for `what`
    // ("pu_x_open: the state of ..."); after a failure the caller releases the set.
    int open(int dev, size_t nbytes, const std::string& what) {
        device = dev;
        bytes = nbytes;
        if (use() != 0) return PU_ENODEV;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess)
            return set_error(PU_EIO, "stream create failed");
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return set_error(PU_EIO, "event create failed");
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return set_error(PU_ENOMEM, what + ": " + std::to_string(bytes) + " bytes of device memory could not be allocated");
        }
        base = (uint8_t*)p;
        return 0;
    }

    hipStream_t pick(void* hip_stream) const { return hip_stream ? (hipStream_t)hip_stream : stream; }

    // Around a launch on `st`: it is ordered after the set's last call, and becomes the last call.
    int order_before(hipStream_t st) {
        if (st != last && ev_recorded && hipStreamWaitEvent(st, ev, 0) != hipSuccess)
            return set_error(PU_EIO, "ordering the call after the set's last call failed");
        return 0;
    }
    int record_after(hipStream_t st, const char* what) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return set_error(PU_EIO, std::string(what) + ": launch failed: " + hipGetErrorString(e));
        if (hipEventRecord(ev, st) != hipSuccess) return set_error(PU_EIO, "event record failed");
        ev_recorded = true;
        last = st;
        return 0;
    }

    // Waits for the set's outstanding calls only: the event of its last launch
    // (every launch on another stream first waits for the one before it).
    int wait_outstanding() {
        if (ev_recorded && hipEventSynchronize(ev) != hipSuccess)
            return set_error(PU_EIO, "waiting for the set's outstanding calls failed");
        return 0;
    }

    // Reads state back to the host once the set's outstanding calls are done:
    // copy(stream) issues the asynchronous copies (true: all were issued), then
    // the stream is synchronised.  On the set's own (non-blocking) stream: a
    // copy on the null stream would wait for every blocking stream.
    template <class Copy>
    int read_back(Copy copy, const char* failed) {
        int rc = use();
        if (!rc) rc = wait_outstanding();
        if (rc) return rc;
        if (!copy(stream) || hipStreamSynchronize(stream) != hipSuccess) return set_error(PU_EIO, failed);
        return 0;
    }

    // Whatever open() got as far as creating; the caller has waited for outstanding calls.
    void release() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (base) (void)hipFree(base);
        if (ev) (void)hipEventDestroy(ev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// A stage's handle S derives from DeviceSet: new_set gives an empty one (NULL
// and the error text when the host has no memory), drop_set ends one that
// failed to open (the error text is the failure's, or the one given) and
// close_set one that is no longer used, after its outstanding calls.
template <class S>
S* new_set() {
    S* s = new (std::nothrow) S;
    if (!s) set_error(PU_ENOMEM, "out of host memory");
    return s;
}
template <class S>
S* drop_set(S* s) {
    s->release();
    delete s;
    return nullptr;
}
template <class S>
S* drop_set(S* s, int code, const char* msg) {
    set_error(code, msg);
    return drop_set(s);
}
template <class S>
void close_set(S* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)s->wait_outstanding();
    drop_set(s);
}

}  // namespace pu
