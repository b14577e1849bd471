// delay_stage.h — what the four delay stages (delay_sum.hip, delay_hist.hip,
// delay_tail.hip, delay_series.hip) share below device_set.h: every one folds each
// replica's records [d_begin[r], d_end[r]) of one request array and one delay array,
// by one launch per call with one workgroup of kThreads per replica.  Included by
// those four files only; everything is local to the file that includes it.
//
// Device side.  RecordRange is the workgroup's range and RecordSource loads its
// records: lanes take consecutive records, kUnroll per lane and trip.  Of the
// delays one dword is loaded per lane, naturally aligned whatever d_begin is; of a
// record the one word that holds what the stage asks for:
//   the class alone       8 B: pu_req16.b, or the last word of a pu_req (mem_type | ...)
//   the core id as well   pu_req16.b again (8 B), or the second half of a pu_req
//                         (16 B: core | prog_id, mem_type | ...)
//   the timer as well     pu_req16.b again (8 B), or two 8-B words of a pu_req (timer,
//                         mem_type | ...): TimedRecordSource, the epoch series' own
// In the first two cases that is the record's last word of its size, so one stride
// arithmetic serves.  The trip loop and the accumulation are the stage's: the
// helpers here are straight-line on purpose.  They are inlined after they have been
// optimised on their own, and a loop or a decode of two fields moved in here
// compiled the kernels to other code than the same text written in the kernel;
// as they stand every kernel is instruction for instruction what it was
// (profiles/refactor_delay_stages_isa.txt).  zero_words_kernel zeroes a stage's
// state for its reset.
//
// Host side.  delay_add is pu_d*_add: the argument check, the set's ordering rule
// around the launch, and the record format as a compile-time constant for the
// stage's launcher.  reset_words is the reset of a stage whose state is zeros.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/primeuncore.h"
#include "common.h"
#include "delay_record_step.h"
#include "device_set.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;   // records per lane and trip

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// The records of this workgroup's replica: [b, e) of the request and delay arrays.
struct RecordRange {
    uint64_t b, e;

    __device__ RecordRange(const uint64_t* d_begin, const uint64_t* d_end)
        : b(d_begin[(int)blockIdx.x]), e(d_end[(int)blockIdx.x]) {}

    // the whole workgroup: nothing to add
    __device__ bool empty() const { return b >= e; }
    __device__ uint64_t len() const { return e - b; }
};

constexpr uint64_t kTrip = (uint64_t)kThreads * kUnroll;   // records of a workgroup's trip

// Where the records of a range are and what of a record the stage asks for (CORE: the
// core id as well as the class).  A stage's trip is
//     for (u < kUnroll) valid[u] = src.load(base + u * kThreads + tid, d[u], w[u]);
//     for (u < kUnroll) ... valid[u], d[u], src.cls(w[u]) ...
// in two loops, so that all loads of the trip are issued before any is used.
template <int FMT, bool CORE>
struct RecordSource {
    typedef typename std::conditional<CORE, u64x2, u64>::type Word;                               // kept of a record
    typedef typename std::conditional<CORE && FMT == PU_REQ_FMT_32, u64x2, u64>::type Loaded;     // loaded of it
    // a record's last word of that size
    static constexpr int kStride = (int)((FMT == PU_REQ_FMT_16 ? sizeof(pu_req16) : sizeof(pu_req)) / sizeof(Loaded));

    const int32_t* dl;
    const Loaded* wd;
    uint64_t len;

    __device__ RecordSource(const void* reqs, const int32_t* delay, uint64_t b, uint64_t len_)
        : dl(delay + b), wd((const Loaded*)reqs + (uint64_t)kStride * b + (kStride - 1)), len(len_) {}

    // Record i of the range into (d, w), of a pu_req16 with the core id into w.x; false, and
    // zeros, at and past the range's end.
    __device__ bool load(uint64_t i, int32_t& d, Word& w) const {
        const bool valid = i < len;
        d = 0;
        w = Word{};
        if (valid) {
            d = dl[i];
            if constexpr (sizeof(Loaded) == sizeof(Word))
                w = wd[(uint64_t)kStride * i];
            else
                w.x = wd[(uint64_t)kStride * i];
        }
        return valid;
    }

    // The class of a word loaded for the class alone.  With the core id the word is the delay
    // summaries' own to take apart (delay_sum.hip): x holds pu_req16.b, or core | prog_id of a
    // pu_req with mem_type | ... in y.
    __device__ static int cls(Word w) {
        static_assert(!CORE, "a word with the core id is taken apart by its stage");
        return FMT == PU_REQ_FMT_16 ? pu_delay_record::class_of_req16_b(w)
                                    : pu_delay_record::class_of_mem_type((uint32_t)(w & 0xFFu));
    }
};

// The same range for a stage that asks for a record's timer beside its class (the epoch
// series, delay_series.hip): of a pu_req16 the word b alone, as above (8 B: the timer is in
// its low bits); of a pu_req the timer (offset 8) and the last word (offset 24), two 8-B
// loads in the one 32-B record, so the lines touched are those of RecordSource.  A source of
// its own, so that RecordSource instantiates for the other three stages what it always did.
template <int FMT>
struct TimedRecordSource {
    static constexpr int kStride = (int)((FMT == PU_REQ_FMT_16 ? sizeof(pu_req16) : sizeof(pu_req)) / sizeof(u64));
    static constexpr int kTimerWord = 1;   // pu_req.timer

    const int32_t* dl;
    const u64* wd;   // the range's first record
    uint64_t len;

    __device__ TimedRecordSource(const void* reqs, const int32_t* delay, uint64_t b, uint64_t len_)
        : dl(delay + b), wd((const u64*)reqs + (uint64_t)kStride * b), len(len_) {}

    // Record i of the range into (d, t, w): w the record's last word, t the timer word of a
    // pu_req (0 for a pu_req16, whose timer is in w); false, and zeros, at and past the range's end.
    __device__ bool load(uint64_t i, int32_t& d, u64& t, u64& w) const {
        const bool valid = i < len;
        d = 0;
        t = 0;
        w = 0;
        if (valid) {
            d = dl[i];
            w = wd[(uint64_t)kStride * i + (kStride - 1)];
            if constexpr (FMT == PU_REQ_FMT_32) t = wd[(uint64_t)kStride * i + kTimerWord];
        }
        return valid;
    }

    __device__ static int cls(u64 w) { return RecordSource<FMT, false>::cls(w); }
    __device__ static int64_t timer(u64 t, u64 w) {
        return FMT == PU_REQ_FMT_16 ? pu_delay_record::timer_of_req16_b(w) : (int64_t)t;
    }
};

__global__ __launch_bounds__(kThreads) void zero_words_kernel(u64* p, size_t words) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < words) p[i] = 0;
}

// pu_d*_reset of a stage whose cleared state is `words` 64-bit zeros at p: on the
// set's own stream, after the set's last call.
int reset_words(pu::DeviceSet* s, void* p, size_t words, const char* who) {
    int rc = s->use();
    if (!rc) rc = s->order_before(s->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, s->stream,
                       (u64*)p, words);
    return s->record_after(s->stream, who);
}

// pu_d*_add: launch(F, st) launches the stage's add kernel for record format
// decltype(F)::value on stream st, one workgroup of kThreads per replica.
template <class Launch>
int delay_add(pu::DeviceSet* s, const char* who, const void* d_reqs, int fmt, const int32_t* d_delay, const uint64_t* d_begin,
              const uint64_t* d_end, void* hip_stream, Launch launch) {
    if (!s || !pu::req_fmt_ok(fmt) || !d_reqs || !d_delay || !d_begin || !d_end || ((uintptr_t)d_reqs & 15))
        return pu::set_error(PU_EINVAL, std::string(who) + ": bad arguments");
    int rc = s->use();
    if (rc) return rc;
    hipStream_t st = s->pick(hip_stream);
    rc = s->order_before(st);
    if (rc) return rc;
    if (fmt == PU_REQ_FMT_16)
        launch(std::integral_constant<int, PU_REQ_FMT_16>{}, st);
    else
        launch(std::integral_constant<int, PU_REQ_FMT_32>{}, st);
    return s->record_after(st, who);
}

}  // namespace
