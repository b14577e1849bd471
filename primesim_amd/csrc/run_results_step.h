// run_results_step.h — the rules of the end-of-run results (pu_dres_*,
// include/primeuncore.h), shared by the device kernels (run_results.hip), the
// host gather (pu_dres_host_gather) and the stand-alone check
// (tests/cpp/queue_header_check.cpp): the decode of a queue header's visit
// counts, the fold of the per-core completion cycles, and the tie rule of a
// maximum.  Everything here compiles as plain C++ on the host (PU_HD is empty
// there) and as __host__ __device__ under hipcc's HIP mode.  All of it is
// integer and independent of order, so any split of the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pu_hd.h"

namespace pu_run_results {

// The engine's packed queue header, restated (engine.hip q_store_hdr / hdr_state; engine.hip is
// embedded for the per-configuration compile and cannot include this file, so
// tests/test_gpu_dres.py is what pins the two together).  32 B per queue, two
// 16-B pieces; the first, a = {n | head, n1 | count}, is four dwords:
//   dwords 0-1  n, every visit of the queue, an exact double
//   dwords 2-3  n1, the visits with the block packet length, an exact double
// Both counts are integers below 2^45, so the low 7 mantissa bits of each
// double are zero and carry the ring cursor (head, count) instead.
constexpr uint32_t kHdrBytes = 32;     // PU_HDR_BYTES
constexpr uint32_t kHdrCursor = 0x7Fu; // PU_HDR_CUR

// One count of piece a: the double whose low dword is `lo` without the cursor
// bits and whose high dword is `hi`, as an integer.
PU_HD inline uint64_t count_of(uint32_t lo, uint32_t hi) {
    const uint64_t bits = ((uint64_t)hi << 32) | (uint64_t)(lo & ~kHdrCursor);
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return (uint64_t)d;
}

// The fold of the per-core completion cycles.  A core that has not completed a
// request holds kNoCycle (what the reset writes and pu_core_completion returns
// for it); every other value counts, whatever its sign.
constexpr int64_t kNoCycle = -1;
struct Completion {
    int32_t done;
    int64_t max, min, sum;
};
PU_HD inline Completion completion_init() { return Completion{0, INT64_MIN, INT64_MAX, 0}; }
PU_HD inline void completion_fold(Completion& c, int64_t cycle) {
    if (cycle == kNoCycle) return;
    c.done++;
    c.max = cycle > c.max ? cycle : c.max;
    c.min = cycle < c.min ? cycle : c.min;
    c.sum = (int64_t)((uint64_t)c.sum + (uint64_t)cycle);
}
PU_HD inline void completion_merge(Completion& c, const Completion& o) {
    c.done += o.done;
    c.max = o.max > c.max ? o.max : c.max;
    c.min = o.min < c.min ? o.min : c.min;
    c.sum = (int64_t)((uint64_t)c.sum + (uint64_t)o.sum);
}

// The busiest queue of a range: the largest count, and among equal counts the
// lowest id.  id -1 is "no queue" (an empty range) and loses against every
// queue, one with no visit included: a range of queues none of which was
// visited answers (0, its lowest id).
struct Busiest {
    uint64_t visits;
    int32_t id;
};
PU_HD inline Busiest busiest_init() { return Busiest{0, -1}; }
PU_HD inline bool busiest_beats(uint64_t v, int32_t id, const Busiest& b) {
    return id >= 0 && (b.id < 0 || v > b.visits || (v == b.visits && id < b.id));
}
PU_HD inline void busiest_take(Busiest& b, uint64_t v, int32_t id) {
    const bool t = busiest_beats(v, id, b);
    b.visits = t ? v : b.visits;
    b.id = t ? id : b.id;
}

}  // namespace pu_run_results
