// delay_tail_step.h — the rule of the slowest-request lists (pu_dtail_*,
// include/primeuncore.h), shared by the host fold (pu_dtail_host_add) and the
// device kernels (delay_tail.hip): the order of two entries, a record as an entry,
// and the sorted insertion that keeps a list of the best k.  A record's class is
// delay_record_step.h's.  Everything here compiles as plain C++ on the host (PU_HD
// is empty there) and as __host__ __device__ under hipcc's HIP mode.  All of it is
// integer, and a list is a function of the set of (delay, position) pairs seen, so
// any split of the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "delay_record_step.h"
#include "pu_hd.h"

namespace pu_delay_tail {

using pu_delay_record::class_at;

static_assert(sizeof(pu_dtail_entry) == 32, "three 8-byte and two 4-byte fields, no padding");

// x is better than y: the larger delay, at equal delays the earlier position.
// Positions of a replica are distinct, so of two different entries exactly one is
// better: a strict total order.
PU_HD inline bool better(int32_t dx, uint64_t px, int32_t dy, uint64_t py) { return dx > dy || (dx == dy && px < py); }
PU_HD inline bool better(const pu_dtail_entry& x, const pu_dtail_entry& y) {
    return better(x.delay, x.position, y.delay, y.position);
}

PU_HD inline pu_dtail_entry entry_of(const pu_req& q, int32_t delay, uint64_t position) {
    return pu_dtail_entry{q.addr, q.timer, position, delay, q.core};
}
PU_HD inline pu_dtail_entry entry_of(const pu_req16& q, int32_t delay, uint64_t position) {
    return pu_dtail_entry{q.a, PU_REQ16_TIMER(q.b), position, delay, pu_delay_record::core_of_req16_b(q.b)};
}
// record i of an array of pu_req (PU_REQ_FMT_32) or pu_req16 (PU_REQ_FMT_16)
PU_HD inline pu_dtail_entry entry_at(const void* reqs, int fmt, size_t i, int32_t delay, uint64_t position) {
    return fmt == PU_REQ_FMT_16 ? entry_of(((const pu_req16*)reqs)[i], delay, position)
                                : entry_of(((const pu_req*)reqs)[i], delay, position);
}

// The number of the list's entries (best first, `count` of them) that are better than (delay, position).
PU_HD inline uint32_t rank_in(const pu_dtail_entry* list, uint32_t count, int32_t delay, uint64_t position) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (better(list[mid].delay, list[mid].position, delay, position))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// True when (delay, position) belongs among the best k of the list and it.
PU_HD inline bool enters(const pu_dtail_entry* list, uint32_t count, int k, int32_t delay, uint64_t position) {
    return count < (uint32_t)k || better(delay, position, list[k - 1].delay, list[k - 1].position);
}

// Keeps list the best min(k, entries offered) entries, best first: e goes where its rank
// puts it, the entries behind it move down one and the k-th falls out.
PU_HD inline void insert(pu_dtail_entry* list, uint32_t* count, int k, const pu_dtail_entry& e) {
    if (!enters(list, *count, k, e.delay, e.position)) return;
    const uint32_t at = rank_in(list, *count, e.delay, e.position);
    if (*count < (uint32_t)k) ++*count;
    for (uint32_t j = *count - 1; j > at; j--) list[j] = list[j - 1];
    list[at] = e;
}

// n records added to one replica's lists: entries [2][k], counts [2], *seen.  (enters() is asked
// first so that only a record that enters is read in full.)
PU_HD inline void fold(pu_dtail_entry* entries, uint32_t* counts, uint64_t* seen, int k, const void* reqs, int fmt,
                       const int32_t* delays, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const int c = class_at(reqs, fmt, i);
        pu_dtail_entry* const list = entries + (size_t)c * (size_t)k;
        const uint64_t position = *seen + i;
        if (enters(list, counts[c], k, delays[i], position)) insert(list, &counts[c], k, entry_at(reqs, fmt, i, delays[i], position));
    }
    *seen += n;
}

}  // namespace pu_delay_tail
