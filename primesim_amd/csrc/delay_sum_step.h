// delay_sum_step.h — the rule of the delay summaries (pu_dsum_*,
// include/primeuncore.h), shared by the host fold (pu_dsum_host_add) and the
// device kernel (delay_sum.hip): the range of core ids, a delay's bucket, and
// the fold of one (class, delay) pair into a summary.  A record's class and core
// id are delay_record_step.h's, named here too for whoever states the summaries'
// rule whole.  Everything here compiles as plain C++ on the host (PU_HD is empty
// there) and as __host__ __device__ under hipcc's HIP mode.  All of it is integer
// and independent of order, so any split of the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "delay_record_step.h"
#include "pu_hd.h"

namespace pu_delay_sum {

using pu_delay_record::class_of_mem_type;
using pu_delay_record::class_of_req16_b;
using pu_delay_record::core_of_req16_b;

// Without a core count only a negative id is out of range.
constexpr uint32_t kNoCoreLimit = 0x80000000u;
PU_HD inline uint32_t core_limit(int32_t num_cores) { return num_cores > 0 ? (uint32_t)num_cores : kNoCoreLimit; }
// core < 0 or core >= limit, as one unsigned comparison
PU_HD inline bool core_out_of_range(int32_t core, uint32_t limit) { return (uint32_t)core >= limit; }

// d <= 0 -> 0; otherwise the number of significant bits of d: 1 -> 1, 2..3 -> 2,
// 4..7 -> 3, ..., 2^30..2^31-1 -> 31.
PU_HD inline int bucket_of(int32_t d) { return d <= 0 ? 0 : 32 - __builtin_clz((uint32_t)d); }

PU_HD inline void class_init(pu_dsum_class* c) {
    c->count = 0;
    c->sum = 0;
    c->min = INT32_MAX;
    c->max = INT32_MIN;
    for (int i = 0; i < PU_DSUM_BUCKETS; i++) c->hist[i] = 0;
}

PU_HD inline void replica_init(pu_dsum_replica* r) {
    class_init(&r->cls[0]);
    class_init(&r->cls[1]);
    r->core_out_of_range = 0;
}

PU_HD inline void fold_one(pu_dsum_class* c, int32_t d) {
    c->count++;
    c->sum += d;
    if (d < c->min) c->min = d;
    if (d > c->max) c->max = d;
    c->hist[bucket_of(d)]++;
}

}  // namespace pu_delay_sum
