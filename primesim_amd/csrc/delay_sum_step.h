// delay_sum_step.h — the rule of the delay summaries (pu_dsum_*,
// include/primeuncore.h), shared by the host fold (pu_dsum_host_add) and the
// device kernel (delay_sum.hip): a request's class, its core id, a delay's
// bucket, and the fold of one (class, delay) pair into a summary.  Everything
// here compiles as plain C++ on the host (PU_HD is empty there) and as
// __host__ __device__ under hipcc's HIP mode.  All of it is integer and
// independent of order, so any split of the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "pu_hd.h"

namespace pu_delay_sum {

// Class 0 is a read, class 1 a write.  The engine passes pu_req.mem_type on
// unchanged as Req.type (engine.hip: replica_steps) and takes the write path
// only where that equals PU_WR; PU_RD, PU_WB and every other value go the other
// way.  pu_req16 carries one bit of it (PU_REQ16_TYPE).
PU_HD inline int class_of_mem_type(uint32_t mem_type) { return mem_type == (uint32_t)PU_WR ? 1 : 0; }
PU_HD inline int class_of_req16_b(uint64_t b) { return PU_REQ16_TYPE(b); }
PU_HD inline int32_t core_of_req16_b(uint64_t b) { return PU_REQ16_CORE(b); }

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
