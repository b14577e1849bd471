// delay_record_step.h — what a delay stage (pu_dsum_*, pu_dhist_*, pu_dtail_*,
// pu_dseries_*, include/primeuncore.h) needs to know of a request record: its class,
// its core id and its timer, from the words the device kernels load (delay_stage.h)
// and from record i of a host array.  Shared by the four stages' rules
// (delay_sum_step.h, delay_hist_step.h, delay_tail_step.h, delay_series_step.h) on
// both sides: plain C++ on the host (PU_HD is empty there), __host__ __device__
// under hipcc's HIP mode.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "pu_hd.h"

namespace pu_delay_record {

// Class 0 is a read, class 1 a write.  The engine passes pu_req.mem_type on
// unchanged as Req.type (engine.hip: replica_steps) and takes the write path
// only where that equals PU_WR; PU_RD, PU_WB and every other value go the other
// way.  pu_req16 carries one bit of it (PU_REQ16_TYPE).
PU_HD inline int class_of_mem_type(uint32_t mem_type) { return mem_type == (uint32_t)PU_WR ? 1 : 0; }
PU_HD inline int class_of_req16_b(uint64_t b) { return PU_REQ16_TYPE(b); }
PU_HD inline int32_t core_of_req16_b(uint64_t b) { return PU_REQ16_CORE(b); }
PU_HD inline int64_t timer_of_req16_b(uint64_t b) { return PU_REQ16_TIMER(b); }

// record i of an array of pu_req (PU_REQ_FMT_32) or pu_req16 (PU_REQ_FMT_16)
PU_HD inline int class_at(const void* reqs, int fmt, size_t i) {
    return fmt == PU_REQ_FMT_16 ? class_of_req16_b(((const pu_req16*)reqs)[i].b)
                                : class_of_mem_type(((const pu_req*)reqs)[i].mem_type);
}
PU_HD inline int32_t core_at(const void* reqs, int fmt, size_t i) {
    return fmt == PU_REQ_FMT_16 ? core_of_req16_b(((const pu_req16*)reqs)[i].b) : ((const pu_req*)reqs)[i].core;
}
PU_HD inline int64_t timer_at(const void* reqs, int fmt, size_t i) {
    return fmt == PU_REQ_FMT_16 ? timer_of_req16_b(((const pu_req16*)reqs)[i].b) : ((const pu_req*)reqs)[i].timer;
}

}  // namespace pu_delay_record
