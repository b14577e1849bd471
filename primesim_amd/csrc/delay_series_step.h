// delay_series_step.h — the rule of the epoch series (pu_dseries_*,
// include/primeuncore.h), shared by the host fold (pu_dseries_host_add) and the
// device kernels (delay_series.hip): the epoch of a record's timer, the fold of one
// delay into a cell and the merge of two cells.  A record's class and timer are
// delay_record_step.h's.  Everything here compiles as plain C++ on the host (PU_HD
// is empty there) and as __host__ __device__ under hipcc's HIP mode.  All of it is
// integer and independent of order (sums, counts and a maximum), so any split of
// the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "delay_record_step.h"
#include "pu_hd.h"

namespace pu_delay_series {

using pu_delay_record::class_at;
using pu_delay_record::timer_at;

constexpr int kMaxEpochs = PU_DSERIES_MAX_EPOCHS;
constexpr int kMaxShift = 62;
static_assert(sizeof(pu_dseries_cell) == 32, "three 8-byte and two 4-byte fields, no padding");

PU_HD inline bool epochs_ok(int epochs) { return epochs >= 1 && epochs <= kMaxEpochs; }
PU_HD inline bool shift_ok(int shift) { return shift >= 0 && shift <= kMaxShift; }

// Epoch 0 holds every timer below t0 + 2^shift, epoch E - 1 every timer from
// t0 + (E - 1) * 2^shift on: the first and the last epoch are catch-alls and no record
// is dropped.  The distance is taken unsigned, so it is defined for any two int64.
PU_HD inline int epoch_of(int64_t timer, int epochs, int64_t t0, int shift) {
    if (timer < t0) return 0;
    const uint64_t e = ((uint64_t)timer - (uint64_t)t0) >> shift;
    return e < (uint64_t)(epochs - 1) ? (int)e : epochs - 1;
}

// The cell of (class, epoch) in a replica's pu_dseries_cell cells[2][epochs].
PU_HD inline int key_of(int cls, int epoch, int epochs) { return cls * epochs + epoch; }

// An empty cell is all zeros: max is the largest of max(d, 0).
PU_HD inline void fold_one(pu_dseries_cell* c, int32_t d) {
    c->count++;
    c->sum += d;
    c->nonpos += d <= 0 ? 1u : 0u;
    if (d > c->max) c->max = d;
}

PU_HD inline void merge(pu_dseries_cell* into, const pu_dseries_cell& from) {
    into->count += from.count;
    into->sum += from.sum;
    into->nonpos += from.nonpos;
    if (from.max > into->max) into->max = from.max;
}

// n records added to one replica's cells[2][epochs].
PU_HD inline void fold(pu_dseries_cell* cells, int epochs, int64_t t0, int shift, const void* reqs, int fmt,
                       const int32_t* delays, size_t n) {
    for (size_t i = 0; i < n; i++)
        fold_one(cells + key_of(class_at(reqs, fmt, i), epoch_of(timer_at(reqs, fmt, i), epochs, t0, shift), epochs), delays[i]);
}

}  // namespace pu_delay_series
