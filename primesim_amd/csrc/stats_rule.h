// stats_rule.h — the one rule that turns a replica's EngineStats (geometry.h)
// and its per-level counter sums into a pu_stats (include/primeuncore.h), shared
// by pu_stats_get (report.cpp), lane 0 of dres_gather_kernel (run_results.hip)
// and the stand-alone check (tests/cpp/stats_rule_check.cpp).  A counter added to
// pu_stats is added here, once.  Compiles as plain C++ on the host (PU_HD is
// empty there) and as __host__ __device__ under hipcc's HIP mode.
#pragma once

#include <cstdint>

#include "../../include/primeuncore.h"
#include "geometry.h"
#include "pu_hd.h"

namespace pu {

constexpr int kStatRows = 6;   // EngineStats.lvl_cnt rows: levels 0-3, PU_CNT_DIR, PU_CNT_TLB

// Writes every byte of `out`.  lv[k] is row k's {ins, miss, evict, wb}, already
// EngineStats.lvl_cnt[k] plus the per-cache counters of that row; levels at or
// above num_levels read as zero whatever lv holds for them, and so does _pad.
PU_HD inline void stats_fill(pu_stats& out, const EngineStats& es, int num_levels, const uint64_t lv[kStatRows][4]) {
    out.net_accesses = es.net_accesses;
    out.net_distance = es.net_distance;
    out.net_total_delay = es.net_total_delay;
    out.net_router_delay = es.net_router_delay;
    out.net_link_delay = es.net_link_delay;
    out.net_inject_delay = es.net_inject_delay;
    out.dram_accesses = es.dram_accesses;
    out.total_bus_contention = es.total_bus_contention;
    out.total_num_broadcast = es.total_num_broadcast;
    out.num_levels = num_levels;
    out._pad = 0;
    for (int l = 0; l < PU_MAX_LEVELS; l++)
        out.level[l] = l < num_levels ? pu_level_stats{lv[l][0], lv[l][1], lv[l][2], lv[l][3]} : pu_level_stats{0, 0, 0, 0};
    out.directory = pu_level_stats{lv[PU_CNT_DIR][0], lv[PU_CNT_DIR][1], lv[PU_CNT_DIR][2], lv[PU_CNT_DIR][3]};
    out.tlb = pu_level_stats{lv[PU_CNT_TLB][0], lv[PU_CNT_TLB][1], lv[PU_CNT_TLB][2], lv[PU_CNT_TLB][3]};
    out.link_flits = es.link_flits;
    out.mg1_calls = es.mg1_calls;
    out.lockdown_calls = es.lockdown_calls;
    out.bus_accesses = es.bus_accesses;
    out.requests = es.requests;
    out.error_flags = es.error_flags;
    out.dram_row_hits = es.dram_row_hits;
    out.dram_row_empty = es.dram_row_empty;
    out.dram_row_conflicts = es.dram_row_conflicts;
    out.dram_bank_wait = es.dram_bank_wait;
}

static_assert(sizeof(EngineStats::lvl_cnt) == kStatRows * 4 * sizeof(uint64_t) && PU_MAX_LEVELS == 4 &&
                  PU_CNT_DIR == 4 && PU_CNT_TLB == 5,
              "lv is indexed like EngineStats.lvl_cnt");

}  // namespace pu
