// stats_rule_check.cpp — the rule that forms a pu_stats
// (primesim_amd/csrc/stats_rule.h, pu::stats_fill) against literals: an
// EngineStats whose word i holds 1000 + i and level rows lv[k][j] = 2000 + 4k + j
// go into a pu_stats pre-filled with 0xA5, for 1 and for 4 levels; every field
// must hold the literal it is due, the levels at or above num_levels zero, _pad
// zero, and no byte may be left as it was.  Host only (tests/test_dres_abi.py
// builds it with the host's address and undefined-behaviour sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../primesim_amd/csrc/stats_rule.h"

static int g_checked = 0;

static bool eq(const char* what, int num_levels, uint64_t got, uint64_t want) {
    g_checked++;
    if (got == want) return true;
    std::printf("FAIL num_levels %d: %s is %llu, expected %llu\n", num_levels, what, (unsigned long long)got,
                (unsigned long long)want);
    return false;
}

static bool row(const char* what, int num_levels, const pu_level_stats& s, uint64_t first) {
    // first == 0: the row is all zero; else {first, first + 1, first + 2, first + 3}
    return eq(what, num_levels, s.ins, first) && eq(what, num_levels, s.miss, first ? first + 1 : 0) &&
           eq(what, num_levels, s.evict, first ? first + 2 : 0) && eq(what, num_levels, s.wb, first ? first + 3 : 0);
}

static bool check(int num_levels) {
    static_assert(sizeof(EngineStats) == 43 * 8, "EngineStats is 43 words");
    uint64_t words[43];
    for (int i = 0; i < 43; i++) words[i] = 1000 + (uint64_t)i;
    EngineStats es;
    std::memcpy(&es, words, sizeof es);
    uint64_t lv[pu::kStatRows][4];
    for (int k = 0; k < pu::kStatRows; k++)
        for (int j = 0; j < 4; j++) lv[k][j] = 2000 + 4 * (uint64_t)k + (uint64_t)j;

    pu_stats st;
    std::memset(&st, 0xA5, sizeof st);
    pu::stats_fill(st, es, num_levels, lv);

    const int nl = num_levels;
    bool ok = eq("net_accesses", nl, st.net_accesses, 1000) && eq("net_distance", nl, st.net_distance, 1001) &&
              eq("net_total_delay", nl, st.net_total_delay, 1002) && eq("net_router_delay", nl, st.net_router_delay, 1003) &&
              eq("net_link_delay", nl, st.net_link_delay, 1004) && eq("net_inject_delay", nl, st.net_inject_delay, 1005) &&
              eq("dram_accesses", nl, st.dram_accesses, 1006) && eq("total_bus_contention", nl, st.total_bus_contention, 1007) &&
              eq("total_num_broadcast", nl, (uint64_t)st.total_num_broadcast, 1008) &&
              eq("num_levels", nl, (uint64_t)(int64_t)st.num_levels, (uint64_t)(int64_t)num_levels) &&
              eq("_pad", nl, (uint64_t)(int64_t)st._pad, 0) &&
              row("level[0]", nl, st.level[0], 2000) && row("level[1]", nl, st.level[1], num_levels > 1 ? 2004 : 0) &&
              row("level[2]", nl, st.level[2], num_levels > 2 ? 2008 : 0) &&
              row("level[3]", nl, st.level[3], num_levels > 3 ? 2012 : 0) && row("directory", nl, st.directory, 2016) &&
              row("tlb", nl, st.tlb, 2020) && eq("link_flits", nl, st.link_flits, 1009) &&
              eq("mg1_calls", nl, st.mg1_calls, 1010) && eq("lockdown_calls", nl, st.lockdown_calls, 1011) &&
              eq("bus_accesses", nl, st.bus_accesses, 1012) && eq("requests", nl, st.requests, 1013) &&
              eq("error_flags", nl, st.error_flags, 1014) && eq("dram_row_hits", nl, st.dram_row_hits, 1015) &&
              eq("dram_row_empty", nl, st.dram_row_empty, 1016) &&
              eq("dram_row_conflicts", nl, st.dram_row_conflicts, 1017) && eq("dram_bank_wait", nl, st.dram_bank_wait, 1018);
    if (!ok) return false;

    // every byte was written: no 8-B word of the record still holds the fill
    static_assert(sizeof(pu_stats) % 8 == 0, "pu_stats is whole words");
    uint64_t w[sizeof(pu_stats) / 8];
    std::memcpy(w, &st, sizeof st);
    for (size_t i = 0; i < sizeof(pu_stats) / 8; i++)
        if ((uint32_t)w[i] == 0xA5A5A5A5u || (uint32_t)(w[i] >> 32) == 0xA5A5A5A5u) {
            std::printf("FAIL num_levels %d: word %zu of pu_stats was not written\n", num_levels, i);
            return false;
        }
    return true;
}

int main() {
    // the fields compared above are all of pu_stats: 10 words, 6 rows of 4, 10 words
    static_assert(sizeof(pu_stats) == (10 + 6 * 4 + 10) * 8, "a field was added to pu_stats: compare it here");
    if (!check(1) || !check(4)) return 1;
    std::printf("OK %d fields\n", g_checked);
    return 0;
}
