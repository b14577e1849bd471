// report.cpp — what a run leaves behind, read back from a replica: its counters
// (read_replica, read_pages), the per-core completion cycles
// (pu_core_completion), the counters as a pu_stats (pu_stats_get, by the rule of
// stats_rule.h) and the report text (pu_report).
//
// Replaces:
//   UncoreManager::report           (reference src/uncore_manager.cpp:87-98)
//   System::report                  (reference src/system.cpp:956-1111)
//   ThreadSched::report             (reference src/thread_sched.cpp:105-116)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "handle.h"
#include "stats_rule.h"

// Copies replica r's engine-side counters.
int pu::read_replica(pu_handle* h, int r, EngineStats* es, std::vector<uint64_t> cnt[PU_MAX_LEVELS + 2],
                     std::vector<uint32_t> alive[PU_MAX_LEVELS + 2]) {
    int qrc = pu::resident_quiesce(h);
    if (qrc) return qrc;
    const Geo& g = h->geo;
    char* base = h->arena + (size_t)r * g.replica_bytes;
    HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
    HIP_TRY(hipMemcpy(es, base + g.off_stats, sizeof(EngineStats), hipMemcpyDeviceToHost), PU_EIO);
    // [num_levels + 1]: per-core TLB counters (ins, miss, evict, wb)
    cnt[g.num_levels + 1].assign(g.tlb_enable ? (size_t)g.num_cores * 4 : 0, 0);
    if (g.tlb_enable)
        HIP_TRY(hipMemcpy(cnt[g.num_levels + 1].data(), base + g.tlb.off_cnt, (size_t)g.num_cores * 32,
                          hipMemcpyDeviceToHost), PU_EIO);
    for (int l = 0; l <= g.num_levels; l++) {
        bool dir = l == g.num_levels;
        size_t nc = dir ? (size_t)g.N : (size_t)g.lv[l].ncaches;
        cnt[l].resize(nc * 4);
        alive[l].resize(nc);
        uint64_t oc = dir ? g.dir.off_cnt : g.lv[l].off_cnt;
        uint64_t oa = dir ? g.dir.off_alive : g.lv[l].off_alive;
        HIP_TRY(hipMemcpy(cnt[l].data(), base + oc, nc * 32, hipMemcpyDeviceToHost), PU_EIO);
        HIP_TRY(hipMemcpy(alive[l].data(), base + oa, nc * 4, hipMemcpyDeviceToHost), PU_EIO);
    }
    return 0;
}

// The page table of replica r (empty unless tlb_enable).
int pu::read_pages(pu_handle* h, int r, std::vector<PageEnt>* out) {
    const Geo& g = h->geo;
    out->clear();
    if (!g.tlb_enable) return 0;
    out->resize(g.tlb.pages_cap);
    char* base = h->arena + (size_t)r * g.replica_bytes;
    HIP_TRY(hipMemcpy(out->data(), base + g.tlb.off_pages, g.tlb.pages_cap * sizeof(PageEnt), hipMemcpyDeviceToHost),
            PU_EIO);
    return 0;
}

namespace {

// Cache::report (cache.cpp:430-441)
void cache_report(std::ostream& o, uint64_t size, uint64_t ways, const uint64_t* c) {
    o << "=================================================================\n";
    o << "Simulation results for " << size << " Bytes " << ways << "-way set associative cache model:\n";
    o << "The total # of memory instructions: " << c[0] << std::endl;
    o << "The # of cache-missed instructions: " << c[1] << std::endl;
    o << "The # of evicted instructions: " << c[2] << std::endl;
    o << "The # of writeback instructions: " << c[3] << std::endl;
    o << "The cache miss rate: " << 100 * (double)c[1] / (double)c[0] << "%" << std::endl;
    o << "=================================================================\n\n";
}

}  // namespace

extern "C" {

int pu_core_completion(pu_handle* h, int replica, int64_t* out, size_t n) {
    if (!h || !out) return pu::set_error(PU_EINVAL, "bad arguments");
    if (replica < 0 || replica >= h->R) return pu::set_error(PU_ERANGE, "replica out of range");
    size_t k = n < (size_t)h->geo.num_cores ? n : (size_t)h->geo.num_cores;
    int qrc = pu::resident_quiesce(h);
    if (qrc) return qrc;
    std::vector<int64_t> tmp((size_t)h->geo.num_cores);
    char* base = h->arena + (size_t)replica * h->geo.replica_bytes;
    HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
    HIP_TRY(hipMemcpy(tmp.data(), base + h->geo.off_completion, tmp.size() * 8, hipMemcpyDeviceToHost), PU_EIO);
    for (size_t i = 0; i < k; i++) out[i] = tmp[i];
    return 0;
}

int pu_stats_get(pu_handle* h, int replica, pu_stats* out) {
    if (!h || !out) return pu::set_error(PU_EINVAL, "bad arguments");
    if (replica < 0 || replica >= h->R) return pu::set_error(PU_ERANGE, "replica out of range");
    EngineStats es;
    std::vector<uint64_t> cnt[PU_MAX_LEVELS + 2];
    std::vector<uint32_t> alive[PU_MAX_LEVELS + 2];
    int rc = pu::read_replica(h, replica, &es, cnt, alive);
    if (rc) return rc;
    // lvl_cnt plus the per-cache counters: the levels, the directory ([num_levels]), the TLBs ([num_levels + 1])
    const int nl = h->geo.num_levels;
    uint64_t lv[pu::kStatRows][4];
    std::memcpy(lv, es.lvl_cnt, sizeof lv);
    for (int l = 0; l <= nl + 1; l++) {
        uint64_t* row = lv[l == nl ? PU_CNT_DIR : l == nl + 1 ? PU_CNT_TLB : l];
        for (size_t i = 0; i + 3 < cnt[l].size(); i += 4)
            for (int j = 0; j < 4; j++) row[j] += cnt[l][i + (size_t)j];
    }
    pu::stats_fill(*out, es, nl, lv);
    return 0;
}

// UncoreManager::report (uncore_manager.cpp:87-98) -> ThreadSched::report
// (thread_sched.cpp:105-116) -> System::report (system.cpp:956-1111) with
// Network::report (network.cpp:310-323) and Dram::report (dram.cpp:50-55).
long pu_report(pu_handle* h, int replica, int include_time, char* buf, size_t cap) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    if (replica < 0 || replica >= h->R) return pu::set_error(PU_ERANGE, "replica out of range");
    EngineStats es;
    std::vector<uint64_t> cnt[PU_MAX_LEVELS + 2];
    std::vector<uint32_t> alive[PU_MAX_LEVELS + 2];
    int rc = pu::read_replica(h, replica, &es, cnt, alive);
    if (rc) return rc;
    const Geo& g = h->geo;
    const pu_sys_cfg& y = h->cfg.sys;
    std::ostringstream o;
    o << "*********************************************************\n";
    o << "*                   PriME Simulator                     *\n";
    o << "*********************************************************\n\n";
    if (include_time) {                  // uncore_manager.cpp:92-93
        double sim_time = (double)(h->sim_finish.tv_sec - h->sim_start.tv_sec) +
                          (double)(h->sim_finish.tv_nsec - h->sim_start.tv_nsec) / 1000000000.0;
        o << "Total computation time: " << sim_time << " seconds\n";
    }
    o << std::endl;
    o << "Core Allocation:\n";
    for (const auto& kv : h->sched_of(replica).map)
        o << "(proc ID: " << kv.first.first << " ,thread ID: " << kv.first.second << ") => "
          << "core ID: " << kv.second << std::endl;
    o << std::endl;
    // Network::report
    double avg_delay = (double)es.net_total_delay / es.net_accesses;
    o << "Network Stat:\n";
    o << "# of accesses: " << es.net_accesses << std::endl;
    o << "Total network communication distance: " << es.net_distance << std::endl;
    o << "Total network delay: " << es.net_total_delay << std::endl;
    o << "Total router delay: " << es.net_router_delay << std::endl;
    o << "Total link delay: " << es.net_link_delay << std::endl;
    o << "Total inject delay: " << es.net_inject_delay << std::endl;
    o << "Total contention delay: " << es.net_link_delay - es.net_distance * y.network.link_delay << std::endl;
    o << "Average network delay: " << avg_delay << std::endl << std::endl;
    // Dram::report
    o << "DRAM Statistics:\n";
    o << "Total # of DRAM accesses: " << es.dram_accesses << std::endl;
    if (g.dram_banks > 0) {   // opt-in bank model (pu_dram_cfg): lines the reference never prints
        o << "DRAM banks: " << g.dram_banks << ", row bytes: " << y.dram.row_bytes << std::endl;
        o << "Row buffer hits: " << es.dram_row_hits << std::endl;
        o << "Row buffer misses (bank closed): " << es.dram_row_empty << std::endl;
        o << "Row buffer conflicts: " << es.dram_row_conflicts << std::endl;
        o << "Total bank wait cycles: " << es.dram_bank_wait << std::endl;
    }
    o << std::endl << "Simulation result for cache system: \n\n";
    if (y.verbose_report) {
        o << "Home Occupation:\n";
        const int w = g.net_width;
        if (g.net_type == 1) {
            o << "Allocated home locations in 3D coordinates:" << std::endl;
            for (int i = 0; i < g.N; i++)
                if (alive[g.num_levels][(size_t)i])
                    o << "(" << (i % (w * w)) % w << ", " << (i % (w * w)) / w << ", " << i / (w * w) << ")\n";
        } else {
            o << "Allocated home locations in 2D coordinates:" << std::endl;
            for (int i = 0; i < g.N; i++)
                if (alive[g.num_levels][(size_t)i]) o << "(" << i % w << ", " << i / w << ")\n";
        }
        o << std::endl;
    }
    o << std::endl;
    if (g.tlb_enable) {
        // system.cpp:990-1014 ("replaced" is never accumulated, Q16)
        const auto& tc = cnt[g.num_levels + 1];
        uint64_t ins = es.lvl_cnt[PU_CNT_TLB][0], miss = es.lvl_cnt[PU_CNT_TLB][1];
        for (size_t i = 0; i + 3 < tc.size(); i += 4) {
            ins += tc[i];
            miss += tc[i + 1];
        }
        double miss_rate = (double)miss / (double)ins;
        o << "TLB Cache" << "===========================================================\n";
        o << "Simulation results for " << y.tlb_cache.size << " Bytes " << y.tlb_cache.num_ways
          << "-way set associative cache model:\n";
        o << "The total # of TLB access instructions: " << ins << std::endl;
        o << "The # of cache-missed instructions: " << miss << std::endl;
        o << "The # of replaced instructions: " << 0 << std::endl;
        o << "The cache miss rate: " << 100 * miss_rate << "%" << std::endl;
        o << "=================================================================\n\n";
        if (y.verbose_report) {
            // PageTable::report (page_table.cpp:79-87): std::map order of (prog, vpage)
            std::vector<PageEnt> tab;
            int prc = pu::read_pages(h, replica, &tab);
            if (prc) return prc;
            std::vector<std::pair<std::pair<int, uint64_t>, uint64_t>> pages;
            for (const PageEnt& e : tab)
                if (e.used) pages.push_back({{e.prog, e.vpage}, e.ppage});
            std::sort(pages.begin(), pages.end());
            o << "Page translation:\n";
            o << "Total # of pages: " << pages.size() << std::endl;
            for (const auto& kv : pages)
                o << std::dec << "(proc ID: " << kv.first.first << " ,vpage Num: " << std::hex << kv.first.second
                  << ") => " << "ppage Num: " << kv.second << std::dec << std::endl;
        }
    }
    o << std::endl;
    o << "Total delay caused by bus contention: " << es.total_bus_contention << " cycles\n";
    o << "Total # of broadcast: " << (int)es.total_num_broadcast << "\n\n";
    for (int i = 0; i < g.num_levels; i++) {
        // per-level sums (compiled configuration, Geo.cnt_sum) + per-cache
        // counters of caches that exist (a counted cache always does)
        uint64_t ins = es.lvl_cnt[i][0], miss = es.lvl_cnt[i][1], evict = es.lvl_cnt[i][2], wb = es.lvl_cnt[i][3];
        for (size_t j = 0; j < alive[i].size(); j++) {
            if (!alive[i][j]) continue;
            ins += cnt[i][j * 4 + 0];
            miss += cnt[i][j * 4 + 1];
            evict += cnt[i][j * 4 + 2];
            wb += cnt[i][j * 4 + 3];
        }
        double miss_rate = (double)miss / (double)ins;
        o << "LEVEL" << i << "===========================================================\n";
        o << "Simulation results for " << y.cache[i].size << " Bytes " << y.cache[i].num_ways
          << "-way set associative cache model:\n";
        o << "The total # of memory instructions: " << ins << std::endl;
        o << "The # of cache-missed instructions: " << miss << std::endl;
        o << "The # of evicted instructions: " << evict << std::endl;
        o << "The # of writeback instructions: " << wb << std::endl;
        o << "The cache miss rate: " << 100 * miss_rate << "%" << std::endl;
        o << "=================================================================\n\n";
    }
    {
        const auto& dc = cnt[g.num_levels];
        const auto& da = alive[g.num_levels];
        uint64_t ins = es.lvl_cnt[PU_CNT_DIR][0], miss = es.lvl_cnt[PU_CNT_DIR][1], evict = es.lvl_cnt[PU_CNT_DIR][2];
        for (size_t j = 0; j < da.size(); j++) {
            if (!da[j]) continue;
            ins += dc[j * 4 + 0];
            miss += dc[j * 4 + 1];
            evict += dc[j * 4 + 2];
        }
        double miss_rate = (double)miss / (double)ins;
        o << "Directory Cache" << "===========================================================\n";
        o << "Simulation results for " << y.directory_cache.size << " Bytes " << y.directory_cache.num_ways
          << "-way set associative cache model:\n";
        o << "The total # of memory instructions: " << ins << std::endl;
        o << "The # of cache-missed instructions: " << miss << std::endl;
        o << "The # of replaced instructions: " << evict << std::endl;
        o << "The cache miss rate: " << 100 * miss_rate << "%" << std::endl;
        o << "=================================================================\n\n";
    }
    if (y.verbose_report) {
        o << "Statistics for each cache with non-zero accesses: \n\n";
        for (int i = 0; i < g.num_levels; i++) {
            o << "LEVEL" << i << "*****************************************************\n\n";
            for (size_t j = 0; j < alive[i].size(); j++) {
                if (alive[i][j] && cnt[i][j * 4] > 0) {
                    o << "The " << j << "th cache:\n";
                    cache_report(o, y.cache[i].size, y.cache[i].num_ways, &cnt[i][j * 4]);
                }
            }
            o << "************************************************************\n\n";
        }
        o << "****************************************************" << std::endl;
        o << "Statistics for each directory caches with non-zero accesses" << std::endl;
        const auto& dc = cnt[g.num_levels];
        const auto& da = alive[g.num_levels];
        for (size_t j = 0; j < da.size(); j++) {
            if (da[j] && dc[j * 4] > 0) {
                o << "Report for directory cache " << j << std::endl;
                cache_report(o, y.directory_cache.size, y.directory_cache.num_ways, &dc[j * 4]);
            }
        }
        if (g.tlb_enable) {
            o << "****************************************************" << std::endl;
            o << "Statistics for each TLB cache with non-zero accesses" << std::endl;
            const auto& tc = cnt[g.num_levels + 1];
            for (int j = 0; j < g.num_cores; j++) {
                if (tc[(size_t)j * 4] > 0) {
                    o << "Report for tlb cache " << j << std::endl;
                    cache_report(o, y.tlb_cache.size, y.tlb_cache.num_ways, &tc[(size_t)j * 4]);
                }
            }
        }
    }
    std::string s = o.str();
    if (buf && cap) {
        size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (long)s.size();
}

}  // extern "C"
