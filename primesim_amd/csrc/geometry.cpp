// geometry.cpp — from a configuration to its Geo (geometry.h): the validation
// of a pu_sim_cfg and the layout of a replica (pu::config_geometry, what
// pu_create builds its handle on), that Geo as source text
// (pu_config_geo_source) and the engine's queue numbering inverted
// (pu_config_queue_ends).  Plain host C++: nothing here includes HIP or needs a
// device, so all of it runs under the host's sanitizers
// (tests/cpp/geometry_check.cpp).

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "geo_emit.h"

namespace {

int ilog2(uint64_t x) { return (int)std::log2((double)x); }

}  // namespace

// Validates the configuration (every condition under which the reference
// is undefined or this engine does not implement the branch) and computes the
// replica layout.
int pu::config_geometry(const pu_sim_cfg* c, Geo* g, uint64_t pool_cap) {
    std::memset(g, 0, sizeof(*g));
    const pu_sys_cfg& y = c->sys;
    if (y.num_levels < 1 || y.num_levels > PU_MAX_LEVELS) return pu::set_error(PU_EINVAL, "num_levels must be 1..4");
    if (y.num_cores < 1) return pu::set_error(PU_EINVAL, "num_cores must be >= 1");
    if (y.sys_type != 0 && y.sys_type != 1) return pu::set_error(PU_EINVAL, "sys_type must be 0 (directory) or 1 (bus)");
    const bool bus_sys = y.sys_type == 1;
    g->num_cores = y.num_cores;
    g->num_levels = y.num_levels;
    g->sys_type = y.sys_type;
    g->protocol_type = y.protocol_type;
    g->max_num_sharers = y.max_num_sharers;
    g->shared_llc = y.shared_llc;
    g->tlb_enable = y.tlb_enable;
    g->dram_access_time = y.dram_access_time;
    g->bus_latency = y.bus_latency;
    g->cnt_sum = y.verbose_report ? 0 : 1;   // per-level sums suffice unless the report lists every cache
    Layout lay;
    int nbus = 0;
    for (int l = 0; l < y.num_levels; l++) {
        const pu_cache_cfg& cc = y.cache[l];
        LevelGeo& L = g->lv[l];
        if (cc.share < 1 || cc.block_size < 1 || cc.num_ways < 1) return pu::set_error(PU_EINVAL, "bad cache geometry");
        if (cc.num_ways > PU_MAX_WAYS_WIDE) return pu::set_error(PU_ENOTSUP, "at most 4096 ways per set");
        L.nsets = cc.size / (cc.block_size * cc.num_ways);
        if (L.nsets < 1) return pu::set_error(PU_EINVAL, "cache has no sets");
        L.nways = cc.num_ways;
        L.block = cc.block_size;
        L.offbits = ilog2(cc.block_size);
        L.idxbits = ilog2(L.nsets);
        if (L.offbits + L.idxbits >= 64) return pu::set_error(PU_EINVAL, "cache geometry exceeds 64-bit addresses");
        L.access_time = cc.access_time;
        L.share = cc.share;
        L.ncaches = (int)std::ceil((double)y.num_cores / cc.share);
        L.nchildren = l == 0 ? 0 : cc.share / y.cache[l - 1].share;
        L.has_bus = cc.share > 1 ? 1 : 0;
        if (l > 0 && cc.share % y.cache[l - 1].share != 0) return pu::set_error(PU_EINVAL, "cache shares must nest");
        if (l > 0 && g->lv[l - 1].ncaches % L.nchildren != 0)
            return pu::set_error(PU_ENOTSUP, "a shared level's children must fill every parent (num_caches is a ceil, "
                                             "system.cpp:76; init_caches gives the last parent all share ratio "
                                             "children, system.cpp:184-188)");
        if (L.has_bus) {
            if (y.bus_latency < 1) return pu::set_error(PU_EINVAL, "bus_latency must be >= 1 for shared levels");
            L.bus_q0 = nbus;   // fixed up below (after the link count is known)
            nbus += L.ncaches;
        }
    }
    if (y.cache[0].share != 1)
        return pu::set_error(PU_ENOTSUP, "L1 share must be 1 (System::access passes cache[0][core_id], system.cpp:161)");
    const int N = g->lv[y.num_levels - 1].ncaches;
    g->N = N;
    const pu_cache_cfg& dc = y.directory_cache;
    if (dc.size == 0) return pu::set_error(PU_EINVAL, "a directory is required (system.cpp:1052)");
    if (dc.num_ways < 1 || dc.block_size < 1) return pu::set_error(PU_EINVAL, "bad directory geometry");
    if (dc.num_ways > PU_MAX_WAYS_WIDE) return pu::set_error(PU_ENOTSUP, "at most 4096 directory ways");
    DirGeo& D = g->dir;
    D.nsets = dc.size / (dc.block_size * dc.num_ways);
    if (D.nsets < 1) return pu::set_error(PU_EINVAL, "directory has no sets");
    D.nways = dc.num_ways;
    D.block = dc.block_size;
    D.offbits = ilog2(dc.block_size);
    D.idxbits = ilog2(D.nsets);
    D.access_time = dc.access_time;
    D.nwords = (N + 63) / 64;
    if (D.nwords > PU_MAX_NWORDS) return pu::set_error(PU_ENOTSUP, "at most 65536 LLC nodes");
    D.sh_wide = N > 4096 ? 1 : 0;         // inline sharer ids: 4 x 12 bits, or 3 x 16 bits
    D.sh_cap = D.sh_wide ? 3 : PU_SH_INLINE;
    if (y.protocol_type == 1 && N != y.num_cores)
        return pu::set_error(PU_EINVAL, "limited-pointer broadcast needs one LLC per core (system.cpp:623)");
    if (!bus_sys && y.network.link_delay < 1) return pu::set_error(PU_EINVAL, "link_delay must be >= 1");
    if (y.network.data_width < 1) return pu::set_error(PU_EINVAL, "data_width must be >= 1");
    if (y.network.header_flits < 1)
        return pu::set_error(PU_ENOTSUP, "header_flits must be >= 1 (a zero-flit packet, network.cpp:104: touching "
                                         "intervals make the tree search depend on the tree's shape, "
                                         "queue_model_history_tree.cpp:66; a zero service rate, "
                                         "queue_model_m_g_1.cpp:28-35)");
    if (y.network.router_delay >= (1ull << 31) || y.network.link_delay >= (1ull << 31) ||
        y.network.inject_delay >= (1ull << 31))
        return pu::set_error(PU_ENOTSUP, "router/link/inject delays must be < 2^31 cycles");
    g->home_offbits = ilog2(dc.block_size);
    g->home_mask_bits = (int)std::ceil(std::log2((double)N));
    {
        // Reachable directory sets (DirGeo): with a = addr >> offbits, the raw
        // home is a mod 2^hb (folded to raw mod 2^(hb-1) when >= N) and the set
        // is a mod nsets, so a home only sees sets congruent to it modulo
        // G = gcd(nsets, 2^hb), or 2^(hb-1) when folding can occur.
        int lg = 0;
        const int hb = g->home_mask_bits;
        if (D.offbits == g->home_offbits && hb > 0) {
            int v2 = 0;
            while (v2 < 63 && ((D.nsets >> v2) & 1) == 0) v2++;
            lg = std::min(v2, hb);
            if ((uint64_t)N < (1ull << hb)) lg = std::min(lg, hb - 1);
        }
        D.cset_shift = lg;
        D.csets = D.nsets >> lg;
    }
    g->net_type = y.network.net_type;
    g->net_width = g->net_type == 1 ? (int)std::ceil(std::cbrt((double)N)) : (int)std::ceil(std::sqrt((double)N));
    g->header_flits = y.network.header_flits;
    g->data_width = y.network.data_width;
    g->router_delay = y.network.router_delay;
    g->link_delay = y.network.link_delay;
    g->inject_delay = y.network.inject_delay;
    const int w = g->net_width;
    pu_set_net_magic(w, g->header_flits, g->data_width, (int)g->lv[y.num_levels - 1].block, &g->w_magic,
                     &g->w2_magic, &g->w2, &g->blk_len, &g->plen_blk);
    // the bus system never transmits (mesi_bus has no network), so it keeps no link queues
    g->nlinks = bus_sys ? 0 : (w > 1 ? (w - 1) * w * (g->net_type == 1 ? 3 * w : 2) : 0);
    g->nqueues = g->nlinks + nbus;
    if (y.tlb_enable) {
        const pu_cache_cfg& tc = y.tlb_cache;
        TlbGeo& T = g->tlb;
        if (tc.size == 0 || tc.num_ways < 1 || tc.block_size < 1) return pu::set_error(PU_EINVAL, "tlb_enable needs a TLB");
        if (tc.num_ways > PU_MAX_WAYS_WIDE) return pu::set_error(PU_ENOTSUP, "at most 4096 TLB ways");
        if (y.page_size < 1) return pu::set_error(PU_EINVAL, "page_size must be >= 1");
        T.nsets = tc.size / (tc.block_size * tc.num_ways);
        if (T.nsets < 1) return pu::set_error(PU_EINVAL, "TLB has no sets");
        T.nways = tc.num_ways;
        T.page_size = (uint64_t)y.page_size;
        T.offbits = ilog2((uint64_t)y.page_size);     // Cache::init for TLB_CACHE (cache.cpp:66-69)
        T.idxbits = ilog2(T.nsets);
        T.access_time = tc.access_time;
        T.page_miss_delay = y.page_miss_delay;
        uint64_t cap = 1ull << 22;     // 3.1 M distinct pages (12 GiB at 4 KB) before PU_ERRF_PAGES
        if (const char* e = std::getenv("PRIMEUNCORE_PAGE_ENTRIES")) cap = std::strtoull(e, nullptr, 10);
        uint64_t p2 = 64;
        while (p2 < cap && p2 < (1ull << 32)) p2 <<= 1;
        T.pages_cap = p2;
    }
    for (int l = 0; l < y.num_levels; l++)
        if (g->lv[l].has_bus) g->lv[l].bus_q0 += g->nlinks;
    const pu_dram_cfg& dm = y.dram;   // opt-in bank model (pu_dram_cfg); 0 banks = the reference's Dram
    if (dm.banks < 0 || dm.banks > (1 << 20) || (dm.banks & (dm.banks - 1)) != 0)
        return pu::set_error(PU_EINVAL, "dram banks must be 0 or a power of two <= 2^20");
    if (dm.banks > 0) {
        if (dm.row_bytes < 64 || (dm.row_bytes & (dm.row_bytes - 1)) != 0 || dm.row_bytes > (1ull << 40))
            return pu::set_error(PU_EINVAL, "dram row_bytes must be a power of two in [64, 2^40]");
        if (dm.t_rcd < 0 || dm.t_rp < 0 || dm.t_burst < 0 || dm.t_rcd >= (1 << 24) || dm.t_rp >= (1 << 24) ||
            dm.t_burst >= (1 << 24))
            return pu::set_error(PU_EINVAL, "dram timings must be in [0, 2^24) cycles");
        g->dram_banks = dm.banks;
        g->dram_bank_shift = ilog2((uint64_t)dm.banks);
        g->dram_row_shift = ilog2(dm.row_bytes);
        g->dram_t_rcd = dm.t_rcd;
        g->dram_t_rp = dm.t_rp;
        g->dram_t_burst = dm.t_burst;
    }

    // ---- layout
    for (int l = 0; l < y.num_levels; l++) {
        LevelGeo& L = g->lv[l];
        uint64_t lines = (uint64_t)L.ncaches * L.nsets * L.nways;
        if (lines >= (1ull << 32)) return pu::set_error(PU_ENOTSUP, "at most 2^32 lines per cache level");
        L.off_meta = lay.take(lines * sizeof(LineMeta));
        L.off_ts = lay.take(lines * sizeof(int64_t));
        L.off_alive = lay.take((uint64_t)L.ncaches * 4);
        L.off_cnt = lay.take((uint64_t)L.ncaches * 32);
    }
    // the bus system has no directory lines (its report still prints the
    // directory block, from counters that stay 0)
    uint64_t dlines = bus_sys ? 0 : (uint64_t)N * D.csets * D.nways;
    if (dlines >= (1ull << 32)) return pu::set_error(PU_ENOTSUP, "at most 2^32 directory lines");
    D.off_line = lay.take(dlines * sizeof(DirLine));
    D.off_prog = lay.take(dlines * sizeof(int32_t));
    // sharer sets of more than 4 LLCs live in pool bitmaps: one entry per
    // directory line (a line holds at most one, so the pool cannot run out)
    // unless that exceeds 2 GiB of bitmaps; then as many as fit, and running
    // out stops the replica with PU_ERRF_POOL rather than diverge.
    // PRIMEUNCORE_POOL_ENTRIES overrides (tests)
    uint64_t pool = 0;
    if (!bus_sys) {
        const uint64_t cap = (2ull << 30) / ((uint64_t)D.nwords * 8);
        pool = std::max<uint64_t>(std::min(dlines, cap), 64);
    }
    if (pool_cap && !bus_sys) pool = std::max<uint64_t>(std::min(pool, pool_cap), 64);
    if (const char* e = std::getenv("PRIMEUNCORE_POOL_ENTRIES"); e && !bus_sys) pool = std::strtoull(e, nullptr, 10);
    if (pool > (1ull << 30)) pool = 1ull << 30;
    D.pool_entries = (int32_t)pool;
    D.off_pool = lay.take(pool * (uint64_t)D.nwords * 8);
    D.off_pool_free = lay.take(pool * 4);
    D.off_alive = lay.take((uint64_t)N * 4);
    D.off_cnt = lay.take((uint64_t)N * 32);
    if (y.tlb_enable) {
        TlbGeo& T = g->tlb;
        const uint64_t tl = (uint64_t)y.num_cores * T.nsets * T.nways;
        if (tl >= (1ull << 32)) return pu::set_error(PU_ENOTSUP, "at most 2^32 TLB entries");
        T.off_meta = lay.take(tl * sizeof(LineMeta));
        T.off_ts = lay.take(tl * sizeof(int64_t));
        T.off_ppage = lay.take(tl * sizeof(uint64_t));
        T.off_cnt = lay.take((uint64_t)y.num_cores * 32);
        T.off_pages = lay.take(T.pages_cap * sizeof(PageEnt));
    }
    g->off_qhdr = lay.take((uint64_t)g->nqueues * PU_HDR_BYTES);
    g->off_qring = lay.take((uint64_t)g->nqueues * PU_QRING * sizeof(QueueSlot));
    g->off_stats = lay.take(sizeof(EngineStats));
    g->off_completion = lay.take((uint64_t)y.num_cores * 8);
    g->off_run = lay.take(sizeof(RunState));
    g->off_core_shift = lay.take((uint64_t)y.num_cores * 8);
    g->off_dram = lay.take((uint64_t)g->dram_banks * sizeof(DramBank));
    g->replica_bytes = align_up(lay.cur, 4096);
    return 0;
}

extern "C" {

long pu_config_geo_source(const pu_sim_cfg* cfg, char* buf, size_t cap) {
    if (!cfg) return pu::set_error(PU_EINVAL, "bad arguments");
    Geo geo;
    if (pu::config_geometry(cfg, &geo) != 0) return PU_EINVAL;
    const std::string s = pu::geo_cxx(geo);
    if (buf && cap) {
        const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (long)s.size();
}

// The engine's record numbering (engine.hip net_route_link), inverted.
int pu_config_queue_ends(const pu_sim_cfg* cfg, int q, int* kind, int* a, int* b) {
    if (!cfg || !kind || !a || !b) return pu::set_error(PU_EINVAL, "pu_config_queue_ends: bad arguments");
    Geo g;
    int rc = pu::config_geometry(cfg, &g);
    if (rc) return rc;
    *kind = *a = *b = -1;
    if (q < 0 || q >= g.nqueues) return 0;
    if (q >= g.nlinks) {
        for (int l = 0; l < g.num_levels; l++) {
            const LevelGeo& L = g.lv[l];
            if (L.has_bus && q >= L.bus_q0 && q < L.bus_q0 + L.ncaches) {
                *kind = 3;
                *a = l;
                *b = q - L.bus_q0;
            }
        }
        return 0;
    }
    const int w = g.net_width, w1 = w - 1;   // nlinks > 0, so w > 1
    const int row = q / w1, low = q % w1;    // the record's row of w - 1 edges; the lower coordinate along it
    if (g.net_type != 1) {
        if (row < w) {          // x: row = y
            *kind = 0;
            *a = row * w + low;
            *b = *a + 1;
        } else {                // y: row = w + x
            *kind = 1;
            *a = low * w + (row - w);
            *b = *a + w;
        }
        return 0;
    }
    const int w2 = w * w, blk = row / w2, rr = row % w2, hi = rr / w, lo = rr % w;
    if (blk == 0) {             // x: row = z*w + y
        *kind = 0;
        *a = hi * w2 + lo * w + low;
        *b = *a + 1;
    } else if (blk == 1) {      // y: row = z*w + x
        *kind = 1;
        *a = hi * w2 + low * w + lo;
        *b = *a + w;
    } else {                    // z: row = y*w + x
        *kind = 2;
        *a = low * w2 + hi * w + lo;
        *b = *a + w2;
    }
    return 0;
}

}  // extern "C"
