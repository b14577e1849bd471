// geometry_check.cpp — the HIP-free part of the library's host side
// (primesim_amd/csrc/common.cpp, config.cpp, geometry.cpp) as one stand-alone
// program: three of the project's golden configurations (a directory system on a
// 3D mesh, a bus system, one with the TLB), compiled in as text, go through
// pu_config_parse_xml, pu::config_geometry and pu::geo_cxx; then
// pu_config_queue_ends is asked about every q in [-1, nqueues] and the ends must
// round-trip (a link's b - a is 1, w or w * w by its kind; a bus id lies in its
// level's range).  Configurations the validation refuses must fail with their
// texts: no levels, too many ways, zero-flit packets, and a shared level whose
// children do not fill its last parent (next to ones that do, which pass).
// Host only (tests/test_config.py builds it with the host's address and
// undefined-behaviour sanitizers).
#include <cstdio>
#include <cstring>
#include <string>

#include "../../primesim_amd/csrc/common.cpp"
#include "../../primesim_amd/csrc/config.cpp"
#include "../../primesim_amd/csrc/geometry.cpp"

// tests/golden/mesh3d.xml
static const char k_mesh3d[] = R"xml(<?xml version = "1.0" encoding = "utf-8" standalone = "yes"?>

<simulator>
    <max_msg_size>100</max_msg_size>
    <thread_sync_interval>1000</thread_sync_interval>
    <proc_sync_interval>10000</proc_sync_interval>
    <syscall_cost>10000</syscall_cost>
    <num_recv_threads>1</num_recv_threads>
    <system>
       <dram_access_time>120</dram_access_time>
       <num_levels>1</num_levels>
       <cpi_nonmem>1</cpi_nonmem>
       <num_cores>64</num_cores>
       <sys_type>0</sys_type>
       <protocol_type>0</protocol_type>
       <max_num_sharers>6</max_num_sharers>
       <page_size>4096</page_size>
       <tlb_enable>0</tlb_enable>
       <shared_llc>1</shared_llc>
       <verbose_report>0</verbose_report>
       <freq>2.5</freq>
       <bus_latency>2</bus_latency>
       <page_miss_delay>200</page_miss_delay>
       <network>
          <net_type>1</net_type>
          <data_width>10</data_width>
          <header_flits>3</header_flits>
          <router_delay>0</router_delay>
          <link_delay>1</link_delay>
          <inject_delay>1</inject_delay>
       </network>
       <cache>
          <level>0</level>
          <share>1</share>
          <access_time>1</access_time>
          <size>32768</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </cache>
       <directory_cache>
          <level>0</level>
          <share>1</share>
          <access_time>10</access_time>
          <size>262144</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </directory_cache>
       <tlb_cache>
          <level>0</level>
          <share>1</share>
          <access_time>0</access_time>
          <size>64</size>
          <block_size>1</block_size>
          <num_ways>64</num_ways>
       </tlb_cache>
    </system>
</simulator>
)xml";

// tests/golden/bus_l2_shared.xml
static const char k_bus_l2_shared[] = R"xml(<?xml version = "1.0" encoding = "utf-8" standalone = "yes"?>

<simulator>
    <max_msg_size>100</max_msg_size>
    <thread_sync_interval>1000</thread_sync_interval>
    <proc_sync_interval>10000</proc_sync_interval>
    <syscall_cost>10000</syscall_cost>
    <num_recv_threads>1</num_recv_threads>
    <system>
       <dram_access_time>120</dram_access_time>
       <num_levels>2</num_levels>
       <cpi_nonmem>1</cpi_nonmem>
       <num_cores>64</num_cores>
       <sys_type>1</sys_type>
       <protocol_type>0</protocol_type>
       <max_num_sharers>6</max_num_sharers>
       <page_size>4096</page_size>
       <tlb_enable>0</tlb_enable>
       <shared_llc>1</shared_llc>
       <verbose_report>0</verbose_report>
       <freq>2.5</freq>
       <bus_latency>3</bus_latency>
       <page_miss_delay>200</page_miss_delay>
       <network>
          <net_type>0</net_type>
          <data_width>10</data_width>
          <header_flits>3</header_flits>
          <router_delay>0</router_delay>
          <link_delay>1</link_delay>
          <inject_delay>1</inject_delay>
       </network>
       <cache>
          <level>0</level>
          <share>1</share>
          <access_time>1</access_time>
          <size>8192</size>
          <block_size>64</block_size>
          <num_ways>4</num_ways>
       </cache>
       <cache>
          <level>1</level>
          <share>4</share>
          <access_time>6</access_time>
          <size>65536</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </cache>
       <directory_cache>
          <level>0</level>
          <share>1</share>
          <access_time>10</access_time>
          <size>262144</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </directory_cache>
       <tlb_cache>
          <level>0</level>
          <share>1</share>
          <access_time>0</access_time>
          <size>64</size>
          <block_size>1</block_size>
          <num_ways>64</num_ways>
       </tlb_cache>
    </system>
</simulator>
)xml";

// tests/golden/tlb_c1.xml
static const char k_tlb_c1[] = R"xml(<?xml version = "1.0" encoding = "utf-8" standalone = "yes"?>

<simulator>
    <max_msg_size>100</max_msg_size>
    <thread_sync_interval>1000</thread_sync_interval>
    <proc_sync_interval>10000</proc_sync_interval>
    <syscall_cost>10000</syscall_cost>
    <num_recv_threads>1</num_recv_threads>
    <system>
       <dram_access_time>120</dram_access_time>
       <num_levels>1</num_levels>
       <cpi_nonmem>1</cpi_nonmem>
       <num_cores>16</num_cores>
       <sys_type>0</sys_type>
       <protocol_type>0</protocol_type>
       <max_num_sharers>6</max_num_sharers>
       <page_size>4096</page_size>
       <tlb_enable>1</tlb_enable>
       <shared_llc>1</shared_llc>
       <verbose_report>0</verbose_report>
       <freq>2.5</freq>
       <bus_latency>2</bus_latency>
       <page_miss_delay>200</page_miss_delay>
       <network>
          <net_type>0</net_type>
          <data_width>10</data_width>
          <header_flits>3</header_flits>
          <router_delay>0</router_delay>
          <link_delay>1</link_delay>
          <inject_delay>1</inject_delay>
       </network>
       <cache>
          <level>0</level>
          <share>1</share>
          <access_time>1</access_time>
          <size>32768</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </cache>
       <directory_cache>
          <level>0</level>
          <share>1</share>
          <access_time>10</access_time>
          <size>262144</size>
          <block_size>64</block_size>
          <num_ways>8</num_ways>
       </directory_cache>
       <tlb_cache>
          <level>0</level>
          <share>1</share>
          <access_time>0</access_time>
          <size>64</size>
          <block_size>1</block_size>
          <num_ways>64</num_ways>
       </tlb_cache>
    </system>
</simulator>
)xml";

static bool fail(const char* name, const std::string& what) {
    std::printf("FAIL %s: %s\n", name, what.c_str());
    return false;
}

// The queues of one configuration; adds their number to *total.
static bool check(const char* name, const char* xml, bool bus_sys, bool three_d, bool tlb, long* total) {
    pu_sim_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    if (pu_config_parse_xml(xml, std::strlen(xml), &cfg) != 0) return fail(name, std::string("parse: ") + pu_last_error());
    Geo g;
    if (pu::config_geometry(&cfg, &g) != 0) return fail(name, std::string("geometry: ") + pu_last_error());
    if ((g.sys_type == 1) != bus_sys || (g.net_type == 1) != three_d || (g.tlb_enable != 0) != tlb)
        return fail(name, "not the kind of system it was picked for");
    if (bus_sys ? g.nlinks != 0 : g.nlinks <= 0) return fail(name, "link count");
    if (tlb && (g.tlb.pages_cap == 0 || g.tlb.off_pages == 0)) return fail(name, "no page table");
    const std::string src = pu::geo_cxx(g);
    if (src.find("#define PU_JIT_NL " + std::to_string(g.num_levels) + "\n") != 0 ||
        src.find(".replica_bytes = " + std::to_string(g.replica_bytes) + "ULL") == std::string::npos)
        return fail(name, "geo_cxx");
    char small[16];
    if (pu_config_geo_source(&cfg, small, sizeof small) != (long)src.size() || std::strlen(small) != sizeof small - 1 ||
        std::memcmp(small, src.data(), sizeof small - 1) != 0)
        return fail(name, "pu_config_geo_source into a short buffer");

    const int w = g.net_width, nodes = three_d ? w * w * w : w * w;
    int buses = 0;
    for (int q = -1; q <= g.nqueues; q++) {
        int kind = 7, a = 7, b = 7;
        if (pu_config_queue_ends(&cfg, q, &kind, &a, &b) != 0) return fail(name, std::string("queue_ends: ") + pu_last_error());
        const std::string at = "queue " + std::to_string(q);
        if (q < 0 || q >= g.nqueues) {
            if (kind != -1 || a != -1 || b != -1) return fail(name, at + " is no queue");
        } else if (q < g.nlinks) {
            const int step = kind == 0 ? 1 : kind == 1 ? w : kind == 2 && three_d ? w * w : 0;
            if (step == 0 || a < 0 || b >= nodes || b - a != step) return fail(name, at + ": not a mesh edge");
        } else {
            if (kind != 3 || a < 0 || a >= g.num_levels) return fail(name, at + ": not a bus");
            const LevelGeo& L = g.lv[a];
            if (!L.has_bus || b < 0 || b >= L.ncaches || q != L.bus_q0 + b) return fail(name, at + ": outside its level's range");
            buses++;
        }
    }
    int want_buses = 0;
    for (int l = 0; l < g.num_levels; l++) want_buses += g.lv[l].has_bus ? g.lv[l].ncaches : 0;
    if (buses != want_buses || g.nlinks + buses != g.nqueues) return fail(name, "bus count");
    *total += g.nqueues;
    return true;
}

// A configuration the validation refuses: the code and the text.
static bool refused(const char* name, const pu_sim_cfg& cfg, int code, const char* text) {
    Geo g;
    const int rc = pu::config_geometry(&cfg, &g);
    if (rc != code || std::strcmp(pu_last_error(), text) != 0)
        return fail(name, "returned " + std::to_string(rc) + " \"" + pu_last_error() + "\"");
    int kind, a, b;
    if (pu_config_queue_ends(&cfg, 0, &kind, &a, &b) != code || pu_config_geo_source(&cfg, nullptr, 0) != PU_EINVAL)
        return fail(name, "the entries built on it do not fail");
    return true;
}

int main() {
    long total = 0;
    if (!check("mesh3d", k_mesh3d, false, true, false, &total)) return 1;
    if (!check("bus_l2_shared", k_bus_l2_shared, true, false, false, &total)) return 1;
    if (!check("tlb_c1", k_tlb_c1, false, false, true, &total)) return 1;

    pu_sim_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    if (pu_config_parse_xml(k_mesh3d, sizeof k_mesh3d - 1, &cfg) != 0) return 1;
    pu_sim_cfg bad = cfg;
    bad.sys.num_levels = 0;
    if (!refused("num_levels 0", bad, PU_EINVAL, "num_levels must be 1..4")) return 1;
    bad = cfg;
    bad.sys.cache[0].num_ways = 4097;
    if (!refused("4097 ways", bad, PU_ENOTSUP, "at most 4096 ways per set")) return 1;

    // zero-flit packets (network.cpp:104), whatever the system
    static const char k_flits[] =
        "header_flits must be >= 1 (a zero-flit packet, network.cpp:104: touching intervals make the tree search "
        "depend on the tree's shape, queue_model_history_tree.cpp:66; a zero service rate, "
        "queue_model_m_g_1.cpp:28-35)";
    bad = cfg;
    bad.sys.network.header_flits = 0;
    if (!refused("header_flits 0", bad, PU_ENOTSUP, k_flits)) return 1;
    bad.sys.network.header_flits = -1;
    if (!refused("header_flits -1", bad, PU_ENOTSUP, k_flits)) return 1;
    bad.sys.network.header_flits = 1;
    Geo g;
    if (pu::config_geometry(&bad, &g) != 0 || g.header_flits != 1) return !fail("header_flits 1", pu_last_error());

    // a shared level whose children do not fill its last parent (system.cpp:76, :184-188)
    static const char k_fill[] =
        "a shared level's children must fill every parent (num_caches is a ceil, system.cpp:76; init_caches gives "
        "the last parent all share ratio children, system.cpp:184-188)";
    pu_sim_cfg l2;
    std::memset(&l2, 0, sizeof l2);
    if (pu_config_parse_xml(k_bus_l2_shared, sizeof k_bus_l2_shared - 1, &l2) != 0) return 1;
    static const struct { int cores, share; bool ok; } fills[] = {
        {9, 2, false}, {2, 8, false}, {10, 4, false}, {12, 4, true}, {64, 4, true}};
    for (const auto& f : fills)
        for (int sys_type = 0; sys_type < 2; sys_type++) {
            bad = l2;
            bad.sys.sys_type = sys_type;
            bad.sys.num_cores = f.cores;
            bad.sys.cache[1].share = f.share;
            const std::string name = std::to_string(f.cores) + " cores, share " + std::to_string(f.share);
            if (!f.ok) {
                if (!refused(name.c_str(), bad, PU_ENOTSUP, k_fill)) return 1;
            } else if (pu::config_geometry(&bad, &g) != 0 || g.lv[1].ncaches * f.share != f.cores) {
                return !fail(name.c_str(), pu_last_error());
            }
        }

    std::printf("OK %ld queues\n", total);
    return 0;
}
