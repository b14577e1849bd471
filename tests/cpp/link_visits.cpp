// link_visits.cpp — the per-link oracle of the end-of-run results: the CPU
// restatement (oracle/cpu_ref.cpp) built with its CPUREF_TRACE hook, which here
// counts the visits of every link and the flits sent over it.  hop() adds a
// packet's length to the run's link_flits before it calls the hook, so the
// difference of that counter between two hook calls is the packet of the hop.
// tests/link_oracle.py builds this file as a shared library of its own and
// drives it through the cpuref_* entries plus the three below.
#define CPUREF_TRACE 1
#include "../../oracle/cpu_ref.cpp"

static Sys* g_sys = nullptr;        // the system whose run is traced
static uint64_t g_flits_seen = 0;   // its link_flits at the last hook call
static std::vector<uint64_t> g_visits, g_flits;

void cpuref_trace_link(size_t link, bool, size_t) {
    if (!g_sys) return;
    if (link >= g_visits.size()) {
        g_visits.resize(link + 1, 0);
        g_flits.resize(link + 1, 0);
    }
    g_visits[link]++;
    g_flits[link] += g_sys->st.link_flits - g_flits_seen;
    g_flits_seen = g_sys->st.link_flits;
}

extern "C" {

// Start counting the runs of system h (one system at a time).
void linkvisits_begin(void* h) {
    g_sys = (Sys*)h;
    g_flits_seen = g_sys ? g_sys->st.link_flits : 0;
    g_visits.assign(g_sys ? g_sys->links.size() : 0, 0);
    g_flits.assign(g_visits.size(), 0);
}

// Links in the restatement's numbering (Sys::link_index).
size_t linkvisits_count(void) { return g_visits.size(); }

// Visits and flits of links [0, n).
int linkvisits_read(uint64_t* visits, uint64_t* flits, size_t n) {
    if (n > g_visits.size()) return -1;
    for (size_t i = 0; i < n; i++) {
        visits[i] = g_visits[i];
        flits[i] = g_flits[i];
    }
    return 0;
}

int linkvisits_width(void* h) { return h ? ((Sys*)h)->w : 0; }

}  // extern "C"
