// common.h — host-side helpers shared by the C-ABI translation units.
#pragma once

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/primeuncore.h"

struct Geo;   // geometry.h

namespace pu {

// Records a message for pu_last_error() and returns `code` (common.cpp).
int set_error(int code, const std::string& msg);
// The calling thread's last message.
const std::string& last_error();

// 0 when `device` is a HIP device of this machine, else PU_ENODEV with the
// error "no HIP device available", followed by " (note)" where a note is given.
int device_check(int device, const char* note = nullptr);

inline bool req_fmt_ok(int fmt) { return fmt == PU_REQ_FMT_32 || fmt == PU_REQ_FMT_16; }

// pu_run_device with extra kernel flags (PU_KF_*, geometry.h): the server's
// per-receive-thread stop.  use_replay_mode = false launches open-loop whatever
// pu_set_replay_mode left on the handle (live clients' timers are real).
int run_device_flags(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
                     uint32_t extra_flags, bool use_replay_mode = true);
// RunState.limit_at of replicas [0, n) after the last launch: the index into
// that launch's request array of the first request that raised a
// PU_ERRF_LIMITS bit (UINT64_MAX: none).
int limit_positions(pu_handle* h, uint64_t* out, size_t n);

// The geometry pu_create builds for cfg, validated (geometry.cpp): 0, or PU_E*
// with the error text.  pool_cap > 0 bounds the sharer-bitmap pool's entries.
// No device.
int config_geometry(const pu_sim_cfg* cfg, Geo* out, uint64_t pool_cap = 0);

// A replica's layout is laid down field after field, each aligned
// (geometry.cpp; the network unit hook lays down a small one of its own).
inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
struct Layout {
    uint64_t cur = 0;
    uint64_t take(uint64_t bytes, uint64_t align = 256) {
        cur = align_up(cur, align);
        uint64_t o = cur;
        cur += bytes;
        return o;
    }
};

// ThreadSched (reference src/thread_sched.cpp:55-91) with its quirks: the
// first free core is taken, a busy core is marked with its prog id, a core is
// freed only while core_stat == 1, and getCoreId inserts 0 for an unknown
// (prog, thread) through std::map::operator[].  The map's (prog, thread) order
// is the order ThreadSched::report prints.
struct Sched {
    std::vector<int> stat;
    std::map<std::pair<int, int>, int> map;
    int alloc(int prog, int th) {
        for (size_t i = 0; i < stat.size(); i++)
            if (stat[i] == 0) {
                stat[i] = prog;
                map[{prog, th}] = (int)i;
                return (int)i;
            }
        return -1;
    }
    int dealloc(int prog, int th) {
        int c = map[{prog, th}];
        if (c >= 0 && c < (int)stat.size() && stat[(size_t)c] == 1) {
            stat[(size_t)c] = 0;
            return 1;
        }
        return 0;
    }
    int get(int prog, int th) { return map[{prog, th}]; }
};

}  // namespace pu
