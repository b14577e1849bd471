// handle.h — struct pu_handle and what the translation units that work on one
// share: the engine's entry points (engine.hip), HIP_TRY, and the internal
// functions more than one file calls.  Private to the library and host code
// only: uncore.cpp, resident.cpp, report.cpp, unit_hooks.cpp and the stage
// files (run_results.hip, replica_fork.hip) include it; server.cpp and the
// HIP-free files keep to common.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "jit.h"

// engine.hip: the init kernels and the unit-test hooks (the engine kernels
// themselves are compiled per configuration, jit.h)
extern "C" int pu_engine_lds_header_queues(void);
extern "C" int pu_engine_init_pool(char* arena, uint64_t replica_bytes, uint64_t off_pool_free, uint64_t off_run,
                                   int pool_entries, int nreplicas, hipStream_t stream);
extern "C" int pu_engine_unit_queue(const Geo* d_geo, char* base, uint64_t minp, const uint64_t* t,
                                    const uint64_t* p, uint64_t n, uint64_t* out, uint64_t* mg1, hipStream_t s);
extern "C" int pu_engine_unit_mg1(const uint64_t* n, const double* sum, const double* sum_sq, const uint64_t* newest,
                                  uint64_t cnt, uint64_t* out, uint8_t* path, hipStream_t s);
extern "C" int pu_engine_unit_network(const Geo* d_geo, char* base, const int32_t* src, const int32_t* dst,
                                      const int32_t* len, const uint64_t* timer, uint64_t n, uint64_t* out,
                                      hipStream_t s);
extern "C" int pu_engine_init_queues(char* arena, uint64_t replica_bytes, uint64_t off_qhdr, uint64_t off_qring,
                                     int nqueues, int nreplicas, int wide, hipStream_t stream);

struct pu_handle {
    pu_sim_cfg cfg;
    Geo geo;
    Geo* d_geo = nullptr;
    char* arena = nullptr;
    int R = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    struct timespec sim_start{}, sim_finish{};   // UncoreManager::sim_start_time / sim_finish_time
    uint32_t replay_flags = 0;   // PU_KF_CLOSED under PU_REPLAY_CLOSED
    uint32_t dev_req_flags = 0;  // PU_KF_REQ16 under PU_REQ_FMT_16 (the device-run entry points)
    int cus = 0;                 // compute units of the device (latency-mode launches)
    bool lds_headers_ok = false; // the replica's queue headers fit one CU's LDS
    bool lds_headers_short = false;   // latency mode for short host batches too
    pu::JitKernels jit;          // the engine compiled for this configuration (jit.cpp): every launch runs it
    int last_kernel = -1;        // jit.f[s][h] of the last launch or resident command, as s * 2 + h (-1: none yet)
    // ThreadSched (thread_sched.cpp): the shared one, and per-replica copies
    // made on first use of a per-replica call (pu_*_core_replica: the server's
    // sessions); the shared calls update both
    pu::Sched sched;
    std::vector<std::unique_ptr<pu::Sched>> rsched;
    pu::Sched& sched_of(int r) { return rsched[(size_t)r] ? *rsched[(size_t)r] : sched; }
    // staging for host-buffer batches: one device block [offsets | requests]
    // filled by one copy from a pinned host twin, and pinned landing slots for
    // the delays and the replica's error flags
    pu_req* d_reqs = nullptr;
    int32_t* d_delays = nullptr;
    uint64_t* d_off = nullptr;
    uint8_t* h_in = nullptr;     // pinned: [offsets (64 B) | reqs[cap]]
    int32_t* h_delays = nullptr; // pinned: delays[cap]
    uint64_t* h_tail = nullptr;  // pinned: error flags, RunState
    size_t stage_cap = 0;
    // Resident mode (engine.hip resident_body; geometry.h PuMailbox): one
    // latency-mode workgroup serving pu_access / short host batches of one
    // replica through a mailbox in host-coherent pinned memory
    struct Resident {
        int mode = 1;               // PRIMEUNCORE_RESIDENT (0 off) / pu_set_resident
        bool running = false;       // a resident kernel was launched and not yet joined
        int replica = -1;
        uint64_t seq = 0;           // commands posted
        uint64_t acked = 0;         // commands completed
        PuMailbox* mb = nullptr;    // host address
        void* mb_dev = nullptr;     // the same memory, as the device sees it
        pu_req* stage = nullptr;    // device staging of a command's requests
        hipStream_t stream = nullptr;
        hipEvent_t after = nullptr; // orders the kernel after the handle's stream
        uint64_t idle_ticks = 5000000;   // 50 ms of s_memrealtime (100 MHz)
        uint64_t commands = 0, launches = 0;
        uint64_t phase_ticks[4] = {0, 0, 0, 0};   // summed kernel-side phases (PuResDev.phase, full answers)
        uint64_t err = 0;                         // the replica's error flags as of the last full answer
        uint64_t fast = 0;                        // commands answered by the fast word
        uint64_t call_ns = 0;                     // summed host-side post-to-ack time
    } res;
    std::mutex mu;
};

#define HIP_TRY(expr, code)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return pu::set_error(code, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace pu {

// ---- resident.cpp.  Unless said otherwise the caller holds h->mu.
// Joins the handle's resident kernel, if one runs: a STOP command unless it
// already left (idle), then a wait for its stream.  The replica's queue headers
// are in device memory afterwards.
int resident_stop(pu_handle* h);
// The same for callers that do not hold h->mu: takes it.
int resident_quiesce(pu_handle* h);
// A batch of n requests may go through the resident kernel.
bool resident_eligible(const pu_handle* h, size_t n);
// One command: the requests through the resident kernel of `replica` (started
// or restarted here); delays, error flags and (TLB) the last translated address
// come back through the mailbox.
int resident_run(pu_handle* h, int replica, const pu_req* reqs, size_t n, uint32_t flags, int32_t* delay_out,
                 uint64_t* err_out, uint64_t* last_addr);
// Joins the kernel and releases everything resident mode allocated.
void resident_free(pu_handle* h);

// ---- report.cpp.  Neither is called with h->mu held (read_replica quiesces).
// Replica r's engine-side counters: EngineStats, and per level, the directory
// ([num_levels]) and the TLBs ([num_levels + 1]) the per-cache {ins, miss,
// evict, wb} and the alive words.
int read_replica(pu_handle* h, int r, EngineStats* es, std::vector<uint64_t> cnt[PU_MAX_LEVELS + 2],
                 std::vector<uint32_t> alive[PU_MAX_LEVELS + 2]);
// The page table of replica r (empty unless tlb_enable).
int read_pages(pu_handle* h, int r, std::vector<PageEnt>* out);

// ---- uncore.cpp
// Gathers EngineStats.error_flags of replicas [0, n) (one strided copy).  The caller holds h->mu.
int gather_error_flags(pu_handle* h, uint64_t* out, size_t n);
// PU_ESTATE with a message when `flags` holds an engine-limit or undefined-
// state bit (everything but the reference's own negative-delay stop).
int limit_error(uint64_t flags, int replica);
// The thread-scheduler side of pu_replica_fork: replicas [first, first + n) but
// src get a copy of src's own scheduler, or lose theirs when src reads the
// shared one.  The caller holds h->mu and has checked the range.
void fork_sched(pu_handle* h, int src, int first, int n);

}  // namespace pu
