// uncore.cpp — the handle (handle.h) of the C ABI of include/primeuncore.h: its
// lifetime (pu_create, pu_destroy, pu_reset), the staging of host batches, the
// one launch of the HIP engine every batch path goes through (pu_access*,
// pu_run_device*, the replica pool), the thread->core map, and the small
// getters.  What else the ABI holds lives in files of its own:
//   common.cpp      the error text
//   geometry.cpp    a configuration's validation and replica layout (no HIP)
//   resident.cpp    the host side of the resident mailbox protocol
//   report.cpp      statistics and the report text
//   unit_hooks.cpp  the unit-test hooks
//
// Replaces, for the hot path only:
//   UncoreManager::init/allocCore/deallocCore/getCoreId/uncore_access
//                                   (reference src/uncore_manager.cpp:46-86)
//   System::init                    (reference src/system.cpp:47-141)
//   ThreadSched                     (reference src/thread_sched.cpp:44-118)
// There is no CPU fallback: without a HIP device pu_create fails (PU_ENODEV).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "handle.h"
#include "jit.h"

namespace pu {

int device_check(int device, const char* note) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && device >= 0 && device < ndev) return 0;
    return set_error(PU_ENODEV, std::string("no HIP device available") + (note ? " (" + std::string(note) + ")" : ""));
}

}  // namespace pu

namespace {

// The device's target name ("gfx950" from "gfx950:sramecc+:xnack-").
std::string device_target(int device) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return "";
    const std::string a = p.gcnArchName;
    return a.substr(0, a.find(':'));
}
// gfx950 hands LDS to workgroups in 1,280-B units out of a CU's 160 KB
// (measured: tools/probe/residency.hip, profiles/r5a_residency.json — one-wave
// workgroups of 6,144 / 7,152 / 8,192 / 16,384 / 32,768 B reside 25 / 21 /
// 18 / 9 / 4 per CU, hipOccupancy says 26 / 22 / 20 / 10 / 5).  A time-sliced
// launch whose grid exceeds the resident waves takes two slices: round 4's
// six-wave kernel (7,152 B: 22 by hipOccupancy, 21 resident) ran at half rate.
// Other targets are not measured: their residency is hipOccupancy's alone.
constexpr int kLdsGranule = 1280;
int lds_limited_per_cu(int lds_bytes, int lds_per_cu, int granule) {
    if (lds_bytes <= 0 || lds_per_cu <= 0 || granule <= 0) return 1 << 30;
    const int unit = (lds_bytes + granule - 1) / granule * granule;
    return lds_per_cu / unit;
}

int reset_state(pu_handle* h) {
    HIP_TRY(hipMemsetAsync(h->arena, 0, h->geo.replica_bytes * (size_t)h->R, h->stream), PU_EIO);
    // completion cycles start at -1 ("no request yet")
    HIP_TRY(hipMemset2DAsync(h->arena + h->geo.off_completion, h->geo.replica_bytes, 0xFF,
                             (size_t)h->geo.num_cores * 8, (size_t)h->R, h->stream), PU_EIO);
    int rc = pu_engine_init_queues(h->arena, h->geo.replica_bytes, h->geo.off_qhdr, h->geo.off_qring,
                                   h->geo.nqueues, h->R, 0, h->stream);
    if (rc) return pu::set_error(rc, "queue init launch failed");
    rc = pu_engine_init_pool(h->arena, h->geo.replica_bytes, h->geo.dir.off_pool_free, h->geo.off_run,
                             h->geo.dir.pool_entries, h->R, h->stream);
    if (rc) return pu::set_error(rc, "pool init launch failed");
    HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
    return 0;
}

constexpr size_t kOffBytes = 64;   // offsets, padded so the requests start on a cache line
constexpr size_t kTailBytes = 8 + sizeof(RunState);
constexpr size_t kShortBatch = 16384;   // host batches below this skip the LDS header image

void free_stage(pu_handle* h) {
    if (h->d_off) (void)hipFree(h->d_off);   // d_reqs lives in the same block
    if (h->d_delays) (void)hipFree(h->d_delays);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_delays) (void)hipHostFree(h->h_delays);
    if (h->h_tail) (void)hipHostFree(h->h_tail);
    h->d_off = nullptr;
    h->d_reqs = nullptr;
    h->d_delays = nullptr;
    h->h_in = nullptr;
    h->h_delays = nullptr;
    h->h_tail = nullptr;
    h->stage_cap = 0;
}

int ensure_stage(pu_handle* h, size_t n) {
    if (n <= h->stage_cap && h->d_off) return 0;
    size_t cap = n < 4096 ? 4096 : n;
    int rc = pu::resident_stop(h);   // hipFree may wait for the whole device
    if (rc) return rc;
    free_stage(h);
    const size_t in_bytes = kOffBytes + cap * sizeof(pu_req);
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, in_bytes), PU_ENOMEM);
    h->d_off = (uint64_t*)p;
    h->d_reqs = (pu_req*)((uint8_t*)p + kOffBytes);
    HIP_TRY(hipMalloc(&h->d_delays, cap * sizeof(int32_t)), PU_ENOMEM);
    HIP_TRY(hipHostMalloc((void**)&h->h_in, in_bytes, hipHostMallocDefault), PU_ENOMEM);
    HIP_TRY(hipHostMalloc((void**)&h->h_delays, cap * sizeof(int32_t), hipHostMallocDefault), PU_ENOMEM);
    HIP_TRY(hipHostMalloc((void**)&h->h_tail, kTailBytes, hipHostMallocDefault), PU_ENOMEM);
    h->stage_cap = cap;
    return 0;
}

// Wait for a short synchronous launch by polling: a blocking wait lets the
// host thread sleep and it wakes well after the kernel ends (the
// per-request API pays that on every call). Long launches fall back to the
// blocking wait after a few milliseconds of polling.
int wait_stream(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return pu::set_error(PU_EIO, std::string("hipStreamQuery: ") + hipGetErrorString(e));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    HIP_TRY(hipStreamSynchronize(s), PU_EIO);
    return 0;
}

int launch(pu_handle* h, int replica0, int nblocks, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
           hipStream_t s, uint64_t* d_pos = nullptr, uint64_t budget_ticks = 0, uint32_t extra_flags = 0,
           bool short_launch = false, bool use_replay_mode = true, uint32_t* d_sched = nullptr) {
    int rrc = pu::resident_stop(h);   // a launch reads the queue headers from HBM
    if (rrc) return rrc;
    HIP_TRY(hipEventRecord(h->ev0, s), PU_EIO);
    // latency mode: with at most one replica per CU each wave keeps its queue
    // headers in the CU's LDS for the launch (engine.hip, LH). Copying the
    // image in and out costs ~17 us a launch, more than a short host batch
    // (a lone uncore_access, one MEM_REQUESTS message) wins back, so those
    // run with the headers in HBM (tools/latency_bench.py)
    // (a replica-pool launch is always a throughput launch)
    // (16-B request records: throughput kernels only, the latency helper reads pu_req)
    const int lh = h->lds_headers_ok && nblocks <= h->cus && !short_launch && !d_sched &&
                   !(extra_flags & PU_KF_REQ16) ? 1 : 0;
    const uint32_t flags = (extra_flags & PU_KF_NOHALT) || !use_replay_mode ? extra_flags
                                                                          : (h->replay_flags | extra_flags);
    int rc = pu::jit_launch(h->jit, d_pos != nullptr, lh != 0, nblocks, s, h->d_geo, h->arena, replica0, d_reqs,
                            d_off, d_delay, d_pos, budget_ticks, flags, d_sched, h->R);
    if (rc) return pu::set_error(rc, "engine launch failed");
    h->last_kernel = pu::jit_launch_kernel(d_pos != nullptr, lh != 0, d_sched != nullptr);   // what jit_launch ran
    HIP_TRY(hipEventRecord(h->ev1, s), PU_EIO);
    return 0;
}

}  // namespace

// Gathers EngineStats.error_flags of replicas [0, n) (one strided copy).
int pu::gather_error_flags(pu_handle* h, uint64_t* out, size_t n) {
    if (n == 0) return 0;
    int rrc = pu::resident_stop(h);
    if (rrc) return rrc;
    const Geo& g = h->geo;
    HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
    HIP_TRY(hipMemcpy2D(out, sizeof(uint64_t), h->arena + g.off_stats + offsetof(EngineStats, error_flags),
                        g.replica_bytes, sizeof(uint64_t), n, hipMemcpyDeviceToHost), PU_EIO);
    return 0;
}

// PU_ESTATE with a message when `flags` holds an engine-limit or undefined-
// state bit (everything but the reference's own negative-delay stop).
int pu::limit_error(uint64_t flags, int replica) {
    const uint64_t bad = flags & PU_ERRF_LIMITS;
    if (!bad) return 0;
    std::string m = "replica " + std::to_string(replica) + " stopped:";
    if (bad & PU_ERRF_POOL) m += " sharer-bitmap pool exhausted (PRIMEUNCORE_POOL_ENTRIES);";
    if (bad & PU_ERRF_PAGES) m += " page table full (PRIMEUNCORE_PAGE_ENTRIES);";
    if (bad & PU_ERRF_PROG) m += " prog_id outside the packed directory line's range;";
    if (bad & PU_ERRF_WB_MISS) m += " write-back missed at its home (reference NULL dereference, Q13);";
    if (bad & PU_ERRF_EMPTY_SHARER) m += " owner lookup on an empty sharer set;";
    if (bad & PU_ERRF_QUEUE) m += " queue-model precondition violated;";
    return pu::set_error(PU_ESTATE, m);
}

extern "C" {

#ifndef PU_SRC_HASH
#define PU_SRC_HASH "unknown"
#endif
// The source hash (tools/src_hash.py over primesim_amd/csrc and include/) the
// library was built from: tests and smoke() compare it with the checkout.
const char* pu_version(void) { return "primeuncore 0.2 (gfx950) src " PU_SRC_HASH; }

int pu_set_replay_mode(pu_handle* h, int mode) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    if (mode != PU_REPLAY_OPEN && mode != PU_REPLAY_CLOSED) return pu::set_error(PU_EINVAL, "unknown replay mode");
    std::lock_guard<std::mutex> lk(h->mu);
    h->replay_flags = mode == PU_REPLAY_CLOSED ? PU_KF_CLOSED : 0u;
    return 0;
}

int pu_error_flags(pu_handle* h, uint64_t* out, size_t n) {
    if (!h || (!out && n)) return pu::set_error(PU_EINVAL, "bad arguments");
    if (n > (size_t)h->R) return pu::set_error(PU_ERANGE, "more replicas than the handle holds");
    std::lock_guard<std::mutex> lk(h->mu);
    return pu::gather_error_flags(h, out, n);
}

int pu_config_jit_warm(const pu_sim_cfg* cfg) {
    if (!cfg) return pu::set_error(PU_EINVAL, "bad arguments");
    Geo geo;
    if (pu::config_geometry(cfg, &geo) != 0) return PU_EINVAL;
    return pu::jit_warm(geo, nullptr);
}

int pu_compiled_config(const pu_handle* h) { return h ? 2 : 0; }
int pu_compiled_compiler(const pu_handle* h) {
    if (!h) return 0;
    int off = 0;
    for (int part = 0; part < pu::kJitParts; part++) off += h->jit.cc[part] == pu::kJitOffline;
    return off == pu::kJitParts ? 2 : off == 0 ? 1 : 3;   // 3: the parts came from different compilers
}

const char* pu_last_launch_kernel(pu_handle* h) {
    if (!h) return "";
    std::lock_guard<std::mutex> lk(h->mu);
    const char* name = h->last_kernel < 0 ? nullptr : pu::jit_kernel_name(h->last_kernel >> 1, h->last_kernel & 1);
    return name ? name : "";
}

const char* pu_jit_source_tag(void) {
    static const std::string tag = pu::jit_source_tag();
    return tag.c_str();
}

int pu_jit_prof_read(unsigned long long* out, int n, int reset) {
    if (n < 0 || (n > 0 && !out)) return pu::set_error(PU_EINVAL, "bad arguments");
    return pu::jit_prof_read(out, n, reset);
}

int pu_limit_positions(pu_handle* h, uint64_t* out, size_t n) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    return pu::limit_positions(h, out, n);
}

pu_handle* pu_create(const pu_sim_cfg* cfg, int num_replicas, int device) {
    if (!cfg || num_replicas < 1) {
        pu::set_error(PU_EINVAL, "bad arguments");
        return nullptr;
    }
    Geo geo;
    if (pu::config_geometry(cfg, &geo) != 0) return nullptr;
    pu::jit_note_gpu();   // this process starts no compiler from here on
    if (pu::device_check(device, "the engine has no CPU fallback") != 0) return nullptr;
    pu_handle* h = new pu_handle();
    h->cfg = *cfg;
    h->geo = geo;
    h->R = num_replicas;
    h->device = device;
    auto fail = [&](const std::string& m) -> pu_handle* {
        pu::set_error(PU_ENOMEM, m);
        pu_destroy(h);
        return nullptr;
    };
    if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) h->cus = 0;
    {
        // "0" turns latency mode off, "2" uses it for short host batches too (A/B runs, tests)
        const char* e = std::getenv("PRIMEUNCORE_LDS_HEADERS");
        h->lds_headers_ok = geo.nqueues <= pu_engine_lds_header_queues() && !(e && e[0] == '0');
        h->lds_headers_short = e && e[0] == '2';
        // resident mode for pu_access / short host batches (on unless "0")
        const char* r = std::getenv("PRIMEUNCORE_RESIDENT");
        h->res.mode = r && r[0] == '0' ? 0 : 1;
        const char* idle = std::getenv("PRIMEUNCORE_RESIDENT_IDLE_MS");
        if (idle && std::atof(idle) > 0) h->res.idle_ticks = (uint64_t)(std::atof(idle) * 1e5);
    }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail("stream create failed");
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return fail("event create failed");
    if (hipMalloc(&h->d_geo, sizeof(Geo)) != hipSuccess) return fail("hipMalloc(geo) failed");
    {
        // The exact sharer pool (one bitmap per directory line, up to 2 GiB) is
        // usually a small share of a replica, but a config whose homes see every
        // set can make it dominate.  When the replicas asked for would not fit
        // the device with it, shrink the pool to what fits rather than fail:
        // running out then stops a replica loudly (PU_ERRF_POOL), never silently.
        size_t free_b = 0, total_b = 0;
        const uint64_t pool_b = (uint64_t)geo.dir.pool_entries * ((uint64_t)geo.dir.nwords * 8 + 4);
        if (pool_b && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            geo.replica_bytes * (uint64_t)num_replicas > (uint64_t)(free_b * 0.95)) {
            const uint64_t rest = geo.replica_bytes - pool_b;
            const uint64_t per = (uint64_t)(free_b * 0.95) / (uint64_t)num_replicas;
            if (per > rest + 64 * ((uint64_t)geo.dir.nwords * 8 + 4)) {
                const uint64_t entries = (per - rest) / ((uint64_t)geo.dir.nwords * 8 + 4);
                Geo g2;
                if (pu::config_geometry(cfg, &g2, entries) == 0 && g2.replica_bytes < geo.replica_bytes) {
                    std::fprintf(stderr,
                                 "[primeuncore] sharer-bitmap pool reduced from %d to %d entries per replica so %d "
                                 "replicas fit the device (%.1f -> %.1f MiB each); exhausting it stops a replica "
                                 "with PU_ERRF_POOL\n",
                                 geo.dir.pool_entries, g2.dir.pool_entries, num_replicas,
                                 geo.replica_bytes / 1048576.0, g2.replica_bytes / 1048576.0);
                    geo = g2;
                    h->geo = geo;
                }
            }
        }
    }
    if (hipMemcpy(h->d_geo, &geo, sizeof(Geo), hipMemcpyHostToDevice) != hipSuccess) return fail("geo upload failed");
    size_t bytes = geo.replica_bytes * (size_t)num_replicas;
    if (hipMalloc(&h->arena, bytes) != hipSuccess) {
        h->arena = nullptr;
        return fail("hipMalloc of " + std::to_string(bytes) + " bytes for the replica arena failed");
    }
    // the only engine kernels: a compile or load failure fails the handle (the compiler's log in the message)
    if (const int rc = pu::jit_load(geo, &h->jit, true); rc != 0) {
        std::string m = pu::last_error();
        pu_destroy(h);
        pu::set_error(rc, m);
        return nullptr;
    }
    h->sched.stat.assign((size_t)cfg->sys.num_cores, 0);
    h->rsched.resize((size_t)num_replicas);
    if (reset_state(h) != 0) {
        std::string m = pu::last_error();
        pu_destroy(h);
        pu::set_error(PU_EIO, m);
        return nullptr;
    }
    return h;
}

void pu_destroy(pu_handle* h) {
    if (!h) return;
    pu::resident_free(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->arena) (void)hipFree(h->arena);
    if (h->d_geo) (void)hipFree(h->d_geo);
    pu::jit_unload(&h->jit);
    free_stage(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int pu_reset(pu_handle* h) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = pu::resident_stop(h);
    if (rc) return rc;
    return reset_state(h);
}

int pu_num_replicas(const pu_handle* h) { return h ? h->R : 0; }
uint64_t pu_replica_bytes(const pu_handle* h) { return h ? h->geo.replica_bytes : 0; }
uint64_t pu_replica_pool_bytes(const pu_handle* h) {
    return h ? (uint64_t)h->geo.dir.pool_entries * ((uint64_t)h->geo.dir.nwords * 8 + 4) : 0;
}

int pu_resident_replicas(const pu_handle* h) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    int cus = 0, lds_cu = 0, per_cu = 1 << 30;
    HIP_TRY(hipSetDevice(h->device), PU_ENODEV);
    // a device that reports no per-CU LDS (0, or a per-block figure below one
    // workgroup's) keeps hipOccupancy's count rather than resolving to 0 slots
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, h->device) != hipSuccess)
        lds_cu = 0;
    const int granule = device_target(h->device) == "gfx950" ? kLdsGranule : 0;
    // both throughput launch kinds (time-sliced, replica pool: separate
    // instantiations, each its own registers and LDS), one wave per replica
    for (int mode = 1; mode <= 2; mode++) {
        int n = 0, lds = 0;
        int rc = pu::jit_occupancy(h->jit, mode, &n, &lds);
        if (rc) return pu::set_error(rc, "occupancy query failed");
        const int by_lds = lds_limited_per_cu(lds, lds_cu, granule);
        if (by_lds > 0) n = std::min(n, by_lds);
        per_cu = std::min(per_cu, n);
    }
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device), PU_EIO);
    return per_cu * cus;
}

int pu_alloc_core(pu_handle* h, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto& r : h->rsched)
        if (r) r->alloc(prog_id, thread_id);
    return h->sched.alloc(prog_id, thread_id);
}

int pu_get_core_id(pu_handle* h, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto& r : h->rsched)
        if (r) r->get(prog_id, thread_id);
    return h->sched.get(prog_id, thread_id);   // operator[]: inserts 0 like the reference
}

int pu_dealloc_core(pu_handle* h, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto& r : h->rsched)
        if (r) r->dealloc(prog_id, thread_id);
    return h->sched.dealloc(prog_id, thread_id);
}

namespace {
pu::Sched* replica_sched(pu_handle* h, int replica) {
    if (replica < 0 || replica >= h->R) return nullptr;
    auto& r = h->rsched[(size_t)replica];
    if (!r) r.reset(new pu::Sched(h->sched));
    return r.get();
}
}  // namespace

int pu_alloc_core_replica(pu_handle* h, int replica, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    pu::Sched* s = replica_sched(h, replica);
    if (!s) return pu::set_error(PU_ERANGE, "replica out of range");
    return s->alloc(prog_id, thread_id);
}

int pu_dealloc_core_replica(pu_handle* h, int replica, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    pu::Sched* s = replica_sched(h, replica);
    if (!s) return pu::set_error(PU_ERANGE, "replica out of range");
    return s->dealloc(prog_id, thread_id);
}

int pu_get_core_id_replica(pu_handle* h, int replica, int prog_id, int thread_id) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    pu::Sched* s = replica_sched(h, replica);
    if (!s) return pu::set_error(PU_ERANGE, "replica out of range");
    return s->get(prog_id, thread_id);
}

namespace {
int access_batch(pu_handle* h, int replica, const pu_req* reqs, size_t n, int32_t* delay_out, uint32_t extra,
                 uint64_t* last_addr = nullptr) {
    if (!h || (!reqs && n)) return pu::set_error(PU_EINVAL, "bad arguments");
    if (replica < 0 || replica >= h->R) return pu::set_error(PU_ERANGE, "replica out of range");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (pu::resident_eligible(h, n)) {
        // no launch: the resident kernel (headers already in its CU's LDS)
        const uint32_t flags = (extra & PU_KF_NOHALT) ? extra : (h->replay_flags | extra);
        uint64_t err = 0;
        int rrc = pu::resident_run(h, replica, reqs, n, flags, delay_out, &err, last_addr);
        if (rrc) return rrc;
        return pu::limit_error(err, replica);
    }
    int rc = ensure_stage(h, n);
    if (rc) return rc;
    // one host-to-device copy of [offsets | requests] from pinned memory
    const uint64_t off[2] = {0, (uint64_t)n};
    std::memcpy(h->h_in, off, kOffBytes);
    std::memcpy(h->h_in + kOffBytes, reqs, n * sizeof(pu_req));
    HIP_TRY(hipMemcpyAsync(h->d_off, h->h_in, kOffBytes + n * sizeof(pu_req), hipMemcpyHostToDevice, h->stream),
            PU_EIO);
    rc = launch(h, replica, 1, h->d_reqs, h->d_off, h->d_delays, h->stream, nullptr, 0, extra,
                n < kShortBatch && !h->lds_headers_short);
    if (rc) return rc;
    if (delay_out)
        HIP_TRY(hipMemcpyAsync(h->h_delays, h->d_delays, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream),
                PU_EIO);
    char* rbase = h->arena + (size_t)replica * h->geo.replica_bytes;
    HIP_TRY(hipMemcpyAsync(h->h_tail, rbase + h->geo.off_stats + offsetof(EngineStats, error_flags), 8,
                           hipMemcpyDeviceToHost, h->stream), PU_EIO);
    if (last_addr)
        HIP_TRY(hipMemcpyAsync(h->h_tail + 1, rbase + h->geo.off_run, sizeof(RunState), hipMemcpyDeviceToHost,
                               h->stream), PU_EIO);
    rc = wait_stream(h->stream);
    if (rc) return rc;
    if (delay_out) std::memcpy(delay_out, h->h_delays, n * sizeof(int32_t));
    if (last_addr) {
        RunState rs;
        std::memcpy(&rs, h->h_tail + 1, sizeof(rs));
        *last_addr = rs.last_addr;
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_ms = ms;
    // an engine limit stopped the replica where the reference would continue:
    // the delays after that request are not the reference's, say so
    return pu::limit_error(h->h_tail[0], replica);
}
}  // namespace

int pu_access_batch(pu_handle* h, int replica, const pu_req* reqs, size_t n, int32_t* delay_out) {
    return access_batch(h, replica, reqs, n, delay_out, 0);
}

int pu_access(pu_handle* h, int core_id, int prog_id, int mem_type, uint64_t* addr, int64_t timer) {
    int32_t d = 0;
    int rc = pu_access_status(h, core_id, prog_id, mem_type, addr, timer, &d);
    return rc ? rc : d;
}

int pu_access_status(pu_handle* h, int core_id, int prog_id, int mem_type, uint64_t* addr, int64_t timer,
                     int32_t* delay_out) {
    if (!h || !addr || !delay_out) return pu::set_error(PU_EINVAL, "bad arguments");
    if (core_id >= h->cfg.sys.num_cores) {              // System::access, system.cpp:147-150
        *delay_out = -1;
        return 0;
    }
    pu_req r;
    std::memset(&r, 0, sizeof(r));
    r.addr = *addr;
    r.timer = timer;
    r.core = core_id;
    r.prog_id = prog_id;
    r.mem_type = (uint8_t)mem_type;
    r.batch_start = 1;   // a lone request: running delay 0, `timer` used as given
    int32_t d = 0;
    // UncoreManager::uncore_access has no prime.cpp halt rule (PU_KF_NOHALT); a
    // closed-loop shift would move the caller's timer, so it is never applied here
    // with the TLB on, InsMem::addr_dmem comes back as the physical address (system.cpp:916)
    int rc = access_batch(h, 0, &r, 1, &d, PU_KF_NOHALT, h->geo.tlb_enable ? addr : nullptr);
    if (rc) return rc;
    *delay_out = d;
    return 0;
}

int pu_run_device(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay, void* hip_stream) {
    if (!h || !d_reqs || !d_off || !d_delay) return pu::set_error(PU_EINVAL, "bad arguments");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    std::lock_guard<std::mutex> lk(h->mu);
    return launch(h, 0, h->R, d_reqs, d_off, d_delay, s, nullptr, 0, h->dev_req_flags);
}

int pu_set_device_req_format(pu_handle* h, int fmt) {
    if (!h || !pu::req_fmt_ok(fmt)) return pu::set_error(PU_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    h->dev_req_flags = fmt == PU_REQ_FMT_16 ? PU_KF_REQ16 : 0u;
    return 0;
}

int pu_pack_req16(const pu_req* in, size_t n, pu_req16* out) {
    if (n && (!in || !out)) return pu::set_error(PU_EINVAL, "bad arguments");
    for (size_t i = 0; i < n; i++) {
        const pu_req& q = in[i];
        if (q.timer < 0 || q.timer >= (int64_t)1 << PU_REQ16_TIMER_BITS || q.core < 0 ||
            q.core >= 1 << PU_REQ16_CORE_BITS || q.prog_id < 0 || q.prog_id >= 1 << PU_REQ16_PROG_BITS ||
            q.mem_type > 1 || q.batch_start > 1 || q.tag != 0)
            return pu::set_error(PU_ERANGE, "request " + std::to_string(i) + " does not fit pu_req16");
        out[i].a = q.addr;
        out[i].b = PU_REQ16_B(q.timer, q.core, q.prog_id, q.mem_type, q.batch_start);
    }
    return 0;
}

}  // extern "C"

int pu::limit_positions(pu_handle* h, uint64_t* out, size_t n) {
    if (!h || (!out && n)) return pu::set_error(PU_EINVAL, "bad arguments");
    if (n > (size_t)h->R) return pu::set_error(PU_ERANGE, "more replicas than the handle holds");
    if (n == 0) return 0;
    int rrc = pu::resident_stop(h);
    if (rrc) return rrc;
    const Geo& g = h->geo;
    HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
    HIP_TRY(hipMemcpy2D(out, sizeof(uint64_t), h->arena + g.off_run + offsetof(RunState, limit_at), g.replica_bytes,
                        sizeof(uint64_t), n, hipMemcpyDeviceToHost), PU_EIO);
    return 0;
}

void pu::fork_sched(pu_handle* h, int src, int first, int n) {
    const pu::Sched* const own = h->rsched[(size_t)src].get();
    for (int d = first; d < first + n; d++)
        if (d != src) h->rsched[(size_t)d].reset(own ? new pu::Sched(*own) : nullptr);
}

int pu::run_device_flags(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
                         uint32_t extra_flags, bool use_replay_mode) {
    if (!h || !d_reqs || !d_off || !d_delay) return pu::set_error(PU_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    return launch(h, 0, h->R, d_reqs, d_off, d_delay, h->stream, nullptr, 0, extra_flags, false, use_replay_mode);
}

extern "C" {

int pu_run_device_sliced(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
                         uint64_t* d_pos, uint64_t budget_us, void* hip_stream) {
    if (!h || !d_reqs || !d_off || !d_delay || !d_pos) return pu::set_error(PU_EINVAL, "bad arguments");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    std::lock_guard<std::mutex> lk(h->mu);
    return launch(h, 0, h->R, d_reqs, d_off, d_delay, s, d_pos, budget_us * 100,   // s_memrealtime: 100 MHz
                  h->dev_req_flags);
}

int pu_pool_slots(pu_handle* h) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    const int res = pu_resident_replicas(h);
    if (res < 0) return res;
    return res < h->R ? res : h->R;
}

long pu_pool_words(int slots) { return slots < 1 ? pu::set_error(PU_EINVAL, "slots < 1") : (long)PU_POOL_WORDS(slots); }

int pu_run_device_pool(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
                       uint64_t* d_pos, uint32_t* d_sched, int slots, uint64_t budget_us, void* hip_stream) {
    if (!h || !d_reqs || !d_off || !d_delay || !d_pos || !d_sched || budget_us == 0)
        return pu::set_error(PU_EINVAL, "bad arguments (the pool needs a time slice: budget_us > 0)");
    const int most = pu_pool_slots(h);
    if (most < 0) return most;
    if (slots < 1 || slots > most)
        return pu::set_error(PU_ERANGE, "slots must be 1.." + std::to_string(most) + " (pu_pool_slots)");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    std::lock_guard<std::mutex> lk(h->mu);
    return launch(h, 0, slots, d_reqs, d_off, d_delay, s, d_pos, budget_us * 100, h->dev_req_flags, false, true,
                  d_sched);
}

int pu_synchronize(pu_handle* h) {
    if (!h) return pu::set_error(PU_EINVAL, "null handle");
    int qrc = pu::resident_quiesce(h);   // a device-wide wait would otherwise last until the resident kernel idles out
    if (qrc) return qrc;
    HIP_TRY(hipDeviceSynchronize(), PU_EIO);
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_ms = ms;
    return 0;
}

double pu_last_kernel_ms(pu_handle* h) { return h ? h->last_ms : 0.0; }

void pu_sim_start_time(pu_handle* h) {
    if (h) clock_gettime(CLOCK_REALTIME, &h->sim_start);
}
void pu_sim_finish_time(pu_handle* h) {
    if (h) clock_gettime(CLOCK_REALTIME, &h->sim_finish);
}

}  // extern "C"
