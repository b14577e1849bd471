// resident.cpp — the host side of resident mode (engine.hip resident_body;
// geometry.h PuMailbox): one latency-mode workgroup stays on the GPU and serves
// pu_access / short host batches of one replica through a mailbox in
// host-coherent pinned memory.  Every step of the protocol is here once:
//   post_stop        the STOP command
//   join             the kernel has left: wait for its stream, take its ack
//   resident_ensure  start (or restart) the kernel
//   resident_run     one command and its answer
//   resident_atexit  every live kernel told to stop when the process ends
// The handle's mutex guards all of it: the caller holds h->mu except where said
// (handle.h).  pu_set_resident and pu_resident_info are the ABI's view of it.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "handle.h"
#include "jit.h"

namespace {

constexpr size_t kResCap = 16384;   // requests per command (= the short-batch bound)

size_t res_bytes() { return sizeof(PuMailbox) + kResCap * (sizeof(pu_req) + sizeof(int32_t)); }

// Posts a STOP command: the kernel leaves when it sees it.  A STOP is never acked.
void post_stop(pu_handle::Resident& R) {
    volatile PuMailbox* mb = R.mb;
    mb->h.flags_cmd = PU_RES_STOP << 16;
    mb->h.n = 0;
    std::atomic_thread_fence(std::memory_order_release);
    mb->h.seq = ++R.seq;
}

// The kernel has left, or was told to: wait for its stream and take its ack.
int join(pu_handle* h) {
    auto& R = h->res;
    volatile PuMailbox* mb = R.mb;
    R.running = false;
    HIP_TRY(hipStreamSynchronize(R.stream), PU_EIO);
    // (commands answered by the fast word leave d.ack behind: R.acked knows them)
    R.acked = std::max<uint64_t>(R.acked, (uint64_t)mb->d.ack);
    return 0;
}

// Every handle with a resident kernel, joined at process exit through the
// mailbox alone (the kernel leaves by itself within the idle time anyway).
std::mutex g_res_mu;
std::vector<pu_handle*> g_res_handles;
void resident_atexit() {
    std::lock_guard<std::mutex> lk(g_res_mu);
    for (pu_handle* h : g_res_handles) {
        auto& R = h->res;
        if (!R.running || !R.mb) continue;
        volatile PuMailbox* mb = R.mb;
        post_stop(R);
        const auto t0 = std::chrono::steady_clock::now();
        while (!mb->d.exited && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(2)) {}
    }
}

// A resident kernel for `replica` is running (started or restarted here).
int resident_ensure(pu_handle* h, int replica) {
    auto& R = h->res;
    if (R.running && R.replica == replica && !((volatile PuMailbox*)R.mb)->d.exited) return 0;
    int rc = pu::resident_stop(h);
    if (rc) return rc;
    if (!R.mb) {
        void* p = nullptr;
        HIP_TRY(hipHostMalloc(&p, res_bytes(), hipHostMallocCoherent | hipHostMallocMapped), PU_ENOMEM);
        std::memset(p, 0, res_bytes());
        R.mb = (PuMailbox*)p;
        HIP_TRY(hipHostGetDevicePointer(&R.mb_dev, p, 0), PU_EIO);
        HIP_TRY(hipMalloc(&R.stage, kResCap * sizeof(pu_req)), PU_ENOMEM);
        HIP_TRY(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking), PU_EIO);
        HIP_TRY(hipEventCreateWithFlags(&R.after, hipEventDisableTiming), PU_EIO);
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (g_res_handles.empty()) std::atexit(resident_atexit);
        g_res_handles.push_back(h);
    }
    {   // the error flags this kernel starts from (fast answers do not carry them; full answers do)
        uint64_t e0 = 0;
        HIP_TRY(hipMemcpyAsync(&e0, h->arena + (size_t)replica * h->geo.replica_bytes + h->geo.off_stats +
                                        offsetof(EngineStats, error_flags), 8, hipMemcpyDeviceToHost, h->stream),
                PU_EIO);
        HIP_TRY(hipStreamSynchronize(h->stream), PU_EIO);
        R.err = e0;
    }
    volatile PuMailbox* mb = R.mb;
    mb->d.exited = 0;
    mb->d.ack = R.acked;   // the kernel waits for seq != ack: a posted, unacked command runs first
    mb->h.seq = R.seq;
    std::atomic_thread_fence(std::memory_order_release);
    // after everything already queued on the handle's stream (the header image it copies in)
    HIP_TRY(hipEventRecord(R.after, h->stream), PU_EIO);
    HIP_TRY(hipStreamWaitEvent(R.stream, R.after, 0), PU_EIO);
    if (pu::jit_launch_resident(h->jit, R.stream, h->d_geo, h->arena, replica, R.stage, R.mb_dev, R.idle_ticks,
                                (int)kResCap) != 0)
        return pu::set_error(PU_EIO, "resident kernel launch failed");
    h->last_kernel = pu::kJitResidentKernel;
    R.running = true;
    R.replica = replica;
    R.launches++;
    return 0;
}

}  // namespace

// Join the resident kernel: a STOP command unless it already left (idle), then
// wait for its stream.  Its headers are back in HBM afterwards.
int pu::resident_stop(pu_handle* h) {
    auto& R = h->res;
    if (!R.running) return 0;
    if (!((volatile PuMailbox*)R.mb)->d.exited) post_stop(R);
    int rc = join(h);
    if (rc) return rc;
    R.seq = R.acked;   // a STOP is never acked; the next kernel starts from the last completed command
    return 0;
}

int pu::resident_quiesce(pu_handle* h) {   // (unlocked callers) the engine state in HBM is current
    std::lock_guard<std::mutex> lk(h->mu);
    return resident_stop(h);
}

bool pu::resident_eligible(const pu_handle* h, size_t n) {
    return h->res.mode && h->jit.f[3][1] && h->lds_headers_ok && n <= kResCap;
}

// One command: the requests through the resident kernel; delays, error flags
// and (TLB) the last translated address come back through the mailbox.
int pu::resident_run(pu_handle* h, int replica, const pu_req* reqs, size_t n, uint32_t flags, int32_t* delay_out,
                     uint64_t* err_out, uint64_t* last_addr) {
    auto& R = h->res;
    int rc = resident_ensure(h, replica);
    if (rc) return rc;
    volatile PuMailbox* mb = R.mb;
    const auto t0 = std::chrono::steady_clock::now();
    static_assert(sizeof(pu_req) == sizeof(PuResHost::req0), "a request fits the command line");
    if (n == 1) std::memcpy((void*)mb->h.req0, reqs, sizeof(pu_req));   // travels with the command
    else std::memcpy(R.mb + 1, reqs, n * sizeof(pu_req));
    mb->h.n = (uint32_t)n;
    mb->h.flags_cmd = (flags & 0xFFFFu) | (PU_RES_RUN << 16);
    std::atomic_thread_fence(std::memory_order_release);
    const uint64_t seq = ++R.seq;
    mb->h.seq = seq;
    h->last_kernel = pu::kJitResidentKernel;   // the command goes to the running resident kernel
    // a one-request command may come back as the fast word {seq, delay}
    bool fast = false;
    for (uint64_t spin = 1;; spin++) {
        if (n == 1) {
            const uint64_t f = mb->d.fast;
            if ((uint32_t)f == (uint32_t)seq) {
                fast = true;
                if (delay_out) delay_out[0] = (int32_t)(uint32_t)(f >> 32);
                break;
            }
        }
        if (mb->d.ack == seq) break;
        if ((spin & 1023) == 0) {
            if (mb->d.exited && mb->d.ack != seq) {
                // it left (idle) just before the command arrived: a new kernel takes it
                rc = join(h);
                if (rc) return rc;
                rc = resident_ensure(h, replica);
                if (rc) return rc;
                continue;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                R.mode = 0;   // never again on this handle
                return pu::set_error(PU_EIO, "resident kernel did not answer within 60 s");
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    R.acked = seq;
    R.commands++;
    if (fast) {
        R.fast++;
        *err_out = R.err;      // no new error bit (else the kernel answers in full)
    } else {
        for (int k = 0; k < 4; k++) R.phase_ticks[k] += mb->d.phase[k];
        if (delay_out)
            std::memcpy(delay_out, (const int32_t*)((const pu_req*)(R.mb + 1) + kResCap), n * sizeof(int32_t));
        R.err = mb->d.err;
        *err_out = R.err;
        if (last_addr) *last_addr = mb->d.last_addr;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->last_ms = ms;
    R.call_ns += (uint64_t)(ms * 1e6);
    return 0;
}

void pu::resident_free(pu_handle* h) {
    auto& R = h->res;
    (void)resident_stop(h);
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        for (size_t i = 0; i < g_res_handles.size(); i++)
            if (g_res_handles[i] == h) {
                g_res_handles.erase(g_res_handles.begin() + (long)i);
                break;
            }
    }
    if (R.stage) (void)hipFree(R.stage);
    if (R.mb) (void)hipHostFree(R.mb);
    if (R.after) (void)hipEventDestroy(R.after);
    if (R.stream) (void)hipStreamDestroy(R.stream);
    R.stage = nullptr;
    R.mb = nullptr;
    R.after = nullptr;
    R.stream = nullptr;
}

extern "C" {

int pu_set_resident(pu_handle* h, int mode) {
    if (!h || mode < -1 || mode > 1) return pu::set_error(PU_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    const int prev = h->res.mode;
    if (mode == 0) {
        int rc = pu::resident_stop(h);
        if (rc) return rc;
    }
    if (mode >= 0) h->res.mode = mode;
    return prev;
}

int pu_resident_info(pu_handle* h, uint64_t* out, size_t n) {
    if (!h || (!out && n)) return pu::set_error(PU_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    const auto& R = h->res;
    const bool live = R.running && R.mb && !((volatile PuMailbox*)R.mb)->d.exited;
    const uint64_t v[10] = {live ? 1u : 0u, R.commands, R.launches, pu::resident_eligible(h, 1) ? 1u : 0u,
                            R.phase_ticks[0], R.phase_ticks[1], R.phase_ticks[2], R.phase_ticks[3], R.call_ns,
                            R.fast};
    for (size_t k = 0; k < n && k < 10; k++) out[k] = v[k];
    return (int)(n < 10 ? n : 10);
}

}  // extern "C"
