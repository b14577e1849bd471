// unit_hooks.cpp — the unit-test hooks of the C ABI (pu_unit_queue_run,
// pu_unit_mg1_run, pu_unit_network_run): each runs one piece of the engine
// (engine.hip's unit kernels: a queue, the M/G/1 wait, the network) on inputs
// of the caller's, on a small replica of its own.  No handle is involved.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "handle.h"
#include "jit.h"
#include "stats_rule.h"

namespace {

// RAII bag of device buffers for the unit hooks.
struct DevBufs {
    std::vector<void*> ptrs;
    ~DevBufs() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class T>
    T* up(const T* host, size_t n) {
        void* d = nullptr;
        if (hipMalloc(&d, n * sizeof(T) + 8) != hipSuccess) return nullptr;
        ptrs.push_back(d);
        if (host && n && hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T*)d;
    }
};

int unit_prepare(int device) {
    pu::jit_note_gpu();
    int rc = pu::device_check(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PU_ENODEV);
    return 0;
}

}  // namespace

extern "C" {

int pu_unit_queue_run(uint64_t min_proc, const uint64_t* t, const uint64_t* p, size_t n, uint64_t* delay_out,
                      uint64_t* mg1_calls, int device) {
    if ((!t || !p || !delay_out) && n) return pu::set_error(PU_EINVAL, "bad arguments");
    int rc = unit_prepare(device);
    if (rc) return rc;
    Geo g;
    std::memset(&g, 0, sizeof(g));
    g.off_qhdr = 0;
    g.off_qring = 256;
    g.nqueues = 1;
    g.replica_bytes = 256 + PU_QRING * sizeof(QueueSlot);
    DevBufs b;
    Geo* dg = b.up(&g, 1);
    char* base = b.up<char>(nullptr, g.replica_bytes);
    uint64_t* dt = b.up(t, n);
    uint64_t* dp = b.up(p, n);
    uint64_t* dout = b.up<uint64_t>(nullptr, n);
    uint64_t* dmg = b.up<uint64_t>(nullptr, 1);
    if (!dg || !base || !dt || !dp || !dout || !dmg) return pu::set_error(PU_ENOMEM, "unit buffers");
    HIP_TRY(hipMemset(base, 0, g.replica_bytes), PU_EIO);
    rc = pu_engine_init_queues(base, g.replica_bytes, g.off_qhdr, g.off_qring, 1, 1, 1, nullptr);   // wide header
    if (rc) return pu::set_error(rc, "queue init failed");
    rc = pu_engine_unit_queue(dg, base, min_proc, dt, dp, n, dout, dmg, nullptr);
    if (rc) return pu::set_error(rc, "unit queue launch failed");
    HIP_TRY(hipDeviceSynchronize(), PU_EIO);
    if (n) HIP_TRY(hipMemcpy(delay_out, dout, n * 8, hipMemcpyDeviceToHost), PU_EIO);
    if (mg1_calls) HIP_TRY(hipMemcpy(mg1_calls, dmg, 8, hipMemcpyDeviceToHost), PU_EIO);
    return 0;
}

int pu_unit_mg1_run(const uint64_t* num_arrivals, const double* sum, const double* sum_sq, const uint64_t* newest,
                    size_t n, uint64_t* wait_out, int device) {
    return pu_unit_mg1_path_run(num_arrivals, sum, sum_sq, newest, n, wait_out, nullptr, device);
}

int pu_unit_mg1_path_run(const uint64_t* num_arrivals, const double* sum, const double* sum_sq,
                         const uint64_t* newest, size_t n, uint64_t* wait_out, uint8_t* path_out, int device) {
    if ((!num_arrivals || !sum || !sum_sq || !newest || !wait_out) && n) return pu::set_error(PU_EINVAL, "bad arguments");
    for (size_t i = 0; i < n; i++)
        if (num_arrivals[i] >= (1ull << 53))   // the engine holds the count as an exact double
            return pu::set_error(PU_ERANGE, "num_arrivals >= 2^53");
    int rc = unit_prepare(device);
    if (rc) return rc;
    DevBufs b;
    uint64_t* dn = b.up(num_arrivals, n);
    double* ds = b.up(sum, n);
    double* dq = b.up(sum_sq, n);
    uint64_t* dw = b.up(newest, n);
    uint64_t* dout = b.up<uint64_t>(nullptr, n);
    uint8_t* dpath = path_out ? b.up<uint8_t>(nullptr, n) : nullptr;
    if (n && (!dn || !ds || !dq || !dw || !dout || (path_out && !dpath))) return pu::set_error(PU_ENOMEM, "unit buffers");
    rc = pu_engine_unit_mg1(dn, ds, dq, dw, n, dout, dpath, nullptr);
    if (rc) return pu::set_error(rc, "unit M/G/1 launch failed");
    HIP_TRY(hipDeviceSynchronize(), PU_EIO);
    if (n) HIP_TRY(hipMemcpy(wait_out, dout, n * 8, hipMemcpyDeviceToHost), PU_EIO);
    if (n && path_out) HIP_TRY(hipMemcpy(path_out, dpath, n, hipMemcpyDeviceToHost), PU_EIO);
    return 0;
}

int pu_unit_network_run(int num_nodes, int net_type, int data_width, int header_flits, uint64_t router_delay,
                        uint64_t link_delay, uint64_t inject_delay, const int32_t* src, const int32_t* dst,
                        const int32_t* len, const uint64_t* timer, size_t n, uint64_t* delay_out, pu_stats* st,
                        int device) {
    if ((!src || !dst || !len || !timer || !delay_out) && n) return pu::set_error(PU_EINVAL, "bad arguments");
    if (num_nodes < 1 || data_width < 1 || link_delay < 1) return pu::set_error(PU_EINVAL, "bad network");
    for (size_t i = 0; i < n; i++)
        if (src[i] < 0 || src[i] >= num_nodes || dst[i] < 0 || dst[i] >= num_nodes)
            return pu::set_error(PU_ERANGE, "node id out of range");
    int rc = unit_prepare(device);
    if (rc) return rc;
    Geo g;
    std::memset(&g, 0, sizeof(g));
    g.N = num_nodes;
    g.net_type = net_type;
    g.net_width = net_type == 1 ? (int)std::ceil(std::cbrt((double)num_nodes)) : (int)std::ceil(std::sqrt((double)num_nodes));
    g.header_flits = header_flits;
    g.data_width = data_width;
    g.router_delay = router_delay;
    g.link_delay = link_delay;
    g.inject_delay = inject_delay;
    const int w = g.net_width;
    pu_set_net_magic(w, header_flits, data_width, -1, &g.w_magic, &g.w2_magic, &g.w2, &g.blk_len, &g.plen_blk);
    g.nlinks = w > 1 ? (w - 1) * w * (net_type == 1 ? 3 * w : 2) : 0;
    g.nqueues = g.nlinks;
    pu::Layout lay;
    g.off_qhdr = lay.take((uint64_t)g.nqueues * PU_HDR_WIDE_BYTES);   // the unit hook's wide headers
    g.off_qring = lay.take((uint64_t)g.nqueues * PU_QRING * sizeof(QueueSlot));
    g.off_stats = lay.take(sizeof(EngineStats));
    g.replica_bytes = pu::align_up(lay.cur, 4096);
    DevBufs b;
    Geo* dg = b.up(&g, 1);
    char* base = b.up<char>(nullptr, g.replica_bytes);
    int32_t* ds = b.up(src, n);
    int32_t* dd = b.up(dst, n);
    int32_t* dl = b.up(len, n);
    uint64_t* dt = b.up(timer, n);
    uint64_t* dout = b.up<uint64_t>(nullptr, n);
    if (!dg || !base || !ds || !dd || !dl || !dt || !dout) return pu::set_error(PU_ENOMEM, "unit buffers");
    HIP_TRY(hipMemset(base, 0, g.replica_bytes), PU_EIO);
    rc = pu_engine_init_queues(base, g.replica_bytes, g.off_qhdr, g.off_qring, g.nqueues, 1, 1, nullptr);
    if (rc) return pu::set_error(rc, "queue init failed");
    rc = pu_engine_unit_network(dg, base, ds, dd, dl, dt, n, dout, nullptr);
    if (rc) return pu::set_error(rc, "unit network launch failed");
    HIP_TRY(hipDeviceSynchronize(), PU_EIO);
    if (n) HIP_TRY(hipMemcpy(delay_out, dout, n * 8, hipMemcpyDeviceToHost), PU_EIO);
    if (st) {
        EngineStats es;
        HIP_TRY(hipMemcpy(&es, base + g.off_stats, sizeof(es), hipMemcpyDeviceToHost), PU_EIO);
        // no cache level: the network's counters, link_flits, mg1_calls and error_flags; all else stayed zero
        const uint64_t none[pu::kStatRows][4] = {};
        pu::stats_fill(*st, es, 0, none);
    }
    return 0;
}

}  // extern "C"
