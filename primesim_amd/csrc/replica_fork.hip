// replica_fork.hip — a warmed replica branched on the device (pu_replica_fork,
// include/primeuncore.h).  A replica's whole engine state is one
// position-independent block of the handle's arena (every reference inside it is
// an offset or an index), so a fork is a copy of that block over each
// destination's block.  The index rules are in replica_fork_step.h.
//
// replica_fork_kernel<NT>: grid (tiles of the source) x (destination groups,
// G <= kMaxGroups), workgroups of 256.  A workgroup loads its 16-KiB tile of the
// source once, four 16-B loads per lane issued before any is used, then walks its
// group's destinations first + g, first + g + G, ... (src left out) and stores the
// tile to each with 16-B stores; the last tile of a replica is masked by lane.  The
// source is read G times in all (from L2 and the Infinity Cache after the first),
// every destination written once.  All addressing is 64-bit.  No atomics; the loop
// is bounded by n.  NT selects __builtin_nontemporal_store; which of the two is
// launched is decided by measurement and PRIMEUNCORE_FORK_STORES
// = plain | nt overrides it for that measurement.
//
// PU_FORK_BY_COPIES: one hipMemcpyAsync device-to-device per destination on the
// same stream: the yardstick, and the kernel's independent twin in the tests.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "geometry.h"
#include "handle.h"
#include "replica_fork_step.h"

using namespace pu_fork_step;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
static_assert(sizeof(u32x4) == kPieceBytes, "a piece is one 16-B load");

constexpr bool kDefaultNonTemporal = true;   // 4.6 % faster at C4 x 7,168 (130 GB), 1 % slower at C2 (8.5 GB)

template <bool NT>
__global__ __launch_bounds__(kLanes) void replica_fork_kernel(char* arena, uint64_t replica_bytes, int src, int first,
                                                               int n, int G) {
    const uint64_t tile = blockIdx.x;
    const int g = (int)blockIdx.y, lane = (int)threadIdx.x;
    const char* const from = arena + (uint64_t)src * replica_bytes;

    uint64_t off[kPieces];
    u32x4 v[kPieces];
#pragma unroll
    for (int u = 0; u < kPieces; u++) {
        off[u] = piece_offset(tile, lane, u);
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (piece_live(off[u], replica_bytes)) v[u] = *(const u32x4*)(from + off[u]);
    }
    const int64_t end = dest_end(first, n);
    for (int64_t d = dest_begin(first, g); d < end; d += G) {
        if (!dest_taken(d, src)) continue;
        char* const to = arena + (uint64_t)d * replica_bytes;
#pragma unroll
        for (int u = 0; u < kPieces; u++)
            if (piece_live(off[u], replica_bytes)) {
                if (NT) __builtin_nontemporal_store(v[u], (u32x4*)(to + off[u]));
                else *(u32x4*)(to + off[u]) = v[u];
            }
    }
}

bool non_temporal_stores() {
    const char* e = std::getenv("PRIMEUNCORE_FORK_STORES");
    if (e && !std::strcmp(e, "nt")) return true;
    if (e && !std::strcmp(e, "plain")) return false;
    return kDefaultNonTemporal;
}

}  // namespace

extern "C" int pu_replica_fork(pu_handle* h, int src, int first, int n, int flags, void* hip_stream) {
    if (flags & ~PU_FORK_BY_COPIES) return pu::set_error(PU_EINVAL, "pu_replica_fork: unknown flags");
    if (src < 0 || first < 0 || n < 0) return pu::set_error(PU_EINVAL, "pu_replica_fork: negative argument");
    if (!h) return pu::set_error(PU_EINVAL, "pu_replica_fork: no handle");
    if (src >= h->R) return pu::set_error(PU_ERANGE, "pu_replica_fork: source replica out of range");
    if ((int64_t)first + n > h->R) return pu::set_error(PU_ERANGE, "pu_replica_fork: more replicas than the handle holds");
    if (n == 0) return 0;

    std::lock_guard<std::mutex> lk(h->mu);
    int rc = pu::resident_stop(h);   // the source's queue headers leave the chip first
    if (rc) return rc;
    pu::fork_sched(h, src, first, n);
    if (dest_count(src, first, n) == 0) return 0;
    if (hipSetDevice(h->device) != hipSuccess) return pu::set_error(PU_ENODEV, "hipSetDevice failed");
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    const uint64_t bytes = h->geo.replica_bytes;

    if (flags & PU_FORK_BY_COPIES) {
        const char* const from = h->arena + (uint64_t)src * bytes;
        for (int d = first; d < first + n; d++)
            if (dest_taken(d, src) &&
                hipMemcpyAsync(h->arena + (uint64_t)d * bytes, from, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return pu::set_error(PU_EIO, "pu_replica_fork: copy to replica " + std::to_string(d) + " failed");
        return 0;
    }
    const dim3 grid((unsigned)tiles_of(bytes), (unsigned)groups_of(n));
    if (non_temporal_stores())
        hipLaunchKernelGGL(replica_fork_kernel<true>, grid, dim3(kLanes), 0, st, h->arena, bytes, src, first, n, (int)grid.y);
    else
        hipLaunchKernelGGL(replica_fork_kernel<false>, grid, dim3(kLanes), 0, st, h->arena, bytes, src, first, n, (int)grid.y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pu::set_error(PU_EIO, std::string("pu_replica_fork: launch failed: ") + hipGetErrorString(e));
    return 0;
}
