// delay_series.hip — an ensemble's delays over simulated time on the device
// (pu_dseries_*, include/primeuncore.h): per replica, class and epoch of the records'
// own timers a cell of count, sum, largest delay and number of non-positive delays, a
// stage beside the delay summaries (delay_sum.hip), histograms (delay_hist.hip) and
// slowest requests (delay_tail.hip) on the same stream.  Each pu_dseries_add folds
// every replica's records [d_begin[r], d_end[r]) of the request and delay arrays into
// its cells by the rule of delay_series_step.h, which the host twin
// (pu_dseries_host_add, below) runs too.
//
// State, one allocation per set (E epochs, fixed at open):
//   cells   pu_dseries_cell [count][2][E] (32 B each; 64 E bytes per replica)
//   slabs   pu_dseries_cell [G][2][E], the partial merges of the ensemble total (G <= kGroups)
//   total   pu_dseries_cell [2][E]
//
// dseries_add_kernel<FMT>: one launch per call, one workgroup of 256 per replica,
// which owns that replica's row for the launch; no atomics on device memory.
//   * The range and the loads are delay_stage.h's TimedRecordSource: 8 B of a pu_req16,
//     two 8-B words of a pu_req, in the lines the other stages' loads touch.
//   * The partial cells are the workgroup's pu_dseries_cell [2][E] in dynamic LDS (64 E
//     bytes, 32 KB at E = 512), 64-bit like the stored ones: exact for a range of any length.
//   * A record's key is class * E + epoch; every record in the range does its own LDS
//     atomics on its cell: count, sum, and nonpos or max.  Reducing equal keys in the wave
//     first (broadcast the first live lane's key, ballot, popcounts and DPP scans of sum and
//     maximum, one lane's update, up to four rounds) was built and measured on the engine's
//     own records: it lost (the engine's timers restart every quantum,
//     so a wave instruction's 64 records fall into 19 cells at E = 64 and 59 at E = 512
//     there), so it is not here.
//   * At the end the non-empty cells are merged into the replica's row by plain
//     read-modify-write.
// Ensemble total (dseries_total_partial_kernel, dseries_total_merge_kernel): store and
// merge as delay_hist.hip's totals: a cell per lane, partial slabs over replica groups,
// then the merge of the slabs.
// Every loop is bounded by the range length or a constant.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "delay_series_step.h"
#include "delay_stage.h"
#include "device_set.h"

using namespace pu_delay_series;
using pu::round16;

namespace {

constexpr int kGroups = 120;   // replica groups of the total's first pass, at most
constexpr int kCellWords = (int)(sizeof(pu_dseries_cell) / sizeof(u64));

// fold_one on a cell in LDS that other lanes and waves fold into as well
__device__ inline void fold_atomic(pu_dseries_cell* c, int32_t d) {
    atomicAdd((u64*)&c->count, 1ull);
    atomicAdd((u64*)&c->sum, (u64)(int64_t)d);
    if (d <= 0)
        atomicAdd((u64*)&c->nonpos, 1ull);
    else
        atomicMax(&c->max, d);
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void dseries_add_kernel(pu_dseries_cell* __restrict__ cells, int E, int64_t t0, int shift,
                                                                const void* __restrict__ reqs,
                                                                const int32_t* __restrict__ delay,
                                                                const uint64_t* __restrict__ d_begin,
                                                                const uint64_t* __restrict__ d_end) {
    extern __shared__ __align__(16) unsigned char s_raw[];   // pu_dseries_cell [2][E]
    pu_dseries_cell* const s = (pu_dseries_cell*)s_raw;

    const int r = (int)blockIdx.x;
    const RecordRange rg(d_begin, d_end);
    if (rg.empty()) return;
    const uint64_t len = rg.len();
    const int tid = (int)threadIdx.x;
    const int nkeys = 2 * E;

    for (int k = tid; k < nkeys * kCellWords; k += kThreads) ((u64*)s_raw)[k] = 0;
    __syncthreads();

    const TimedRecordSource<FMT> src(reqs, delay, rg.b, len);
    for (uint64_t base = 0; base < len; base += kTrip) {
        int32_t d[kUnroll];
        u64 t[kUnroll], w[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) valid[u] = src.load(base + (uint64_t)(u * kThreads + tid), d[u], t[u], w[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int key = key_of(src.cls(w[u]), epoch_of(src.timer(t[u], w[u]), E, t0, shift), E);
            if (valid[u]) fold_atomic(s + key, d[u]);
        }
    }
    __syncthreads();   // the cells are complete

    pu_dseries_cell* const row = cells + (size_t)r * (size_t)nkeys;
    for (int k = tid; k < nkeys; k += kThreads) {
        const pu_dseries_cell c = s[k];
        if (c.count) {
            pu_dseries_cell o = row[k];
            merge(&o, c);
            row[k] = o;
        }
    }
}

// Per cell, the merge over the group's replicas first + grp, first + grp + G, ...
// (< first + n) into slab row grp.  G <= n, so every group has a replica.
__global__ __launch_bounds__(kThreads) void dseries_total_partial_kernel(const pu_dseries_cell* __restrict__ cells, int nkeys,
                                                                          int first, int n, int G,
                                                                          pu_dseries_cell* __restrict__ slab) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x, grp = (int)blockIdx.y;
    if (k >= nkeys) return;
    const int end = first + n;
    pu_dseries_cell acc = {};
    for (int r0 = first + grp; r0 < end; r0 += G * kUnroll) {
        pu_dseries_cell v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int r = r0 + u * G;
            v[u] = pu_dseries_cell{};
            if (r < end) v[u] = cells[(size_t)r * (size_t)nkeys + (size_t)k];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) merge(&acc, v[u]);
    }
    slab[(size_t)grp * (size_t)nkeys + (size_t)k] = acc;
}

__global__ __launch_bounds__(kThreads) void dseries_total_merge_kernel(const pu_dseries_cell* __restrict__ slab, int nkeys, int G,
                                                                        pu_dseries_cell* __restrict__ tot) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (k >= nkeys) return;
    pu_dseries_cell acc = {};
    for (int g = 0; g < G; g++) merge(&acc, slab[(size_t)g * (size_t)nkeys + (size_t)k]);
    tot[k] = acc;
}

}  // namespace

struct pu_dseries : pu::DeviceSet {
    int count = 0;
    int epochs = 0;
    int64_t t0 = 0;
    int shift = 0;
    int groups = 1;                 // slab rows allocated
    pu_dseries_cell* cells = nullptr;
    pu_dseries_cell* slab = nullptr;
    pu_dseries_cell* tot = nullptr;

    int nkeys() const { return 2 * epochs; }
};

extern "C" {

pu_dseries* pu_dseries_open(int count, int epochs, int64_t t0, int shift, int device) {
    if (count < 1) {
        pu::set_error(PU_EINVAL, "pu_dseries_open: no replicas");
        return nullptr;
    }
    if (!epochs_ok(epochs)) {
        pu::set_error(PU_EINVAL, "pu_dseries_open: a series holds between 1 and " + std::to_string(kMaxEpochs) + " epochs");
        return nullptr;
    }
    if (!shift_ok(shift)) {
        pu::set_error(PU_EINVAL, "pu_dseries_open: an epoch is 2^shift cycles, shift between 0 and " + std::to_string(kMaxShift));
        return nullptr;
    }
    if (pu::device_check(device, "the device epoch series have no CPU fallback; pu_dseries_host_add folds host arrays") != 0)
        return nullptr;
    pu_dseries* s = pu::new_set<pu_dseries>();
    if (!s) return nullptr;
    s->count = count;
    s->epochs = epochs;
    s->t0 = t0;
    s->shift = shift;
    s->groups = count < kGroups ? count : kGroups;

    // layout: cells | slabs | total
    const size_t row = (size_t)s->nkeys() * sizeof(pu_dseries_cell);
    const size_t off_slab = (size_t)count * row;
    const size_t off_tot = off_slab + (size_t)s->groups * row;
    if (s->open(device, off_tot + row, "pu_dseries_open: the series of " + std::to_string(count) + " replicas") != 0)
        return pu::drop_set(s);
    s->cells = (pu_dseries_cell*)s->base;
    s->slab = (pu_dseries_cell*)(s->base + off_slab);
    s->tot = (pu_dseries_cell*)(s->base + off_tot);
    if (hipMemsetAsync(s->base, 0, s->bytes, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dseries_close(pu_dseries* s) { pu::close_set(s); }

int pu_dseries_add(pu_dseries* s, const void* d_reqs, int fmt, const int32_t* d_delay, const uint64_t* d_begin,
                   const uint64_t* d_end, void* hip_stream) {
    return delay_add(s, "pu_dseries_add", d_reqs, fmt, d_delay, d_begin, d_end, hip_stream, [&](auto F, hipStream_t st) {
        const size_t lds = (size_t)s->nkeys() * sizeof(pu_dseries_cell);
        hipLaunchKernelGGL((dseries_add_kernel<decltype(F)::value>), dim3((unsigned)s->count), dim3(kThreads), lds, st, s->cells,
                           s->epochs, s->t0, s->shift, d_reqs, d_delay, d_begin, d_end);
    });
}

int pu_dseries_read(pu_dseries* s, int first, int n, pu_dseries_cell* out) {
    const int rc = pu::replica_range(s ? s->count : 0, first, n, out != nullptr, "pu_dseries_read");
    if (rc) return rc < 0 ? rc : 0;
    const size_t row = (size_t)s->nkeys();
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpyAsync(out, s->cells + (size_t)first * row, (size_t)n * row * sizeof(pu_dseries_cell),
                                  hipMemcpyDeviceToHost, st) == hipSuccess;
        },
        "reading the series failed");
}

int pu_dseries_read_total(pu_dseries* s, int first, int n, pu_dseries_cell* out) {
    // n == 0 fills the output too: without it there is nothing to call, as without a set
    int rc = pu::replica_range(s && out ? s->count : 0, first, n, true, "pu_dseries_read_total");
    if (rc < 0) return rc;
    const size_t row = (size_t)s->nkeys() * sizeof(pu_dseries_cell);
    if (rc) {
        std::memset(out, 0, row);
        return 0;
    }
    rc = s->use();
    if (rc) return rc;
    // on the set's own stream, after the set's last call by its event
    hipStream_t st = s->stream;
    rc = s->order_before(st);
    if (rc) return rc;
    const int G = n < s->groups ? n : s->groups;
    const unsigned tiles = (unsigned)((s->nkeys() + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(dseries_total_partial_kernel, dim3(tiles, (unsigned)G), dim3(kThreads), 0, st, s->cells, s->nkeys(), first,
                       n, G, s->slab);
    hipLaunchKernelGGL(dseries_total_merge_kernel, dim3(tiles), dim3(kThreads), 0, st, s->slab, s->nkeys(), G, s->tot);
    rc = s->record_after(st, "pu_dseries_read_total");
    if (rc) return rc;
    return s->read_back([&](hipStream_t cs) { return hipMemcpyAsync(out, s->tot, row, hipMemcpyDeviceToHost, cs) == hipSuccess; },
                        "reading the total failed");
}

int pu_dseries_reset(pu_dseries* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dseries_reset: no set");
    return reset_words(s, s->cells, (size_t)s->count * (size_t)s->nkeys() * kCellWords, "pu_dseries_reset");
}

uint64_t pu_dseries_state_bytes(const pu_dseries* s) { return s ? (uint64_t)s->bytes : 0; }

int pu_dseries_epochs(const pu_dseries* s) { return s ? s->epochs : 0; }

int pu_dseries_host_add(pu_dseries_cell* cells, int epochs, int64_t t0, int shift, const void* reqs, int fmt,
                        const int32_t* delays, size_t n) {
    if (!cells || !epochs_ok(epochs) || !shift_ok(shift) || !pu::req_fmt_ok(fmt) || (n && (!reqs || !delays)))
        return pu::set_error(PU_EINVAL, "pu_dseries_host_add: bad arguments");
    fold(cells, epochs, t0, shift, reqs, fmt, delays, n);
    return 0;
}

int pu_dseries_epoch_of(int64_t timer, int epochs, int64_t t0, int shift) {
    if (!epochs_ok(epochs) || !shift_ok(shift)) return pu::set_error(PU_EINVAL, "pu_dseries_epoch_of: bad arguments");
    return epoch_of(timer, epochs, t0, shift);
}

}  // extern "C"
