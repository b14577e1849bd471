// delay_hist.hip — an ensemble's delay quantiles on the device (pu_dhist_*,
// include/primeuncore.h): a log-linear histogram per replica and class, a stage
// beside the delay summaries (delay_sum.hip) on the same stream.  Each
// pu_dhist_add counts every replica's records [d_begin[r], d_end[r]) of the
// request and delay arrays into its histogram by the rule of delay_hist_step.h,
// which the host twins (pu_dhist_host_*, below) run too.
//
// State, one allocation per set:
//   histograms  uint64 [count][2][864] (13,824 B per replica)
//   quantiles   one pu_dhist_quantile per replica and class (40 B), as of the last call
//   slabs       uint64 [G][2][864], the partial sums of the ensemble total (G <= kGroups)
//   total       uint64 [2][864]
//
// dhist_add_kernel<FMT>: one launch per call, one workgroup of 256 per replica,
// which owns that replica's row for the launch; no atomics on device memory.
//   * The range and the loads are delay_stage.h's RecordSource; the class is all this
//     kernel needs of a record, so 8 B of it.
//   * The counters are 2 x 864 64-bit LDS counters of the workgroup (13,824 B static).
//     A record's key is class * 864 + bucket; every record in the range does one LDS
//     atomic add on its counter.  Reducing equal keys in the wave first (broadcast the
//     first live lane's key, ballot, one add of the popcount, up to four rounds) was
//     built and measured on the engine's own delays: it lost (DESIGN.md section 6d:
//     a wave instruction's 64 records fall into 47 counters there), so it is not here.
//   * At the end the non-zero counters are added to the replica's row by plain
//     read-modify-write.
// dhist_quantile_kernel: a wave owns one (replica, class).  Each lane sums 14
// consecutive buckets (64 x 14 >= 864), one wave scan gives every lane the count
// before its buckets, and per quantile the lane whose running sum first reaches the
// rank walks its own 14 buckets.
// Ensemble total (dhist_total_partial_kernel, dhist_total_sum_kernel): store and sum
// as run_results.hip's totals: a counter per lane, partial slabs over replica groups,
// then the sum of the slabs.
// Every loop is bounded by the range length or a constant.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "delay_hist_step.h"
#include "delay_stage.h"
#include "device_set.h"

using namespace pu_delay_hist;
using pu::round16;

namespace {

constexpr int kKeys = 2 * PU_DHIST_BUCKETS;         // counters of a replica
constexpr int kPerLane = 14;                        // buckets a lane of the quantile scan takes
constexpr int kGroups = 120;                        // replica groups of the total's first pass, at most
constexpr int kTiles = (kKeys + kThreads - 1) / kThreads;

static_assert(64 * kPerLane >= PU_DHIST_BUCKETS, "a wave covers a class");
static_assert(sizeof(pu_dhist_quantile) == 40, "count and eight buckets, no padding");

// the quantiles of one call
struct DhistQ {
    uint32_t ppm[PU_DHIST_MAX_Q];
    int32_t nq;
};

template <int FMT>
__global__ __launch_bounds__(kThreads) void dhist_add_kernel(u64* __restrict__ hist, const void* __restrict__ reqs,
                                                              const int32_t* __restrict__ delay,
                                                              const uint64_t* __restrict__ d_begin,
                                                              const uint64_t* __restrict__ d_end) {
    __shared__ u64 s_hist[kKeys];

    const int r = (int)blockIdx.x;
    const RecordRange rg(d_begin, d_end);
    if (rg.empty()) return;
    const uint64_t len = rg.len();
    const int tid = (int)threadIdx.x;

#pragma unroll
    for (int k = tid; k < kKeys; k += kThreads) s_hist[k] = 0;
    __syncthreads();

    const RecordSource<FMT, false> src(reqs, delay, rg.b, len);
    for (uint64_t base = 0; base < len; base += kTrip) {
        int32_t d[kUnroll];
        u64 w[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) valid[u] = src.load(base + (uint64_t)(u * kThreads + tid), d[u], w[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; u++)
            if (valid[u]) atomicAdd(&s_hist[key_of(src.cls(w[u]), d[u])], 1ull);
    }
    __syncthreads();   // the counters are complete

    u64* const row = hist + (size_t)r * kKeys;
#pragma unroll
    for (int k = tid; k < kKeys; k += kThreads) {
        const u64 c = s_hist[k];
        if (c) row[k] += c;
    }
}

// Pair p = blockIdx.x * kWaves + wave of [0, 2n): replica first + p / 2, class p & 1.
__global__ __launch_bounds__(kThreads) void dhist_quantile_kernel(const u64* __restrict__ hist, int first, int n,
                                                                   const DhistQ q, pu_dhist_quantile* __restrict__ out) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int p = (int)blockIdx.x * kWaves + wave;
    if (p >= 2 * n) return;   // the whole wave; the kernel has no barrier
    const int r = first + (p >> 1), c = p & 1;
    const u64* const h = hist + ((size_t)r * 2 + (size_t)c) * PU_DHIST_BUCKETS;

    u64 v[kPerLane];
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int k = lane * kPerLane + j;
        v[j] = k < PU_DHIST_BUCKETS ? h[k] : 0;
        s += v[j];
    }
    u64 incl = s;   // inclusive scan over the lanes
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const u64 t = __shfl_up(incl, k, 64);
        if (lane >= k) incl += t;
    }
    const u64 excl = incl - s;
    const u64 total = __shfl(incl, 63, 64);

    pu_dhist_quantile* const o = out + (size_t)r * 2 + (size_t)c;
    if (lane == 0) o->count = total;
#pragma unroll
    for (int i = 0; i < PU_DHIST_MAX_Q; i++) {
        if (i >= q.nq || total == 0) {
            if (lane == 0) o->bucket[i] = -1;
            continue;
        }
        const u64 rank = rank_of(total, q.ppm[i]);   // 1 .. total
        if (excl < rank && rank <= incl) {           // one lane: the running count reaches rank among its buckets
            u64 run = excl;
            int ans = -1;
#pragma unroll
            for (int j = 0; j < kPerLane; j++) {
                run += v[j];
                if (ans < 0 && run >= rank) ans = lane * kPerLane + j;
            }
            o->bucket[i] = ans;
        }
    }
}

// Per counter, the sum over the group's replicas first + grp, first + grp + G, ...
// (< first + n) into slab row grp.  G <= n, so every group has a replica.
__global__ __launch_bounds__(kThreads) void dhist_total_partial_kernel(const u64* __restrict__ hist, int first, int n, int G,
                                                                        u64* __restrict__ slab) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x, grp = (int)blockIdx.y;
    if (k >= kKeys) return;
    const int end = first + n;
    u64 sum = 0;
    for (int r0 = first + grp; r0 < end; r0 += G * kUnroll) {
        u64 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int r = r0 + u * G;
            v[u] = 0;
            if (r < end) v[u] = hist[(size_t)r * kKeys + (size_t)k];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) sum += v[u];
    }
    slab[(size_t)grp * kKeys + (size_t)k] = sum;
}

__global__ __launch_bounds__(kThreads) void dhist_total_sum_kernel(const u64* __restrict__ slab, int G, u64* __restrict__ tot) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (k >= kKeys) return;
    u64 sum = 0;
    for (int g = 0; g < G; g++) sum += slab[(size_t)g * kKeys + (size_t)k];
    tot[k] = sum;
}

}  // namespace

struct pu_dhist : pu::DeviceSet {
    int count = 0;
    int groups = 1;                 // slab rows allocated
    u64* hist = nullptr;
    pu_dhist_quantile* quant = nullptr;
    u64* slab = nullptr;
    u64* tot = nullptr;
};

extern "C" {

pu_dhist* pu_dhist_open(int count, int device) {
    if (count < 1) {
        pu::set_error(PU_EINVAL, "pu_dhist_open: no replicas");
        return nullptr;
    }
    if (pu::device_check(device, "the device histograms have no CPU fallback; pu_dhist_host_add folds host arrays") != 0)
        return nullptr;
    pu_dhist* s = pu::new_set<pu_dhist>();
    if (!s) return nullptr;
    s->count = count;
    s->groups = count < kGroups ? count : kGroups;

    // layout: histograms | quantile records | slabs | total
    const size_t off_q = round16((size_t)count * kKeys * 8);
    const size_t off_slab = off_q + round16((size_t)count * 2 * sizeof(pu_dhist_quantile));
    const size_t off_tot = off_slab + round16((size_t)s->groups * kKeys * 8);
    if (s->open(device, off_tot + round16((size_t)kKeys * 8),
                "pu_dhist_open: the histograms of " + std::to_string(count) + " replicas") != 0)
        return pu::drop_set(s);
    s->hist = (u64*)s->base;
    s->quant = (pu_dhist_quantile*)(s->base + off_q);
    s->slab = (u64*)(s->base + off_slab);
    s->tot = (u64*)(s->base + off_tot);
    if (hipMemsetAsync(s->base, 0, s->bytes, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dhist_close(pu_dhist* s) { pu::close_set(s); }

int pu_dhist_add(pu_dhist* s, const void* d_reqs, int fmt, const int32_t* d_delay, const uint64_t* d_begin,
                 const uint64_t* d_end, void* hip_stream) {
    return delay_add(s, "pu_dhist_add", d_reqs, fmt, d_delay, d_begin, d_end, hip_stream, [&](auto F, hipStream_t st) {
        hipLaunchKernelGGL((dhist_add_kernel<decltype(F)::value>), dim3((unsigned)s->count), dim3(kThreads), 0, st, s->hist,
                           d_reqs, d_delay, d_begin, d_end);
    });
}

int pu_dhist_read(pu_dhist* s, int first, int n, uint64_t* out) {
    const int rc = pu::replica_range(s ? s->count : 0, first, n, out != nullptr, "pu_dhist_read");
    if (rc) return rc < 0 ? rc : 0;
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpyAsync(out, s->hist + (size_t)first * kKeys, (size_t)n * kKeys * 8, hipMemcpyDeviceToHost, st) ==
                   hipSuccess;
        },
        "reading the histograms failed");
}

int pu_dhist_quantiles(pu_dhist* s, int first, int n, const uint32_t* ppm, int nq, pu_dhist_quantile* out) {
    int rc = pu::replica_range(s ? s->count : 0, first, n, out != nullptr, "pu_dhist_quantiles");
    if (rc < 0) return rc;
    if (!ppm || nq < 1 || nq > PU_DHIST_MAX_Q)
        return pu::set_error(PU_EINVAL, "pu_dhist_quantiles: between 1 and " + std::to_string(PU_DHIST_MAX_Q) + " quantiles");
    DhistQ q;
    std::memset(&q, 0, sizeof q);
    q.nq = nq;
    for (int i = 0; i < nq; i++) {
        if (ppm[i] > kPpmOne) return pu::set_error(PU_EINVAL, "pu_dhist_quantiles: a quantile above 1,000,000 ppm");
        q.ppm[i] = ppm[i];
    }
    if (rc) return 0;   // no replica
    rc = s->use();
    if (rc) return rc;
    // on the set's own stream, after the set's last call by its event
    hipStream_t st = s->stream;
    rc = s->order_before(st);
    if (rc) return rc;
    hipLaunchKernelGGL(dhist_quantile_kernel, dim3((unsigned)((2 * n + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, s->hist,
                       first, n, q, s->quant);
    rc = s->record_after(st, "pu_dhist_quantiles");
    if (rc) return rc;
    return s->read_back(
        [&](hipStream_t cs) {
            return hipMemcpyAsync(out, s->quant + (size_t)first * 2, (size_t)n * 2 * sizeof(pu_dhist_quantile),
                                  hipMemcpyDeviceToHost, cs) == hipSuccess;
        },
        "reading the quantiles failed");
}

int pu_dhist_read_total(pu_dhist* s, int first, int n, uint64_t* out) {
    // n == 0 fills the output too: without it there is nothing to call, as without a set
    int rc = pu::replica_range(s && out ? s->count : 0, first, n, true, "pu_dhist_read_total");
    if (rc < 0) return rc;
    if (rc) {
        std::memset(out, 0, (size_t)kKeys * 8);
        return 0;
    }
    rc = s->use();
    if (rc) return rc;
    hipStream_t st = s->stream;
    rc = s->order_before(st);
    if (rc) return rc;
    const int G = n < s->groups ? n : s->groups;
    hipLaunchKernelGGL(dhist_total_partial_kernel, dim3((unsigned)kTiles, (unsigned)G), dim3(kThreads), 0, st, s->hist, first,
                       n, G, s->slab);
    hipLaunchKernelGGL(dhist_total_sum_kernel, dim3((unsigned)kTiles), dim3(kThreads), 0, st, s->slab, G, s->tot);
    rc = s->record_after(st, "pu_dhist_read_total");
    if (rc) return rc;
    return s->read_back(
        [&](hipStream_t cs) { return hipMemcpyAsync(out, s->tot, (size_t)kKeys * 8, hipMemcpyDeviceToHost, cs) == hipSuccess; },
        "reading the total failed");
}

int pu_dhist_reset(pu_dhist* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dhist_reset: no set");
    return reset_words(s, s->hist, (size_t)s->count * kKeys, "pu_dhist_reset");
}

uint64_t pu_dhist_state_bytes(const pu_dhist* s) { return s ? (uint64_t)s->bytes : 0; }

int pu_dhist_host_add(uint64_t* hist, const void* reqs, int fmt, const int32_t* delays, size_t n) {
    if (!hist || !pu::req_fmt_ok(fmt) || (n && (!reqs || !delays)))
        return pu::set_error(PU_EINVAL, "pu_dhist_host_add: bad arguments");
    for (size_t i = 0; i < n; i++) hist[key_of(pu_delay_record::class_at(reqs, fmt, i), delays[i])]++;
    return 0;
}

int pu_dhist_host_quantiles(const uint64_t* hist_one_class, const uint32_t* ppm, int nq, uint64_t* count_out,
                            int32_t* bucket_out) {
    if (!hist_one_class || !ppm || !bucket_out || nq < 1 || nq > PU_DHIST_MAX_Q)
        return pu::set_error(PU_EINVAL, "pu_dhist_host_quantiles: bad arguments");
    for (int i = 0; i < nq; i++)
        if (ppm[i] > kPpmOne) return pu::set_error(PU_EINVAL, "pu_dhist_host_quantiles: a quantile above 1,000,000 ppm");
    const uint64_t count = class_count(hist_one_class);
    if (count_out) *count_out = count;
    for (int i = 0; i < nq; i++) bucket_out[i] = quantile_bucket(hist_one_class, count, ppm[i]);
    return 0;
}

int pu_dhist_bucket_of(int32_t d) { return bucket_of(d); }

int pu_dhist_bucket_bounds(int bucket, int32_t* lo, int32_t* hi) {
    if (!lo || !hi) return pu::set_error(PU_EINVAL, "pu_dhist_bucket_bounds: bad arguments");
    if (bucket < 0 || bucket >= PU_DHIST_BUCKETS) return pu::set_error(PU_ERANGE, "pu_dhist_bucket_bounds: no such bucket");
    bucket_bounds(bucket, lo, hi);
    return 0;
}

}  // extern "C"
