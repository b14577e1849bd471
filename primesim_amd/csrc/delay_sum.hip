// delay_sum.hip — an ensemble's delays summarised on the device (pu_dsum_*,
// include/primeuncore.h): the last stage of a device-side ensemble.  A set keeps
// one pu_dsum_replica per replica, and optionally a (count, sum) pair per core,
// in device memory; each pu_dsum_add folds every replica's records
// [d_begin[r], d_end[r]) of the request and delay arrays into them by the rule of
// delay_sum_step.h, which the host fold (pu_dsum_host_add, below) runs too.
//
// State, one allocation per set:
//   summaries   one pu_dsum_replica per replica (568 B)
//   with per-core tables: num_cores (int32) and the first core's index (uint64)
//   per replica, then two arrays over all cores of all replicas, a replica's
//   cores contiguous: count (uint64) and sum (int64)
//
// Kernel: one launch per call, one workgroup of 256 per replica, which owns that
// replica's rows for the launch: nothing is accumulated across workgroups and the
// running summary is updated by plain read-modify-write at the end.
//   * The range and the loads are delay_stage.h's RecordSource, asked for the core
//     id as well as the class.
//   * sum, min, max and the out-of-range count live in per-lane registers and meet
//     once, after the loop: a wave reduction by __shfl_xor, then across the four
//     waves through LDS.
//   * the histogram is 2 x 32 64-bit LDS counters of the workgroup, by LDS atomics;
//     a class's count is the sum of its buckets.
//   * per core: a message is up to 100 consecutive requests of one core, so the 64
//     records of a wave-instruction mostly hold one core id.  Each run of equal ids
//     is reduced in the wave first (ballot of "differs from the lane before", a
//     segmented scan by __shfl_up, the run's length from the ballot) and the run's
//     last lane does one add of (length, sum): into an LDS table while the replica
//     has at most kLdsCores cores, flushed to its rows at the end, else by atomics
//     straight on its own rows in device memory (owned by this workgroup, so they
//     only meet the workgroup's other waves).
// LDS is all in the dynamic region (its base stays 16-byte aligned): 768 B plus
// 16 B per core of the largest table among the set's replicas, so 17,152 B at
// 1,024 cores = fourteen 1,280-B units, eight workgroups per CU.
// Every loop is bounded by the range length or a constant.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "delay_stage.h"
#include "delay_sum_step.h"
#include "device_set.h"

using namespace pu_delay_sum;
using pu::round16;

namespace {

constexpr int kLdsCores = 1024;   // the largest per-core table kept in LDS

// what a wave leaves for the combine across waves
struct WavePart {
    long long sum[2];
    unsigned long long oor;
    int32_t mn[2], mx[2];
};

// dynamic LDS, byte offsets (multiples of 16)
constexpr int kOffHist = 0;     // unsigned long long [2][32]
constexpr int kOffPart = 512;   // WavePart [kWaves]
constexpr int kOffTab = 768;    // unsigned long long count[nc], then sum[nc]
static_assert(sizeof(WavePart) * kWaves <= kOffTab - kOffPart, "the wave partials fit their slot");

__global__ __launch_bounds__(kThreads) void dsum_reset_kernel(pu_dsum_replica* rep, const int32_t* ncores,
                                                               const uint64_t* core0, uint64_t* g_cnt, int64_t* g_sum) {
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    pu_dsum_replica* R = rep + r;
    if (tid < 2 * PU_DSUM_BUCKETS) R->cls[tid >> 5].hist[tid & 31] = 0;
    if (tid < 2) {
        R->cls[tid].count = 0;
        R->cls[tid].sum = 0;
        R->cls[tid].min = INT32_MAX;
        R->cls[tid].max = INT32_MIN;
    }
    if (tid == 0) R->core_out_of_range = 0;
    if (ncores) {
        const int nc = ncores[r];
        const uint64_t c0 = core0[r];
        for (int k = tid; k < nc; k += kThreads) {
            g_cnt[c0 + k] = 0;
            g_sum[c0 + k] = 0;
        }
    }
}

template <int FMT, bool CORES>
__global__ __launch_bounds__(kThreads) void dsum_add_kernel(pu_dsum_replica* rep, const int32_t* ncores,
                                                             const uint64_t* core0, uint64_t* g_cnt, int64_t* g_sum,
                                                             const void* reqs, const int32_t* delay,
                                                             const uint64_t* d_begin, const uint64_t* d_end) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    unsigned long long* const s_hist = (unsigned long long*)(s_mem + kOffHist);
    WavePart* const s_part = (WavePart*)(s_mem + kOffPart);
    unsigned long long* const s_tab = (unsigned long long*)(s_mem + kOffTab);

    const int r = (int)blockIdx.x;
    const RecordRange rg(d_begin, d_end);
    if (rg.empty()) return;
    const uint64_t len = rg.len();
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = CORES ? ncores[r] : 0;
    const uint32_t limit = core_limit(nc);
    const bool lds_tab = CORES && nc <= kLdsCores;
    unsigned long long* const my_cnt = CORES ? (unsigned long long*)g_cnt + core0[r] : nullptr;
    unsigned long long* const my_sum = CORES ? (unsigned long long*)g_sum + core0[r] : nullptr;

    if (tid < 2 * PU_DSUM_BUCKETS) s_hist[tid] = 0;
    if (lds_tab)
        for (int k = tid; k < 2 * nc; k += kThreads) s_tab[k] = 0;
    __syncthreads();

    long long sum0 = 0, sum1 = 0;
    unsigned long long oor = 0;
    int32_t mn0 = INT32_MAX, mn1 = INT32_MAX, mx0 = INT32_MIN, mx1 = INT32_MIN;

    // with the core id: out of range is counted without tables too
    const RecordSource<FMT, true> src(reqs, delay, rg.b, len);
    for (uint64_t base = 0; base < len; base += kTrip) {
        int32_t d[kUnroll];
        typename RecordSource<FMT, true>::Word w[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) valid[u] = src.load(base + (uint64_t)(u * kThreads + tid), d[u], w[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            int32_t core;
            bool wr;
            if (FMT == PU_REQ_FMT_16) {
                core = core_of_req16_b(w[u].x);
                wr = class_of_req16_b(w[u].x) != 0;
            } else {
                core = (int32_t)(uint32_t)w[u].x;
                wr = class_of_mem_type((uint32_t)(w[u].y & 0xFFu)) != 0;
            }
            const int32_t dv = d[u];
            const bool out = core_out_of_range(core, limit);
            if (valid[u]) {
                sum0 += wr ? 0 : dv;
                sum1 += wr ? dv : 0;
                mn0 = min(mn0, wr ? INT32_MAX : dv);
                mn1 = min(mn1, wr ? dv : INT32_MAX);
                mx0 = max(mx0, wr ? INT32_MIN : dv);
                mx1 = max(mx1, wr ? dv : INT32_MIN);
                oor += out ? 1u : 0u;
                atomicAdd(&s_hist[(wr ? PU_DSUM_BUCKETS : 0) + bucket_of(dv)], 1ull);
            }
            if (CORES) {
                // runs of equal core ids among the wave's 64 consecutive records; records past the
                // range and cores out of range have key -1 and add nothing
                const bool ok = valid[u] && !out;
                const int32_t key = ok ? core : -1;
                const int32_t prev = __shfl_up(key, 1, 64);
                const bool head = lane == 0 || key != prev;
                const unsigned long long heads = __ballot(head);
                const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // bit 0 is always set
                long long s = ok ? (long long)dv : 0;
#pragma unroll
                for (int k = 1; k < 64; k <<= 1) {
                    const long long v = __shfl_up(s, k, 64);
                    if (lane - k >= start) s += v;
                }
                const bool tail = lane == 63 || (((heads >> 1) >> lane) & 1ull);
                if (ok && tail) {
                    const unsigned long long n = (unsigned long long)(lane - start + 1);
                    if (lds_tab) {
                        atomicAdd(&s_tab[key], n);
                        atomicAdd(&s_tab[nc + key], (unsigned long long)s);
                    } else {
                        atomicAdd(&my_cnt[key], n);
                        atomicAdd(&my_sum[key], (unsigned long long)s);
                    }
                }
            }
        }
    }

    // the wave's registers meet
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sum0 += __shfl_xor(sum0, m, 64);
        sum1 += __shfl_xor(sum1, m, 64);
        oor += __shfl_xor(oor, m, 64);
        mn0 = min(mn0, __shfl_xor(mn0, m, 64));
        mn1 = min(mn1, __shfl_xor(mn1, m, 64));
        mx0 = max(mx0, __shfl_xor(mx0, m, 64));
        mx1 = max(mx1, __shfl_xor(mx1, m, 64));
    }
    if (lane == 0) {
        WavePart& p = s_part[wave];
        p.sum[0] = sum0;
        p.sum[1] = sum1;
        p.oor = oor;
        p.mn[0] = mn0;
        p.mn[1] = mn1;
        p.mx[0] = mx0;
        p.mx[1] = mx1;
    }
    __syncthreads();   // the partials, the histogram and the table are complete

    if (lds_tab)
        for (int k = tid; k < nc; k += kThreads) {
            const unsigned long long c = s_tab[k];
            if (c) {
                my_cnt[k] += c;
                my_sum[k] += s_tab[nc + k];
            }
        }
    if (wave == 0) {   // lane = class * 32 + bucket
        pu_dsum_replica* const R = rep + r;
        const int c = lane >> 5, bk = lane & 31;
        const unsigned long long h = s_hist[lane];
        if (h) R->cls[c].hist[bk] += h;
        unsigned long long n = h;   // the class's count: the sum over its 32 buckets
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
        if (bk == 0) {
            long long s = 0;
            unsigned long long o = 0;
            int32_t mn = INT32_MAX, mx = INT32_MIN;
            for (int k = 0; k < kWaves; k++) {
                s += s_part[k].sum[c];
                o += s_part[k].oor;
                mn = min(mn, s_part[k].mn[c]);
                mx = max(mx, s_part[k].mx[c]);
            }
            pu_dsum_class* const C = &R->cls[c];
            C->count += n;
            C->sum += s;
            C->min = min(C->min, mn);
            C->max = max(C->max, mx);
            if (c == 0) R->core_out_of_range += o;
        }
    }
}

}  // namespace

struct pu_dsum : pu::DeviceSet {
    int count = 0;
    bool cores = false;
    std::vector<int32_t> nc;        // per replica (with tables)
    std::vector<uint64_t> core0;    // a replica's first element in the per-core arrays
    size_t lds_bytes = 0;           // dynamic LDS of a launch
    pu_dsum_replica* rep = nullptr;
    int32_t* d_nc = nullptr;
    uint64_t* d_core0 = nullptr;
    uint64_t* g_cnt = nullptr;
    int64_t* g_sum = nullptr;
};

namespace {

int launch_reset(pu_dsum* s) {
    int rc = s->order_before(s->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(dsum_reset_kernel, dim3((unsigned)s->count), dim3(kThreads), 0, s->stream, s->rep, s->d_nc,
                       s->d_core0, s->g_cnt, s->g_sum);
    return s->record_after(s->stream, "pu_dsum_reset");
}

}  // namespace

extern "C" {

pu_dsum* pu_dsum_open(int count, const int32_t* num_cores, int device) {
    if (count < 1) {
        pu::set_error(PU_EINVAL, "pu_dsum_open: no replicas");
        return nullptr;
    }
    if (num_cores)
        for (int i = 0; i < count; i++)
            if (num_cores[i] < 1) {
                pu::set_error(PU_EINVAL, "pu_dsum_open: invalid num_cores (replica " + std::to_string(i) + ")");
                return nullptr;
            }
    if (pu::device_check(device, "the device summaries have no CPU fallback; pu_dsum_host_add folds host arrays") != 0)
        return nullptr;
    pu_dsum* s = pu::new_set<pu_dsum>();
    if (!s) return nullptr;
    s->count = count;
    s->cores = num_cores != nullptr;

    // layout: summaries | num_cores | first core | per-core counts | per-core sums
    size_t cores = 0, tab = 0;
    if (s->cores) {
        s->nc.assign(num_cores, num_cores + count);
        s->core0.resize((size_t)count);
        for (int i = 0; i < count; i++) {
            s->core0[(size_t)i] = cores;
            cores += (size_t)num_cores[i];
            if (num_cores[i] <= kLdsCores && (size_t)num_cores[i] > tab) tab = (size_t)num_cores[i];
        }
    }
    s->lds_bytes = (size_t)kOffTab + 16 * tab;
    const size_t off_nc = round16((size_t)count * sizeof(pu_dsum_replica));
    const size_t off_c0 = off_nc + (s->cores ? round16((size_t)count * 4) : 0);
    const size_t off_cnt = off_c0 + (s->cores ? round16((size_t)count * 8) : 0);
    const size_t off_sum = off_cnt + round16(cores * 8);

    if (s->open(device, off_sum + round16(cores * 8), "pu_dsum_open: the summaries of " + std::to_string(count) +
                                                          " replicas (" + std::to_string(cores) + " cores)") != 0)
        return pu::drop_set(s);
    s->rep = (pu_dsum_replica*)s->base;
    if (s->cores) {
        s->d_nc = (int32_t*)(s->base + off_nc);
        s->d_core0 = (uint64_t*)(s->base + off_c0);
        s->g_cnt = (uint64_t*)(s->base + off_cnt);
        s->g_sum = (int64_t*)(s->base + off_sum);
        // from the set's own vectors, which live as long as the set
        if (hipMemcpyAsync(s->d_nc, s->nc.data(), (size_t)count * 4, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
            hipMemcpyAsync(s->d_core0, s->core0.data(), (size_t)count * 8, hipMemcpyHostToDevice, s->stream) != hipSuccess)
            return pu::drop_set(s, PU_EIO, "table layout upload failed");
    }
    if (launch_reset(s) != 0) return pu::drop_set(s);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dsum_close(pu_dsum* s) { pu::close_set(s); }

int pu_dsum_add(pu_dsum* s, const void* d_reqs, int fmt, const int32_t* d_delay, const uint64_t* d_begin,
                const uint64_t* d_end, void* hip_stream) {
    return delay_add(s, "pu_dsum_add", d_reqs, fmt, d_delay, d_begin, d_end, hip_stream, [&](auto F, hipStream_t st) {
        const auto kernel = s->cores ? dsum_add_kernel<decltype(F)::value, true> : dsum_add_kernel<decltype(F)::value, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)s->count), dim3(kThreads), s->lds_bytes, st, s->rep, s->d_nc, s->d_core0,
                           s->g_cnt, s->g_sum, d_reqs, d_delay, d_begin, d_end);
    });
}

int pu_dsum_read(pu_dsum* s, int first, int n, pu_dsum_replica* out) {
    const int rc = pu::replica_range(s ? s->count : 0, first, n, out != nullptr, "pu_dsum_read");
    if (rc) return rc < 0 ? rc : 0;
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpyAsync(out, s->rep + first, (size_t)n * sizeof(pu_dsum_replica), hipMemcpyDeviceToHost, st) ==
                   hipSuccess;
        },
        "reading the summaries failed");
}

int pu_dsum_read_cores(pu_dsum* s, int replica, uint64_t* count_out, int64_t* sum_out, size_t n) {
    if (!s || replica < 0) return pu::set_error(PU_EINVAL, "pu_dsum_read_cores: bad arguments");
    if (!s->cores) return pu::set_error(PU_EINVAL, "pu_dsum_read_cores: the set was opened without per-core tables");
    if (replica >= s->count) return pu::set_error(PU_ERANGE, "more replicas than the set holds");
    if (n > (size_t)s->nc[(size_t)replica]) return pu::set_error(PU_ERANGE, "more cores than the replica has");
    if (n == 0 || (!count_out && !sum_out)) return 0;
    const uint64_t c0 = s->core0[(size_t)replica];
    return s->read_back(
        [&](hipStream_t st) {
            return (!count_out || hipMemcpyAsync(count_out, s->g_cnt + c0, n * 8, hipMemcpyDeviceToHost, st) == hipSuccess) &&
                   (!sum_out || hipMemcpyAsync(sum_out, s->g_sum + c0, n * 8, hipMemcpyDeviceToHost, st) == hipSuccess);
        },
        "reading the per-core tables failed");
}

int pu_dsum_reset(pu_dsum* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dsum_reset: no set");
    int rc = s->use();
    return rc ? rc : launch_reset(s);   // on the set's own stream, after the set's last call
}

uint64_t pu_dsum_state_bytes(const pu_dsum* s) { return s ? (uint64_t)s->bytes : 0; }

void pu_dsum_host_init(pu_dsum_replica* acc) {
    if (acc) replica_init(acc);
}

int pu_dsum_host_add(pu_dsum_replica* acc, uint64_t* core_count, int64_t* core_sum, int num_cores, const void* reqs,
                     int fmt, const int32_t* delays, size_t n) {
    if (!acc || !pu::req_fmt_ok(fmt) || (n && (!reqs || !delays)) || !core_count != !core_sum || (core_count && num_cores < 1))
        return pu::set_error(PU_EINVAL, "pu_dsum_host_add: bad arguments");
    const uint32_t limit = core_limit(num_cores);
    for (size_t i = 0; i < n; i++) {
        const int32_t core = pu_delay_record::core_at(reqs, fmt, i);
        fold_one(&acc->cls[pu_delay_record::class_at(reqs, fmt, i)], delays[i]);
        if (core_out_of_range(core, limit)) {
            acc->core_out_of_range++;
        } else if (core_count) {
            core_count[core]++;
            core_sum[core] += delays[i];
        }
    }
    return 0;
}

}  // extern "C"
