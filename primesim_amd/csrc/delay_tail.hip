// delay_tail.hip — every replica's slowest requests on the device (pu_dtail_*,
// include/primeuncore.h): per replica and class a list of the k worst delays with
// the request each belongs to, a stage beside the delay summaries (delay_sum.hip)
// and histograms (delay_hist.hip) on the same stream.  Each pu_dtail_add offers
// every replica's records [d_begin[r], d_end[r]) of the request and delay arrays to
// its lists by the rule of delay_tail_step.h, which the host twin
// (pu_dtail_host_add, below) runs too.
//
// State, one allocation per set:
//   entries     pu_dtail_entry [count][2][k] (32 B each), best first, zero past the count
//   counts      uint32 [count][2]
//   seen        uint64 [count]
//   partials    the ensemble total's first pass: entries, replicas and counts of G <= kGroups lists
//   total       entries [2][k], replicas int32 [2][k], counts [2]
//
// dtail_add_kernel<FMT>: one launch per call, one workgroup of 256 per replica,
// which owns that replica's state for the launch; no atomics anywhere.
//   * The range and the loads are delay_stage.h's RecordSource, asked for the class
//     alone: 8 B of a record.
//   * Each wave keeps one sorted list per class in registers: lane j holds the j-th
//     best (delay, index in the range) of the records the wave has met.  A record is
//     a candidate while the wave's list is short, and once it holds k only when its
//     delay is strictly greater than the list's k-th: one comparison against a bar, which
//     rejects almost every record.  A stored list that is full sets the bar from the
//     start (its k-th delay): in a later chunk hardly a record passes.  A wave
//     instruction's candidates are found by ballot and inserted one at a time in
//     ascending lane order (WaveList::insert: a ballot of the lanes behind the candidate,
//     and a shift of those lanes by one, a DPP move per register).
//   * The tie argument.  A wave meets its records in ascending position: within a
//     wave instruction by lane, from one instruction of a trip to the next, from trip to
//     trip.  So a candidate's position is later than that of every entry already in the
//     wave's list, and among equal delays it is the worst.  Hence (a) it goes behind every
//     entry whose delay is not smaller (the first lane whose delay is strictly smaller, or
//     the first free lane), and (b) with the list full, a delay equal to the k-th's loses
//     to it on position: "not strictly greater than the k-th delay" rejects exactly the
//     records that are not among the wave's best k.
//   * At the end the four waves' lists and the replica's stored lists (whose positions
//     are all below `seen`, so earlier than any of this call) stand in LDS as five
//     sorted lists per class.  An item's rank in the union is its index in its own list
//     plus, by binary search, the number of better items in each of the other four;
//     positions are distinct, so the ranks are too.  Items of rank < k are the new list.
//     Only for those that are new in this call is the request read in full.
// dtail_total_kernel: a wave per class merges sorted lists given in ascending replica
// order into one, by the same insertion: first the replicas' lists of contiguous replica
// groups into partial lists (at most kGroups), then the partial lists into the total.
// Among equal delays the sources arrive by replica, then position, which is the total's order.
// Every loop is bounded by the range length or a constant.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/primeuncore.h"
#include "common.h"
#include "delay_stage.h"
#include "delay_tail_step.h"
#include "device_set.h"

using namespace pu_delay_tail;
using pu::round16;

namespace {

constexpr int kLists = kWaves + 1;         // the waves' lists and the stored one, per class
constexpr int kStored = kWaves;            // the stored list's place among them
constexpr int kMaxK = PU_DTAIL_MAX_K;
constexpr int kSearch = 7;                 // steps of a binary search over at most 64 entries
constexpr int kGroups = 120;               // replica groups of the total's first pass, at most
constexpr int kTotalThreads = 128;         // the total's workgroup: a wave per class

static_assert(kMaxK == 64, "lane j of a wave holds a list's j-th entry");
static_assert((1 << (kSearch - 1)) >= kMaxK, "the search reaches every entry");

// The value of the lane below (lane 0 keeps its own): one DPP move, a wave shift right by one.
__device__ inline int32_t from_lane_below(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ inline u64 from_lane_below(u64 v) {
    const uint32_t lo = (uint32_t)from_lane_below((int32_t)(uint32_t)v), hi = (uint32_t)from_lane_below((int32_t)(v >> 32));
    return (u64)hi << 32 | lo;
}

// A wave's sorted list: lane j < cnt holds the j-th best key (delay d, payload p); cnt, barred
// and bar are wave-uniform.  Once barred, only a delay above bar can still belong to the list.
struct WaveList {
    int32_t d = 0;
    u64 p = 0;
    int cnt = 0;
    bool barred = false;
    int32_t bar = 0;

    __device__ bool admits(int32_t dv) const { return !barred || dv > bar; }

    // Inserts (dv, pv), which admits() has passed and which among equal delays comes after
    // every key already in the list (the file header's tie argument): it goes to the first
    // lane that is free or holds a strictly smaller delay, the keys from there on move up one
    // lane and the one beyond lane k - 1 falls out.  Such a lane exists among the first k: a
    // free one while cnt < k, and a full list's k-th delay is at most bar, so below dv.
    __device__ void insert(int lane, int k, int32_t dv, u64 pv) {
        const int at = __ffsll(__ballot(lane >= cnt || dv > d)) - 1;
        const int32_t d_up = from_lane_below(d);
        const u64 p_up = from_lane_below(p);
        d = lane > at ? d_up : lane == at ? dv : d;
        p = lane > at ? p_up : lane == at ? pv : p;
        if (cnt < k) cnt++;
        if (cnt == k) {   // the list's k-th delay: nothing at or below it enters any more
            const int32_t kth = __builtin_amdgcn_readlane(d, k - 1);
            bar = barred && bar > kth ? bar : kth;
            barred = true;
        }
    }
};

template <int FMT>
__global__ __launch_bounds__(kThreads) void dtail_add_kernel(pu_dtail_entry* __restrict__ entries,
                                                              uint32_t* __restrict__ counts, u64* __restrict__ seen_of,
                                                              int k, const void* __restrict__ reqs,
                                                              const int32_t* __restrict__ delay,
                                                              const uint64_t* __restrict__ d_begin,
                                                              const uint64_t* __restrict__ d_end) {
    __shared__ int32_t s_d[kLists][2][kMaxK];
    __shared__ u64 s_p[kLists][2][kMaxK];
    __shared__ int s_cnt[kLists][2];
    __shared__ pu_dtail_entry s_old[2][kMaxK];

    const int r = (int)blockIdx.x;
    const RecordRange rg(d_begin, d_end);
    if (rg.empty()) return;
    const uint64_t len = rg.len();
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 seen = seen_of[r];
    const RecordSource<FMT, false> src(reqs, delay, rg.b, len);

    // this wave's lists: (delay, index in the range) per class.  A stored list that is full bars
    // from the start: its entries are earlier than any record of this call, so a record whose
    // delay is not above its k-th has k better entries already.
    WaveList mine[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if ((int)counts[r * 2 + c] == k) {
            mine[c].barred = true;
            mine[c].bar = entries[((size_t)r * 2 + c) * k + (k - 1)].delay;
        }
    }

    for (uint64_t base = 0; base < len; base += kTrip) {
        int32_t d[kUnroll];
        u64 w[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) valid[u] = src.load(base + (uint64_t)(u * kThreads + tid), d[u], w[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int cls = src.cls(w[u]);
            const uint64_t first = base + (uint64_t)(u * kThreads + wave * 64);   // lane 0's record
#pragma unroll
            for (int c = 0; c < 2; c++) {
                u64 cand = __ballot(valid[u] && cls == c && mine[c].admits(d[u]));
                for (int step = 0; step < 64 && cand; step++) {   // ascending lanes: ascending positions
                    const int l = __ffsll(cand) - 1;
                    cand &= cand - 1;
                    const int32_t dv = __builtin_amdgcn_readlane(d[u], l);
                    if (mine[c].admits(dv)) mine[c].insert(lane, k, dv, first + (uint64_t)l);   // the bar may have risen since the ballot
                }
            }
        }
    }

    // five sorted lists per class in LDS, positions absolute
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (lane < mine[c].cnt) {
            s_d[wave][c][lane] = mine[c].d;
            s_p[wave][c][lane] = seen + mine[c].p;
        }
        if (lane == 0) s_cnt[wave][c] = mine[c].cnt;
    }
    if (tid < 2 * 64) {   // waves 0 and 1: the stored list of class `wave`
        const int have = (int)counts[r * 2 + wave];
        if (lane < have) {
            const pu_dtail_entry old = entries[((size_t)r * 2 + wave) * k + lane];
            s_old[wave][lane] = old;
            s_d[kStored][wave][lane] = old.delay;
            s_p[kStored][wave][lane] = old.position;
        }
        if (lane == 0) s_cnt[kStored][wave] = have;
    }
    __syncthreads();   // the lists are complete, the stored entries are in LDS

    for (int item = tid; item < kLists * 2 * kMaxK; item += kThreads) {
        const int list = item / (2 * kMaxK), c = (item / kMaxK) & 1, j = item % kMaxK;
        if (j >= s_cnt[list][c]) continue;
        const int32_t dv = s_d[list][c][j];
        const u64 pv = s_p[list][c][j];
        int rank = j;
#pragma unroll
        for (int other = 0; other < kLists; other++) {
            if (other == list) continue;
            int lo = 0, hi = s_cnt[other][c];
#pragma unroll
            for (int step = 0; step < kSearch; step++) {
                if (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (better(s_d[other][c][mid], s_p[other][c][mid], dv, pv))
                        lo = mid + 1;
                    else
                        hi = mid;
                }
            }
            rank += lo;
        }
        if (rank >= k) continue;
        pu_dtail_entry* const out = entries + ((size_t)r * 2 + c) * k + rank;
        if (list == kStored) {
            *out = s_old[c][j];
        } else {   // new in this call: the request in full
            const uint64_t i = rg.b + (pv - seen);
            *out = FMT == PU_REQ_FMT_16 ? entry_of(((const pu_req16*)reqs)[i], dv, pv) : entry_of(((const pu_req*)reqs)[i], dv, pv);
        }
    }
    if (tid < 2) {
        int total = 0;
#pragma unroll
        for (int list = 0; list < kLists; list++) total += s_cnt[list][tid];
        counts[r * 2 + tid] = (uint32_t)(total < k ? total : k);
    }
    if (tid == 0) seen_of[r] = seen + len;
}

// Sources [s0, s1) of block blockIdx.x, s0 = first + blockIdx.x * per, s1 = min(s0 + per,
// first + n): sorted lists src[s][2][k] with counts src_cnt[s][2], taken in ascending s.
// Wave c of the workgroup merges class c into list blockIdx.x of out / out_rep / out_cnt:
// all k slots are written, zero and replica -1 past the count.  An entry's replica is its
// source (src_rep == NULL: the sources are the replicas) or what src_rep holds for it.
__global__ __launch_bounds__(kTotalThreads) void dtail_total_kernel(const pu_dtail_entry* __restrict__ src,
                                                                     const uint32_t* __restrict__ src_cnt,
                                                                     const int32_t* __restrict__ src_rep, int first, int n,
                                                                     int per, int k, pu_dtail_entry* __restrict__ out,
                                                                     int32_t* __restrict__ out_rep,
                                                                     uint32_t* __restrict__ out_cnt) {
    const int lane = (int)threadIdx.x & 63, c = (int)threadIdx.x >> 6;
    const int s0 = first + (int)blockIdx.x * per;
    const int s1 = s0 + per < first + n ? s0 + per : first + n;

    // lane j: the j-th best delay and where its entry is: source << 32 | slot
    WaveList best;
    for (int s = s0; s < s1; s++) {
        const size_t row = (size_t)s * 2 + (size_t)c;
        const int have = (int)src_cnt[row];
        const int32_t d = lane < have ? src[row * k + lane].delay : 0;
        // a source is sorted: its candidates are its first entries
        u64 cand = __ballot(lane < have && best.admits(d));
        for (int step = 0; step < 64 && cand; step++) {
            const int l = __ffsll(cand) - 1;
            cand &= cand - 1;
            const int32_t dv = __builtin_amdgcn_readlane(d, l);
            if (best.admits(dv)) best.insert(lane, k, dv, (u64)(uint32_t)s << 32 | (u64)l);
        }
    }

    const size_t to = ((size_t)blockIdx.x * 2 + (size_t)c) * k + lane;
    if (lane < best.cnt) {
        const int s = (int)(best.p >> 32), slot = (int)(best.p & 0xFFFFFFFFu);
        const size_t from = ((size_t)s * 2 + (size_t)c) * k + slot;
        out[to] = src[from];
        out_rep[to] = src_rep ? src_rep[from] : s;
    } else if (lane < k) {
        out[to] = pu_dtail_entry{};
        out_rep[to] = -1;
    }
    if (lane == 0) out_cnt[blockIdx.x * 2 + c] = (uint32_t)best.cnt;
}

}  // namespace

struct pu_dtail : pu::DeviceSet {
    int count = 0;
    int k = 0;
    size_t reset_words = 0;         // entries, counts and seen, in 8-byte words from base
    pu_dtail_entry* entries = nullptr;
    uint32_t* counts = nullptr;
    u64* seen = nullptr;
    pu_dtail_entry* part = nullptr; // the total's partial lists
    int32_t* part_rep = nullptr;
    uint32_t* part_cnt = nullptr;
    pu_dtail_entry* tot = nullptr;
    int32_t* tot_rep = nullptr;
    uint32_t* tot_cnt = nullptr;
};

extern "C" {

pu_dtail* pu_dtail_open(int count, int k, int device) {
    if (count < 1) {
        pu::set_error(PU_EINVAL, "pu_dtail_open: no replicas");
        return nullptr;
    }
    if (k < 1 || k > kMaxK) {
        pu::set_error(PU_EINVAL, "pu_dtail_open: a list holds between 1 and " + std::to_string(kMaxK) + " entries");
        return nullptr;
    }
    if (pu::device_check(device, "the device lists of the slowest requests have no CPU fallback; pu_dtail_host_add folds host arrays") != 0)
        return nullptr;
    pu_dtail* s = pu::new_set<pu_dtail>();
    if (!s) return nullptr;
    s->count = count;
    s->k = k;
    const size_t groups = (size_t)(count < kGroups ? count : kGroups);

    // layout: entries | counts | seen | partial entries, replicas, counts | total entries, replicas, counts
    const size_t list = (size_t)2 * k;
    const size_t off_cnt = round16((size_t)count * list * sizeof(pu_dtail_entry));
    const size_t off_seen = off_cnt + round16((size_t)count * 2 * 4);
    const size_t off_part = off_seen + round16((size_t)count * 8);
    const size_t off_prep = off_part + round16(groups * list * sizeof(pu_dtail_entry));
    const size_t off_pcnt = off_prep + round16(groups * list * 4);
    const size_t off_tot = off_pcnt + round16(groups * 2 * 4);
    const size_t off_trep = off_tot + round16(list * sizeof(pu_dtail_entry));
    const size_t off_tcnt = off_trep + round16(list * 4);
    if (s->open(device, off_tcnt + round16(2 * 4),
                "pu_dtail_open: the lists of " + std::to_string(count) + " replicas") != 0)
        return pu::drop_set(s);
    s->reset_words = off_part / 8;
    s->entries = (pu_dtail_entry*)s->base;
    s->counts = (uint32_t*)(s->base + off_cnt);
    s->seen = (u64*)(s->base + off_seen);
    s->part = (pu_dtail_entry*)(s->base + off_part);
    s->part_rep = (int32_t*)(s->base + off_prep);
    s->part_cnt = (uint32_t*)(s->base + off_pcnt);
    s->tot = (pu_dtail_entry*)(s->base + off_tot);
    s->tot_rep = (int32_t*)(s->base + off_trep);
    s->tot_cnt = (uint32_t*)(s->base + off_tcnt);
    if (hipMemsetAsync(s->base, 0, s->bytes, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dtail_close(pu_dtail* s) { pu::close_set(s); }

int pu_dtail_add(pu_dtail* s, const void* d_reqs, int fmt, const int32_t* d_delay, const uint64_t* d_begin,
                 const uint64_t* d_end, void* hip_stream) {
    return delay_add(s, "pu_dtail_add", d_reqs, fmt, d_delay, d_begin, d_end, hip_stream, [&](auto F, hipStream_t st) {
        hipLaunchKernelGGL((dtail_add_kernel<decltype(F)::value>), dim3((unsigned)s->count), dim3(kThreads), 0, st, s->entries,
                           s->counts, s->seen, s->k, d_reqs, d_delay, d_begin, d_end);
    });
}

int pu_dtail_read(pu_dtail* s, int first, int n, pu_dtail_entry* out, uint32_t* count_out) {
    const int rc = pu::replica_range(s ? s->count : 0, first, n, out && count_out, "pu_dtail_read");
    if (rc) return rc < 0 ? rc : 0;
    const size_t list = (size_t)2 * s->k;
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpyAsync(out, s->entries + (size_t)first * list, (size_t)n * list * sizeof(pu_dtail_entry),
                                  hipMemcpyDeviceToHost, st) == hipSuccess &&
                   hipMemcpyAsync(count_out, s->counts + (size_t)first * 2, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, st) ==
                       hipSuccess;
        },
        "reading the lists failed");
}

int pu_dtail_read_total(pu_dtail* s, int first, int n, pu_dtail_entry* out, int32_t* replica_out, uint32_t* count_out) {
    // n == 0 fills the outputs too: without them there is nothing to call, as without a set
    int rc = pu::replica_range(s && out && replica_out && count_out ? s->count : 0, first, n, true, "pu_dtail_read_total");
    if (rc < 0) return rc;
    const size_t list = (size_t)2 * s->k;
    if (rc) {
        std::memset(out, 0, list * sizeof(pu_dtail_entry));
        for (size_t i = 0; i < list; i++) replica_out[i] = -1;
        count_out[0] = count_out[1] = 0;
        return 0;
    }
    rc = s->use();
    if (rc) return rc;
    // on the set's own stream, after the set's last call by its event
    hipStream_t st = s->stream;
    rc = s->order_before(st);
    if (rc) return rc;
    // contiguous groups of `per` replicas, every one with a replica: G <= kGroups
    const int per = (n + kGroups - 1) / kGroups, G = (n + per - 1) / per;
    hipLaunchKernelGGL(dtail_total_kernel, dim3((unsigned)G), dim3(kTotalThreads), 0, st, s->entries, s->counts,
                       (const int32_t*)nullptr, first, n, per, s->k, s->part, s->part_rep, s->part_cnt);
    hipLaunchKernelGGL(dtail_total_kernel, dim3(1u), dim3(kTotalThreads), 0, st, s->part, s->part_cnt, s->part_rep, 0, G, G,
                       s->k, s->tot, s->tot_rep, s->tot_cnt);
    rc = s->record_after(st, "pu_dtail_read_total");
    if (rc) return rc;
    return s->read_back(
        [&](hipStream_t cs) {
            return hipMemcpyAsync(out, s->tot, list * sizeof(pu_dtail_entry), hipMemcpyDeviceToHost, cs) == hipSuccess &&
                   hipMemcpyAsync(replica_out, s->tot_rep, list * 4, hipMemcpyDeviceToHost, cs) == hipSuccess &&
                   hipMemcpyAsync(count_out, s->tot_cnt, 2 * 4, hipMemcpyDeviceToHost, cs) == hipSuccess;
        },
        "reading the total failed");
}

int pu_dtail_reset(pu_dtail* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dtail_reset: no set");
    return reset_words(s, s->base, s->reset_words, "pu_dtail_reset");
}

uint64_t pu_dtail_state_bytes(const pu_dtail* s) { return s ? (uint64_t)s->bytes : 0; }

int pu_dtail_k(const pu_dtail* s) { return s ? s->k : 0; }

int pu_dtail_host_add(pu_dtail_entry* entries, uint32_t* counts, uint64_t* seen, int k, const void* reqs, int fmt,
                      const int32_t* delays, size_t n) {
    if (!entries || !counts || !seen || k < 1 || k > kMaxK || !pu::req_fmt_ok(fmt) || (n && (!reqs || !delays)))
        return pu::set_error(PU_EINVAL, "pu_dtail_host_add: bad arguments");
    fold(entries, counts, seen, k, reqs, fmt, delays, n);
    return 0;
}

}  // extern "C"
