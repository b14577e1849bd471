// run_results.hip — an ensemble's end-of-run results gathered on the device
// (pu_dres_*, include/primeuncore.h): the fourth stage of a device-side ensemble.
// One launch reads, for every replica of a range, the counters pu_stats_get
// forms, the fold of the per-core completion cycles, the run state and the visit
// counts of every link and bus queue, and writes one dense pu_dres_replica (and,
// for a set opened with PU_DRES_QUEUES, the replica's row of the per-queue map).
// The rules are in run_results_step.h, which the host gather below runs too.
//
// State, one allocation per set:
//   records     one pu_dres_replica per replica (448 B)
//   with the map: n [R][nqueues] and n1 [R][nqueues] (uint64), a replica's row contiguous
//   slabs       n and n1 [G][nqueues], the partial sums of the totals (G <= kGroups)
//   totals      n and n1 [nqueues]
//
// dres_gather_kernel<MAP>: one workgroup of 256 per replica, which owns that
// replica's record and map row; no atomics.
//   * Queues: lanes take consecutive queues, four per lane and trip (a trip's loads
//     are issued before any is used); of a 32-B header only piece a is loaded (one
//     16-B load).  Links and buses are two ranges of the same loop.  With MAP, n and
//     n1 go to the row by 8-B stores, 512 B contiguous per wave.
//   * Completion cycles: contiguous 8-B loads, four per lane and trip.
//   * Sums, the busiest queue and the used counts live in per-lane registers and
//     meet once: a wave reduction by __shfl_xor, then across the four waves
//     through LDS.
//   * Counters: EngineStats by 8-B loads of 43 lanes into LDS; for a verbose
//     configuration (Geo.cnt_sum == 0) also the per-cache {ins, miss, evict, wb} of
//     every level, the directory and the TLB, a cache per lane by 32-B loads.
//   * One lane assembles the record in LDS; 56 lanes store it, 8 B each.
// The geometry travels as kernel arguments (DresGeo): nothing is compiled per
// configuration.
//
// Totals (dres_totals_partial_kernel<MAP>, dres_totals_sum_kernel): store and
// sum instead of atomics.  Workgroups over (256-queue tile x replica group) each
// sum their group's replicas per queue, from the map or else from the headers,
// into a slab row; the second pass adds the G slab rows.  Integer, so exact.
// Every loop is bounded by a count of the geometry or a constant.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "device_set.h"
#include "geometry.h"
#include "handle.h"
#include "run_results_step.h"
#include "stats_rule.h"

using namespace pu_run_results;
using pu::round16;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;          // queues / cores / replicas per lane and trip
constexpr int kTabs = pu::kStatRows;   // EngineStats.lvl_cnt rows: levels 0-3, PU_CNT_DIR, PU_CNT_TLB
constexpr int kEsWords = (int)(sizeof(EngineStats) / 8);
constexpr int kRecWords = (int)(sizeof(pu_dres_replica) / 8);
constexpr int kGroups = 120;        // replica groups of the totals' first pass, at most

static_assert(sizeof(pu_dres_replica) == 448 && sizeof(pu_dres_replica) % 8 == 0, "the record is 56 words, no padding");
static_assert(sizeof(EngineStats) == 43 * 8, "EngineStats is 43 words");
static_assert(kEsWords <= kThreads && kRecWords <= kThreads, "one lane per word");
static_assert(PU_HDR_BYTES == kHdrBytes, "the header restated in run_results_step.h");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long __attribute__((may_alias)) u64a;

// One table of per-cache counters (32 B per cache), added to lvl_cnt row `row`.
struct DresTab {
    uint64_t off_cnt;
    int32_t ncaches, row;
};
// What the kernels need of Geo.
struct DresGeo {
    uint64_t replica_bytes, off_qhdr, off_completion, off_stats, off_run;
    int32_t nlinks, nqueues, num_cores, num_levels;
    int32_t ntabs, _pad;            // tables to sum: 0 unless Geo.cnt_sum == 0
    DresTab tab[kTabs];
};

// what a wave leaves for the combine across waves
struct WavePart {
    unsigned long long link_n, link_n1, bus_n;
    Busiest link_max, bus_max;
    Completion comp;
    int32_t links_used, buses_used;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ Busiest wave_busiest(Busiest b) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long v = __shfl_xor((unsigned long long)b.visits, m, 64);
        const int32_t id = __shfl_xor(b.id, m, 64);
        busiest_take(b, v, id);
    }
    return b;
}

template <bool MAP>
__global__ __launch_bounds__(kThreads) void dres_gather_kernel(const char* __restrict__ arena, const DresGeo g, int first,
                                                                pu_dres_replica* __restrict__ rec,
                                                                uint64_t* __restrict__ map_n, uint64_t* __restrict__ map_n1) {
    __shared__ WavePart s_part[kWaves];
    __shared__ EngineStats s_es;
    __shared__ unsigned long long s_tab[kTabs][kWaves][4];
    __shared__ uint64_t s_lv[kTabs][4];
    __shared__ pu_dres_replica s_rec;

    const int r = first + (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const char* const base = arena + (size_t)r * g.replica_bytes;
    const int nq = g.nqueues, nl = g.nlinks, nc = g.num_cores;

    if (tid < kEsWords) ((u64a*)&s_es)[tid] = ((const u64a*)(base + g.off_stats))[tid];

    // ---- the queues: links [0, nl), buses [nl, nq)
    unsigned long long link_n = 0, link_n1 = 0, bus_n = 0;
    int32_t links_used = 0, buses_used = 0;
    Busiest link_max = busiest_init(), bus_max = busiest_init();
    const u32x4* const hdr = (const u32x4*)(base + g.off_qhdr);   // piece a of queue q is hdr[2 * q]
    uint64_t* const row_n = MAP ? map_n + (size_t)r * (size_t)nq : nullptr;
    uint64_t* const row_n1 = MAP ? map_n1 + (size_t)r * (size_t)nq : nullptr;
    for (int q0 = 0; q0 < nq; q0 += kThreads * kUnroll) {
        u32x4 a[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int q = q0 + u * kThreads + tid;
            a[u] = u32x4{0u, 0u, 0u, 0u};
            if (q < nq) a[u] = hdr[2 * (size_t)q];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int q = q0 + u * kThreads + tid;
            if (q < nq) {
                const bool link = q < nl;
                const uint64_t n = count_of(a[u].x, a[u].y);
                const uint64_t n1 = link ? count_of(a[u].z, a[u].w) : 0;   // a bus carries one packet length
                if (MAP) {
                    row_n[q] = n;
                    row_n1[q] = n1;
                }
                if (link) {
                    link_n += n;
                    link_n1 += n1;
                    links_used += n ? 1 : 0;
                    busiest_take(link_max, n, q);
                } else {
                    bus_n += n;
                    buses_used += n ? 1 : 0;
                    busiest_take(bus_max, n, q);
                }
            }
        }
    }

    // ---- the completion cycles
    Completion comp = completion_init();
    const int64_t* const cyc = (const int64_t*)(base + g.off_completion);
    for (int k0 = 0; k0 < nc; k0 += kThreads * kUnroll) {
        int64_t c[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int k = k0 + u * kThreads + tid;
            c[u] = kNoCycle;
            if (k < nc) c[u] = cyc[k];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) completion_fold(comp, c[u]);
    }

    // ---- the per-cache counters of a verbose configuration: a cache per lane
    for (int t = 0; t < g.ntabs; t++) {
        const u64x4* const cnt = (const u64x4*)(base + g.tab[t].off_cnt);
        const int ncaches = g.tab[t].ncaches;
        u64x4 s = u64x4{0, 0, 0, 0};
        for (int k = tid; k < ncaches; k += kThreads) s += cnt[k];
        s.x = wave_sum(s.x);
        s.y = wave_sum(s.y);
        s.z = wave_sum(s.z);
        s.w = wave_sum(s.w);
        if (lane == 0) {
            s_tab[t][wave][0] = s.x;
            s_tab[t][wave][1] = s.y;
            s_tab[t][wave][2] = s.z;
            s_tab[t][wave][3] = s.w;
        }
    }

    // ---- the wave's registers meet
    link_n = wave_sum(link_n);
    link_n1 = wave_sum(link_n1);
    bus_n = wave_sum(bus_n);
    links_used = wave_sum(links_used);
    buses_used = wave_sum(buses_used);
    link_max = wave_busiest(link_max);
    bus_max = wave_busiest(bus_max);
    comp.done = wave_sum(comp.done);
    comp.sum = (int64_t)wave_sum((unsigned long long)comp.sum);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const long long mx = __shfl_xor((long long)comp.max, m, 64), mn = __shfl_xor((long long)comp.min, m, 64);
        comp.max = mx > comp.max ? mx : comp.max;
        comp.min = mn < comp.min ? mn : comp.min;
    }
    if (lane == 0) {
        WavePart& p = s_part[wave];
        p.link_n = link_n;
        p.link_n1 = link_n1;
        p.bus_n = bus_n;
        p.link_max = link_max;
        p.bus_max = bus_max;
        p.comp = comp;
        p.links_used = links_used;
        p.buses_used = buses_used;
    }
    __syncthreads();   // the partials, the tables' partials and EngineStats are in LDS

    // lvl_cnt plus, for the tables summed above, the per-cache counters (pu_stats_get, report.cpp):
    // lane = row * 4 + counter
    if (tid < kTabs * 4) {
        const int k = tid >> 2, j = tid & 3;
        unsigned long long v = s_es.lvl_cnt[k][j];
        for (int t = 0; t < g.ntabs; t++)
            if (g.tab[t].row == k)
                for (int w = 0; w < kWaves; w++) v += s_tab[t][w][j];
        s_lv[k][j] = v;
    }
    __syncthreads();

    if (tid == 0) {
        pu_dres_replica& o = s_rec;
        pu::stats_fill(o.stats, s_es, g.num_levels, s_lv);

        const RunState* const run = (const RunState*)(base + g.off_run);
        o.processed = run->processed;
        o.halted = run->halted;

        WavePart a = s_part[0];
        for (int w = 1; w < kWaves; w++) {
            const WavePart& p = s_part[w];
            a.link_n += p.link_n;
            a.link_n1 += p.link_n1;
            a.bus_n += p.bus_n;
            a.links_used += p.links_used;
            a.buses_used += p.buses_used;
            busiest_take(a.link_max, p.link_max.visits, p.link_max.id);
            busiest_take(a.bus_max, p.bus_max.visits, p.bus_max.id);
            completion_merge(a.comp, p.comp);
        }
        o.cores_done = a.comp.done;
        o.completion_max = a.comp.max;
        o.completion_min = a.comp.min;
        o.completion_sum = a.comp.sum;
        o.link_visits = a.link_n;
        o.link_block_visits = a.link_n1;
        o.link_max_visits = a.link_max.visits;
        o.link_max_id = a.link_max.id;
        o.links_used = a.links_used;
        o.bus_visits = a.bus_n;
        o.bus_max_visits = a.bus_max.visits;
        o.bus_max_id = a.bus_max.id;
        o.buses_used = a.buses_used;
    }
    __syncthreads();
    if (tid < kRecWords) ((u64a*)(rec + r))[tid] = ((const u64a*)&s_rec)[tid];
}

// Per queue, the sum over the group's replicas first + grp, first + grp + G, ...
// (< first + n) into slab row grp.  G <= n, so every group has a replica.
template <bool MAP>
__global__ __launch_bounds__(kThreads) void dres_totals_partial_kernel(const char* __restrict__ arena, const DresGeo g,
                                                                        int first, int n, int G,
                                                                        const uint64_t* __restrict__ map_n,
                                                                        const uint64_t* __restrict__ map_n1,
                                                                        uint64_t* __restrict__ slab_n,
                                                                        uint64_t* __restrict__ slab_n1) {
    const int q = (int)blockIdx.x * kThreads + (int)threadIdx.x, grp = (int)blockIdx.y;
    const int nq = g.nqueues;
    if (q >= nq) return;
    const bool link = q < g.nlinks;
    const int end = first + n;
    unsigned long long sn = 0, sn1 = 0;
    for (int r0 = first + grp; r0 < end; r0 += G * kUnroll) {
        if (MAP) {
            uint64_t vn[kUnroll], vn1[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int r = r0 + u * G;
                vn[u] = vn1[u] = 0;
                if (r < end) {
                    vn[u] = map_n[(size_t)r * (size_t)nq + (size_t)q];
                    vn1[u] = map_n1[(size_t)r * (size_t)nq + (size_t)q];
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                sn += vn[u];
                sn1 += vn1[u];
            }
        } else {
            u32x4 a[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int r = r0 + u * G;
                a[u] = u32x4{0u, 0u, 0u, 0u};   // decodes to n = n1 = 0
                if (r < end) a[u] = ((const u32x4*)(arena + (size_t)r * g.replica_bytes + g.off_qhdr))[2 * (size_t)q];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                sn += count_of(a[u].x, a[u].y);
                sn1 += link ? count_of(a[u].z, a[u].w) : 0;
            }
        }
    }
    slab_n[(size_t)grp * (size_t)nq + (size_t)q] = sn;
    slab_n1[(size_t)grp * (size_t)nq + (size_t)q] = sn1;
}

__global__ __launch_bounds__(kThreads) void dres_totals_sum_kernel(const uint64_t* __restrict__ slab_n,
                                                                    const uint64_t* __restrict__ slab_n1, int G, int nq,
                                                                    uint64_t* __restrict__ tot_n,
                                                                    uint64_t* __restrict__ tot_n1) {
    const int q = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (q >= nq) return;
    unsigned long long sn = 0, sn1 = 0;
    for (int k = 0; k < G; k++) {
        sn += slab_n[(size_t)k * (size_t)nq + (size_t)q];
        sn1 += slab_n1[(size_t)k * (size_t)nq + (size_t)q];
    }
    tot_n[q] = sn;
    tot_n1[q] = sn1;
}

DresGeo dres_geo(const Geo& g) {
    DresGeo d;
    std::memset(&d, 0, sizeof d);
    d.replica_bytes = g.replica_bytes;
    d.off_qhdr = g.off_qhdr;
    d.off_completion = g.off_completion;
    d.off_stats = g.off_stats;
    d.off_run = g.off_run;
    d.nlinks = g.nlinks;
    d.nqueues = g.nqueues;
    d.num_cores = g.num_cores;
    d.num_levels = g.num_levels;
    if (!g.cnt_sum) {   // the tables pu_stats_get adds (report.cpp: read_replica)
        for (int l = 0; l < g.num_levels; l++) d.tab[d.ntabs++] = DresTab{g.lv[l].off_cnt, g.lv[l].ncaches, l};
        d.tab[d.ntabs++] = DresTab{g.dir.off_cnt, g.N, PU_CNT_DIR};
        if (g.tlb_enable) d.tab[d.ntabs++] = DresTab{g.tlb.off_cnt, g.num_cores, PU_CNT_TLB};
    }
    return d;
}

}  // namespace

struct pu_dres : pu::DeviceSet {
    pu_handle* h = nullptr;
    DresGeo g{};
    bool map = false;
    int groups = 1;                 // slab rows allocated
    int last_first = 0, last_n = 0; // the range of the last gather
    pu_dres_replica* rec = nullptr;
    uint64_t *map_n = nullptr, *map_n1 = nullptr;
    uint64_t *slab_n = nullptr, *slab_n1 = nullptr;
    uint64_t *tot_n = nullptr, *tot_n1 = nullptr;
};

extern "C" {

pu_dres* pu_dres_open(pu_handle* h, int flags) {
    if (flags & ~PU_DRES_QUEUES) {
        pu::set_error(PU_EINVAL, "pu_dres_open: unknown flags");
        return nullptr;
    }
    if (!h) {
        pu::set_error(PU_EINVAL, "pu_dres_open: no handle (the results are gathered from a handle's replicas on its GPU)");
        return nullptr;
    }
    if (pu::device_check(h->device, "the device gather has no CPU fallback") != 0) return nullptr;
    pu_dres* s = pu::new_set<pu_dres>();
    if (!s) return nullptr;
    s->h = h;
    s->g = dres_geo(h->geo);
    s->map = (flags & PU_DRES_QUEUES) != 0;
    s->groups = h->R < kGroups ? h->R : kGroups;

    // layout: records | map n | map n1 | slab n | slab n1 | totals n | totals n1
    const size_t R = (size_t)h->R, nq = (size_t)s->g.nqueues;
    const size_t map_b = s->map ? round16(R * nq * 8) : 0, slab_b = round16((size_t)s->groups * nq * 8), tot_b = round16(nq * 8);
    const size_t off_map = round16(R * sizeof(pu_dres_replica));
    const size_t off_slab = off_map + 2 * map_b, off_tot = off_slab + 2 * slab_b;
    if (s->open(h->device, off_tot + 2 * tot_b, "pu_dres_open: the results of " + std::to_string(h->R) + " replicas (" +
                                                  std::to_string(nq) + " queues each" + (s->map ? ", with the map)" : ")")) != 0)
        return pu::drop_set(s);
    s->rec = (pu_dres_replica*)s->base;
    if (s->map) {
        s->map_n = (uint64_t*)(s->base + off_map);
        s->map_n1 = (uint64_t*)(s->base + off_map + map_b);
    }
    s->slab_n = (uint64_t*)(s->base + off_slab);
    s->slab_n1 = (uint64_t*)(s->base + off_slab + slab_b);
    s->tot_n = (uint64_t*)(s->base + off_tot);
    s->tot_n1 = (uint64_t*)(s->base + off_tot + tot_b);
    // records, map and totals read as zero until a gather has written them
    if (hipMemsetAsync(s->base, 0, s->bytes, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dres_close(pu_dres* s) { pu::close_set(s); }

int pu_dres_gather(pu_dres* s, int first, int n, void* hip_stream) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dres_gather: no set");
    if (first < 0 || n < 0) return pu::set_error(PU_EINVAL, "pu_dres_gather: bad arguments");
    if ((int64_t)first + n > s->h->R) return pu::set_error(PU_ERANGE, "more replicas than the handle holds");
    int rc = s->use();
    if (rc) return rc;
    if (n == 0) {   // nothing to launch: the totals of this gather are all zero
        s->last_first = first;
        s->last_n = 0;
        return 0;
    }
    std::lock_guard<std::mutex> lk(s->h->mu);   // as gather_error_flags: the headers leave the chip first
    rc = pu::resident_stop(s->h);
    if (rc) return rc;
    hipStream_t st = s->pick(hip_stream);
    rc = s->order_before(st);
    if (rc) return rc;
    if (s->map)
        hipLaunchKernelGGL((dres_gather_kernel<true>), dim3((unsigned)n), dim3(kThreads), 0, st, s->h->arena, s->g, first,
                           s->rec, s->map_n, s->map_n1);
    else
        hipLaunchKernelGGL((dres_gather_kernel<false>), dim3((unsigned)n), dim3(kThreads), 0, st, s->h->arena, s->g, first,
                           s->rec, (uint64_t*)nullptr, (uint64_t*)nullptr);
    rc = s->record_after(st, "pu_dres_gather");
    if (rc) return rc;
    s->last_first = first;   // what the totals refer to: only a gather that was launched
    s->last_n = n;
    return 0;
}

int pu_dres_read(pu_dres* s, int first, int n, pu_dres_replica* out) {
    if (!s || first < 0 || n < 0 || (!out && n)) return pu::set_error(PU_EINVAL, "pu_dres_read: bad arguments");
    if ((int64_t)first + n > s->h->R) return pu::set_error(PU_ERANGE, "more replicas than the handle holds");
    if (n == 0) return 0;
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpyAsync(out, s->rec + first, (size_t)n * sizeof(pu_dres_replica), hipMemcpyDeviceToHost, st) ==
                   hipSuccess;
        },
        "reading the records failed");
}

int pu_dres_read_queues(pu_dres* s, int replica, uint64_t* n_out, uint64_t* n1_out, size_t cap) {
    if (!s || replica < 0) return pu::set_error(PU_EINVAL, "pu_dres_read_queues: bad arguments");
    if (!s->map) return pu::set_error(PU_ENOTSUP, "pu_dres_read_queues: the set was opened without PU_DRES_QUEUES");
    if (replica >= s->h->R) return pu::set_error(PU_ERANGE, "more replicas than the handle holds");
    const size_t nq = (size_t)s->g.nqueues;
    if (cap < nq) return pu::set_error(PU_ERANGE, "pu_dres_read_queues: room for fewer queues than a replica has");
    if (nq == 0 || (!n_out && !n1_out)) return 0;
    const size_t at = (size_t)replica * nq;
    return s->read_back(
        [&](hipStream_t st) {
            return (!n_out || hipMemcpyAsync(n_out, s->map_n + at, nq * 8, hipMemcpyDeviceToHost, st) == hipSuccess) &&
                   (!n1_out || hipMemcpyAsync(n1_out, s->map_n1 + at, nq * 8, hipMemcpyDeviceToHost, st) == hipSuccess);
        },
        "reading the per-queue map failed");
}

int pu_dres_read_queue_totals(pu_dres* s, uint64_t* n_out, uint64_t* n1_out, size_t cap) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dres_read_queue_totals: no set");
    const int nq = s->g.nqueues;
    if (cap < (size_t)nq) return pu::set_error(PU_ERANGE, "pu_dres_read_queue_totals: room for fewer queues than a replica has");
    if (nq == 0 || (!n_out && !n1_out)) return 0;
    int rc = s->use();
    if (rc) return rc;
    if (s->last_n == 0) {
        if (n_out) std::memset(n_out, 0, (size_t)nq * 8);
        if (n1_out) std::memset(n1_out, 0, (size_t)nq * 8);
        return 0;
    }
    if (!s->map) {   // from the headers as they are now
        rc = pu::resident_quiesce(s->h);
        if (rc) return rc;
    }
    // on the set's own stream, after the last gather by the set's event (and so after whatever the
    // gather's stream ordered before it): no stream of a caller is used after the call it was given to
    hipStream_t st = s->stream;
    rc = s->order_before(st);
    if (rc) return rc;
    const int G = s->last_n < s->groups ? s->last_n : s->groups;
    const unsigned tiles = (unsigned)((nq + kThreads - 1) / kThreads);
    if (s->map)
        hipLaunchKernelGGL((dres_totals_partial_kernel<true>), dim3(tiles, (unsigned)G), dim3(kThreads), 0, st, s->h->arena,
                           s->g, s->last_first, s->last_n, G, s->map_n, s->map_n1, s->slab_n, s->slab_n1);
    else
        hipLaunchKernelGGL((dres_totals_partial_kernel<false>), dim3(tiles, (unsigned)G), dim3(kThreads), 0, st, s->h->arena,
                           s->g, s->last_first, s->last_n, G, (const uint64_t*)nullptr, (const uint64_t*)nullptr, s->slab_n,
                           s->slab_n1);
    hipLaunchKernelGGL(dres_totals_sum_kernel, dim3(tiles), dim3(kThreads), 0, st, s->slab_n, s->slab_n1, G, nq, s->tot_n,
                       s->tot_n1);
    rc = s->record_after(st, "pu_dres_read_queue_totals");
    if (rc) return rc;
    return s->read_back(
        [&](hipStream_t cs) {
            return (!n_out || hipMemcpyAsync(n_out, s->tot_n, (size_t)nq * 8, hipMemcpyDeviceToHost, cs) == hipSuccess) &&
                   (!n1_out || hipMemcpyAsync(n1_out, s->tot_n1, (size_t)nq * 8, hipMemcpyDeviceToHost, cs) == hipSuccess);
        },
        "reading the per-queue totals failed");
}

int pu_num_links(const pu_handle* h) { return h ? h->geo.nlinks : 0; }
int pu_num_queues(const pu_handle* h) { return h ? h->geo.nqueues : 0; }
int pu_dres_nqueues(const pu_dres* s) { return s ? s->g.nqueues : 0; }
uint64_t pu_dres_state_bytes(const pu_dres* s) { return s ? (uint64_t)s->bytes : 0; }

int pu_dres_host_gather(pu_handle* h, int replica, pu_dres_replica* out, uint64_t* n_out, uint64_t* n1_out, size_t cap) {
    if (!h || !out) return pu::set_error(PU_EINVAL, "pu_dres_host_gather: bad arguments");
    const Geo& g = h->geo;
    if (replica < 0 || replica >= h->R) return pu::set_error(PU_ERANGE, "replica out of range");
    const size_t nq = (size_t)g.nqueues, nc = (size_t)g.num_cores;
    if ((n_out || n1_out) && cap < nq)
        return pu::set_error(PU_ERANGE, "pu_dres_host_gather: room for fewer queues than a replica has");
    std::memset(out, 0, sizeof *out);
    int rc = pu_stats_get(h, replica, &out->stats);   // joins a resident kernel and waits for the handle's stream
    if (rc) return rc;
    const char* const base = h->arena + (size_t)replica * g.replica_bytes;
    std::vector<int64_t> cyc(nc);
    std::vector<uint32_t> hdr(nq * (kHdrBytes / 4));
    RunState run;
    if (hipMemcpy(cyc.data(), base + g.off_completion, nc * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&run, base + g.off_run, sizeof run, hipMemcpyDeviceToHost) != hipSuccess ||
        (nq && hipMemcpy(hdr.data(), base + g.off_qhdr, nq * kHdrBytes, hipMemcpyDeviceToHost) != hipSuccess))
        return pu::set_error(PU_EIO, "pu_dres_host_gather: copying the replica's state failed");
    out->processed = run.processed;
    out->halted = run.halted;
    Completion c = completion_init();
    for (size_t k = 0; k < nc; k++) completion_fold(c, cyc[k]);
    out->cores_done = c.done;
    out->completion_max = c.max;
    out->completion_min = c.min;
    out->completion_sum = c.sum;
    Busiest lm = busiest_init(), bm = busiest_init();
    for (size_t q = 0; q < nq; q++) {
        const uint32_t* a = &hdr[q * (kHdrBytes / 4)];
        const bool link = (int)q < g.nlinks;
        const uint64_t n = count_of(a[0], a[1]);
        const uint64_t n1 = link ? count_of(a[2], a[3]) : 0;
        if (n_out) n_out[q] = n;
        if (n1_out) n1_out[q] = n1;
        if (link) {
            out->link_visits += n;
            out->link_block_visits += n1;
            out->links_used += n ? 1 : 0;
            busiest_take(lm, n, (int32_t)q);
        } else {
            out->bus_visits += n;
            out->buses_used += n ? 1 : 0;
            busiest_take(bm, n, (int32_t)q);
        }
    }
    out->link_max_visits = lm.visits;
    out->link_max_id = lm.id;
    out->bus_max_visits = bm.visits;
    out->bus_max_id = bm.id;
    return 0;
}

}  // extern "C"
