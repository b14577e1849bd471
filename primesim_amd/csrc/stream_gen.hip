// stream_gen.hip — the synthetic request streams generated on the device
// (pu_dstream_*, include/primeuncore.h): the first stage of a device-side
// ensemble.  A set of streams keeps its generator state in device memory and
// each pu_dstream_next writes the next chunk of every stream as pu_req or
// pu_req16 records, byte for byte what the host generator (stream.cpp)
// produces: both run the core's step of stream_step.h.
//
// State, one allocation per set:
//   headers   one DsHdr per stream: parameters, write percentage, the cursor
//             (quantum, core, requests in the open message, position), limit
//   per core  three arrays over all cores of all streams, a stream's cores
//             contiguous (lane = core loads and stores are contiguous):
//             rng state, cycle, streaming position -- 24 B per core
//   seeds     one word per stream: where pu_dstream_fork puts the new seeds
//   rings     for PU_STREAM_SHARED_UNIFORM streams only: the 16-entry re-use
//             ring as [16][cores] plus one word per core holding its two counters
//
// Kernel: one launch per call, one workgroup per stream, lanes are cores.  Per
// stream the workgroup walks groups of kThreads cores in canonical order from
// the cursor; a trip over one group
//   1. counts, per lane, the requests its core issues before the quantum's
//      barrier (one mix per request: only the gap draws matter), capped at what
//      the call still takes plus one;
//   2. scans the counts over the group (wave scan by __shfl_up, LDS across the
//      waves) and cuts at the first core whose inclusive sum exceeds what the
//      call still takes (stream_step.h: cut_take, cut_here, cursor_advance);
//   3. lets every lane with records to write replay its core from the saved
//      state through make_request, storing each record with 16-B vector
//      stores, and write its state back.
// A trip emits a record or advances the cursor's core (and with it, in the end,
// the quantum, bounded by num_quanta), so every loop is bounded.  A stream is
// owned by one workgroup and a set has one launch at a time: no atomics.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "device_set.h"
#include "stream_step.h"

using namespace pu_stream_step;
using pu::round16;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct DsHdr {
    pu_stream_params p;
    int32_t wpct;
    int32_t q, c, in_msg;  // the cursor (stream_step.h: Cursor)
    int64_t n;
    int64_t limit;
    uint64_t core0;     // the stream's first element in the per-core arrays
    uint64_t ring_off;  // byte offset of the stream's ring block in the allocation; 0: none
};
static_assert(sizeof(DsHdr) % 16 == 0, "headers stay 16-byte aligned");

// What make_request needs of a core; the ring stays in device memory (it is
// indexed at run time: a register array would go to scratch).
struct DevGen {
    SplitMix64 rng;
    uint64_t stream_pos;
    int n_recent, recent_head;
    uint64_t* ring;   // this core's column of the [16][cores] ring
    uint32_t cores;
    PU_HD uint64_t recent_get(uint64_t i) const { return ring[i * cores]; }
    PU_HD void recent_set(int i, uint64_t a) { ring[(uint64_t)i * cores] = a; }
};

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ size_t round16_dev(size_t v) { return (v + 15) & ~(size_t)15; }

template <int FMT>
__device__ __forceinline__ void store_record(void* out, size_t idx, uint64_t addr, int64_t timer, int core, int prog,
                                             uint8_t type, bool batch_start) {
    if (FMT == PU_REQ_FMT_16) {
        u64x2 v;
        v.x = addr;
        v.y = PU_REQ16_B(timer, core, prog, type, batch_start);
        ((u64x2*)out)[idx] = v;
    } else {   // pu_req: addr, timer | core, prog_id | mem_type, batch_start, tag = 0, _pad1 = 0
        u64x2 lo, hi;
        lo.x = addr;
        lo.y = (uint64_t)timer;
        hi.x = (uint64_t)(uint32_t)core | (uint64_t)(uint32_t)prog << 32;
        hi.y = (uint64_t)type | (uint64_t)batch_start << 8;
        u64x2* o = (u64x2*)out + 2 * idx;
        o[0] = lo;
        o[1] = hi;
    }
}

__global__ __launch_bounds__(kThreads) void dstream_init_kernel(const DsHdr* hdrs, uint8_t* base, uint64_t* rng,
                                                                 int64_t* cyc, uint64_t* spos) {
    const DsHdr* H = hdrs + blockIdx.x;
    const int cores = H->p.num_cores;
    const uint64_t seed = H->p.seed, core0 = H->core0, ring_off = H->ring_off;
    uint32_t* ctr = ring_off ? (uint32_t*)(base + ring_off + (size_t)16 * 8 * (size_t)cores) : nullptr;
    for (int k = (int)threadIdx.x; k < cores; k += kThreads) {
        rng[core0 + k] = seed_state(seed, k);
        cyc[core0 + k] = 0;
        spos[core0 + k] = 0;
        if (ctr) ctr[k] = 0;
    }
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void dstream_next_kernel(DsHdr* hdrs, uint8_t* base, uint64_t* rng, int64_t* cyc,
                                                                 uint64_t* spos, void* out, uint64_t n_each,
                                                                 uint64_t stride, uint64_t* d_got) {
    __shared__ uint64_t s_wsum[kWaves];
    __shared__ uint64_t s_cut_take;
    __shared__ int s_cut;

    DsHdr* H = hdrs + blockIdx.x;
    const pu_stream_params p = H->p;
    const int wpct = H->wpct;
    const int64_t limit = H->limit;
    const uint64_t ring_off = H->ring_off;
    uint64_t* const my_rng = rng + H->core0;
    int64_t* const my_cyc = cyc + H->core0;
    uint64_t* const my_spos = spos + H->core0;
    const bool uses_pos = p.kind == PU_STREAM_PRIVATE_STREAMING || p.kind == PU_STREAM_MULTIPROGRAM;
    const bool uses_ring = p.kind == PU_STREAM_SHARED_UNIFORM;
    Cursor cur{H->q, H->c, H->in_msg, H->n};   // every lane keeps the same copy

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)blockIdx.x * stride;
    uint64_t k = 0;   // records this call has written for the stream

    while (cur.q < p.num_quanta && cur.n < limit && k < n_each) {
        const uint64_t want = chunk_want(n_each, k, limit, cur.n);
        const int64_t barrier = (int64_t)(cur.q + 1) * p.quantum;
        const int left = p.num_cores - cur.c;
        const int group = left < kThreads ? left : kThreads;
        const int core = cur.c + tid;
        const bool live = tid < group;

        // 1. count
        uint64_t s = 0, cnt = 0;
        int64_t cycle = 0;
        if (live) {
            s = my_rng[core];
            cycle = my_cyc[core];
            cnt = count_before(s, cycle, barrier, want + 1);
        }

        // 2. scan and cut
        if (tid == 0) s_cut = -1;
        uint64_t incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint64_t woff = 0, total = 0;
        for (int w = 0; w < kWaves; w++) {
            uint64_t v = s_wsum[w];
            if (w < wave) woff += v;
            total += v;
        }
        const uint64_t excl = woff + incl - cnt;
        const uint64_t take = cut_take(excl, cnt, want);
        if (live && cut_here(excl, cnt, want)) {
            s_cut = tid;
            s_cut_take = take;
        }

        // 3. write
        if (take) {
            DevGen g;
            g.rng.s = s;
            g.stream_pos = uses_pos ? my_spos[core] : 0;
            g.n_recent = g.recent_head = 0;
            g.ring = nullptr;
            g.cores = (uint32_t)p.num_cores;
            uint32_t* ctr = nullptr;
            if (uses_ring) {
                g.ring = (uint64_t*)(base + ring_off) + core;
                ctr = (uint32_t*)(base + ring_off + (size_t)16 * 8 * (size_t)p.num_cores) + core;
                const uint32_t w = *ctr;
                g.n_recent = (int)(w & 0xFF);
                g.recent_head = (int)(w >> 8);
            }
            int im = start_in_msg(cur, tid);
            const int prog = prog_of(&p, core);
            const size_t o = row + k + excl;
            for (uint64_t j = 0; j < take; j++) {
                uint64_t a;
                uint8_t t;
                make_request(&p, core, g, wpct, &a, &t);
                store_record<FMT>(out, o + j, a, cycle, core, prog, t, im == 0);
                if (++im == p.max_msg) im = 0;
                cycle += gap_of(g.rng.next());
            }
            my_rng[core] = g.rng.s;
            my_cyc[core] = cycle;
            if (uses_pos) my_spos[core] = g.stream_pos;
            if (uses_ring) *ctr = (uint32_t)g.n_recent | (uint32_t)g.recent_head << 8;
        }
        __syncthreads();   // the cut is known; this trip's state is visible to the workgroup's later trips
        const int cut = s_cut;
        const uint64_t cut_taken = cut >= 0 ? s_cut_take : 0;
        const uint64_t written = total < want ? total : want;
        cursor_advance(cur, group, cut, cut_taken, written, p.num_cores, p.max_msg);
        k += written;
        __syncthreads();   // everyone has read s_cut and s_wsum before the next trip resets them
    }

    if (tid == 0) {
        H->q = cur.q;
        H->c = cur.c;
        H->in_msg = cur.in_msg;
        H->n = cur.n;
        if (d_got) d_got[blockIdx.x] = k;
    }
}

// pu_dstream_fork: one workgroup per destination first + blockIdx.x (the source
// itself leaves at once), lanes are cores.  The three per-core arrays go by
// contiguous loads and stores, the generator state through fork_rng; the ring
// block of a PU_STREAM_SHARED_UNIFORM stream (the same size in both: the host
// has compared the parameters) by 16-B pieces; one lane writes the header's
// cursor, limit and seed (stream_step.h: fork_cursor).  seeds: device memory,
// seeds[i] for stream first + i, or NULL for exact clones.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void dstream_fork_kernel(DsHdr* hdrs, uint8_t* base, uint64_t* rng, int64_t* cyc,
                                                                 uint64_t* spos, int src, int first,
                                                                 const uint64_t* seeds) {
    const int d = first + (int)blockIdx.x;
    if (d == src) return;
    const DsHdr* const S = hdrs + src;
    DsHdr* const D = hdrs + d;
    const int cores = S->p.num_cores;
    const uint64_t s0 = S->core0, d0 = D->core0, s_ring = S->ring_off, d_ring = D->ring_off;
    const bool reseed = seeds != nullptr;
    const uint64_t seed = reseed ? seeds[blockIdx.x] : 0;
    for (int k = (int)threadIdx.x; k < cores; k += kThreads) {
        rng[d0 + k] = fork_rng(rng[s0 + k], reseed, seed, k);
        cyc[d0 + k] = cyc[s0 + k];
        spos[d0 + k] = spos[s0 + k];
    }
    if (s_ring && d_ring) {
        const size_t pieces = round16_dev((size_t)cores * (16 * 8 + 4)) / 16;
        const u32x4* const from = (const u32x4*)(base + s_ring);
        u32x4* const to = (u32x4*)(base + d_ring);
        for (size_t k = threadIdx.x; k < pieces; k += kThreads) to[k] = from[k];
    }
    if (threadIdx.x == 0) fork_cursor(*D, *S, reseed, seed);
}

}  // namespace

struct pu_dstream : pu::DeviceSet {
    int count = 0;
    std::string refuse16;   // why the set has no format 16 ("" = every stream fits)
    std::vector<pu_stream_params> params;   // as the device headers hold them (a fork compares them on the host)
    uint64_t* d_seeds = nullptr;            // [count], in the set's allocation: a fork's seeds on the device
    uint64_t* h_seeds = nullptr;            // [count], pinned: what the last fork's copy reads
    bool seeds_in_flight = false;
    DsHdr* hdrs = nullptr;
    uint64_t* rng = nullptr;
    int64_t* cyc = nullptr;
    uint64_t* spos = nullptr;
};

extern "C" {

pu_dstream* pu_dstream_open(const pu_stream_params* params, int count, int device) {
    if (!params || count <= 0) {
        pu::set_error(PU_EINVAL, "pu_dstream_open: no streams");
        return nullptr;
    }
    for (int i = 0; i < count; i++)
        if (!params_ok(&params[i])) {
            pu::set_error(PU_EINVAL, "pu_dstream_open: invalid stream parameters (stream " + std::to_string(i) + ")");
            return nullptr;
        }
    if (pu::device_check(device, "the device generator has no CPU fallback") != 0) return nullptr;
    pu_dstream* s = pu::new_set<pu_dstream>();
    if (!s) return nullptr;
    s->count = count;

    // layout: headers | rng | cycle | streaming position | fork seeds | ring blocks
    std::vector<DsHdr> hdrs((size_t)count);
    size_t cores = 0;
    for (int i = 0; i < count; i++) {
        DsHdr& h = hdrs[(size_t)i];
        h = DsHdr{};
        h.p = params[i];
        h.wpct = h.p.write_pct >= 0 ? h.p.write_pct : default_write_pct(h.p.kind);
        h.limit = h.p.max_requests > 0 ? h.p.max_requests : INT64_MAX;
        h.core0 = cores;
        cores += (size_t)h.p.num_cores;
        if (s->refuse16.empty() && pu_stream_fits_req16(&params[i]) != 0)
            s->refuse16 = "stream " + std::to_string(i) + " does not fit pu_req16: " + pu_last_error();
    }
    const size_t off_rng = round16((size_t)count * sizeof(DsHdr));
    const size_t off_cyc = off_rng + round16(cores * 8);
    const size_t off_pos = off_cyc + round16(cores * 8);
    const size_t off_seeds = off_pos + round16(cores * 8);
    size_t bytes = off_seeds + round16((size_t)count * 8);
    for (DsHdr& h : hdrs)
        if (h.p.kind == PU_STREAM_SHARED_UNIFORM) {
            h.ring_off = bytes;
            bytes += round16((size_t)h.p.num_cores * (16 * 8 + 4));
        }

    if (s->open(device, bytes, "pu_dstream_open: the state of " + std::to_string(count) + " streams (" +
                                   std::to_string(cores) + " cores)") != 0)
        return pu::drop_set(s);
    s->hdrs = (DsHdr*)s->base;
    s->rng = (uint64_t*)(s->base + off_rng);
    s->cyc = (int64_t*)(s->base + off_cyc);
    s->spos = (uint64_t*)(s->base + off_pos);
    s->d_seeds = (uint64_t*)(s->base + off_seeds);
    s->params.assign(params, params + count);
    if (hipMemcpyAsync(s->hdrs, hdrs.data(), (size_t)count * sizeof(DsHdr), hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return pu::drop_set(s, PU_EIO, "header upload failed");
    hipLaunchKernelGGL(dstream_init_kernel, dim3((unsigned)count), dim3(kThreads), 0, s->stream, s->hdrs, s->base, s->rng,
                       s->cyc, s->spos);
    if (s->record_after(s->stream, "pu_dstream_open") != 0) return pu::drop_set(s);
    if (hipStreamSynchronize(s->stream) != hipSuccess)   // hdrs is a local
        return pu::drop_set(s, PU_EIO, "state initialisation failed");
    return s;
}

void pu_dstream_close(pu_dstream* s) {
    if (s && s->h_seeds) {
        (void)hipSetDevice(s->device);
        (void)s->wait_outstanding();
        (void)hipHostFree(s->h_seeds);
        s->h_seeds = nullptr;
    }
    pu::close_set(s);
}

int pu_dstream_fork(pu_dstream* s, int src, int first, int n, const uint64_t* seeds, void* hip_stream) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dstream_fork: no set");
    if (src < 0 || first < 0 || n < 0) return pu::set_error(PU_EINVAL, "pu_dstream_fork: negative argument");
    if (src >= s->count) return pu::set_error(PU_ERANGE, "pu_dstream_fork: source stream out of range");
    if ((int64_t)first + n > s->count) return pu::set_error(PU_ERANGE, "pu_dstream_fork: more streams than the set holds");
    for (int d = first; d < first + n; d++)
        if (d != src && !fork_params_match(s->params[(size_t)d], s->params[(size_t)src]))
            return pu::set_error(PU_EINVAL, "pu_dstream_fork: the parameters of stream " + std::to_string(d) +
                                                " differ from those of stream " + std::to_string(src) +
                                                " in more than the seed");
    if (n == 0 || (n == 1 && first == src)) return 0;
    int rc = s->use();
    if (rc) return rc;
    if (seeds) {   // through the set's pinned buffer: the copy below is asynchronous, the caller's array is not ours
        if (!s->h_seeds && hipHostMalloc((void**)&s->h_seeds, (size_t)s->count * 8, hipHostMallocDefault) != hipSuccess) {
            s->h_seeds = nullptr;
            (void)hipGetLastError();
            return pu::set_error(PU_ENOMEM, "pu_dstream_fork: no pinned memory for the seeds");
        }
        if (s->seeds_in_flight) {   // an earlier fork's copy may still read the buffer
            rc = s->wait_outstanding();
            if (rc) return rc;
            s->seeds_in_flight = false;
        }
        for (int i = 0; i < n; i++) s->h_seeds[i] = seeds[i];
    }
    hipStream_t st = s->pick(hip_stream);
    rc = s->order_before(st);
    if (rc) return rc;
    if (seeds) {
        if (hipMemcpyAsync(s->d_seeds, s->h_seeds, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess)
            return pu::set_error(PU_EIO, "pu_dstream_fork: seed upload failed");
        s->seeds_in_flight = true;
    }
    hipLaunchKernelGGL(dstream_fork_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, s->hdrs, s->base, s->rng, s->cyc,
                       s->spos, src, first, seeds ? (const uint64_t*)s->d_seeds : (const uint64_t*)nullptr);
    rc = s->record_after(st, "pu_dstream_fork");
    if (rc) return rc;
    for (int i = 0; i < n; i++)   // the seeds the device headers now hold
        if (first + i != src) s->params[(size_t)(first + i)].seed = seeds ? seeds[i] : s->params[(size_t)src].seed;
    return 0;
}

int pu_dstream_next(pu_dstream* s, void* d_out, size_t n_each, size_t stride, int fmt, uint64_t* d_got,
                    void* hip_stream) {
    if (!s || !pu::req_fmt_ok(fmt) || stride < n_each || (!d_out && n_each) || ((uintptr_t)d_out & 15))
        return pu::set_error(PU_EINVAL, "pu_dstream_next: bad arguments");
    if (fmt == PU_REQ_FMT_16 && !s->refuse16.empty()) return pu::set_error(PU_ERANGE, s->refuse16);
    int rc = s->use();
    if (rc) return rc;
    hipStream_t st = s->pick(hip_stream);
    rc = s->order_before(st);
    if (rc) return rc;
    if (fmt == PU_REQ_FMT_16)
        hipLaunchKernelGGL(dstream_next_kernel<PU_REQ_FMT_16>, dim3((unsigned)s->count), dim3(kThreads), 0, st, s->hdrs,
                           s->base, s->rng, s->cyc, s->spos, d_out, (uint64_t)n_each, (uint64_t)stride, d_got);
    else
        hipLaunchKernelGGL(dstream_next_kernel<PU_REQ_FMT_32>, dim3((unsigned)s->count), dim3(kThreads), 0, st, s->hdrs,
                           s->base, s->rng, s->cyc, s->spos, d_out, (uint64_t)n_each, (uint64_t)stride, d_got);
    return s->record_after(st, "pu_dstream_next");
}

int pu_dstream_positions(pu_dstream* s, int64_t* out, size_t n) {
    if (!s || (!out && n)) return pu::set_error(PU_EINVAL, "bad arguments");
    if (n > (size_t)s->count) return pu::set_error(PU_ERANGE, "more streams than the set holds");
    if (n == 0) return 0;
    return s->read_back(
        [&](hipStream_t st) {
            return hipMemcpy2DAsync(out, sizeof(int64_t), (const uint8_t*)s->hdrs + offsetof(DsHdr, n), sizeof(DsHdr),
                                    sizeof(int64_t), n, hipMemcpyDeviceToHost, st) == hipSuccess;
        },
        "reading the stream positions failed");
}

uint64_t pu_dstream_state_bytes(const pu_dstream* s) { return s ? (uint64_t)s->bytes : 0; }

}  // extern "C"
