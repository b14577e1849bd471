// trace_place.hip — one recorded trace replayed across an ensemble, placed per
// replica on the device (pu_dtrace_*, include/primeuncore.h): the recorded-trace
// counterpart of stream_gen.hip.  The trace (pu_req records, cores already
// resolved) sits in device memory once; every pu_dtrace_next writes the next
// chunk of it into every replica's window, each under that replica's thread
// placement and start skew, as pu_req or pu_req16 records, byte for byte what
// the host twin (pu_trace_place) gives: both run the step of trace_place_step.h.
//
// State, one allocation per set:
//   trace       n pu_req records, shared by all replicas
//   placement   int32[count][num_cores], where the set has one
//   skew        int32[count][num_cores], where the set has one
// The cursor is one position for the whole set and lives on the host: what a
// call writes follows from its arguments alone.
//
// dtrace_place_kernel<FMT, STAGED>: workgroups of 256, one per (replica, tile of
// 1,024 consecutive records), folded into a linear index.  Lane l takes records
// tile_begin + l, + 256, ...: a wave's 64 lanes store 64 consecutive records.
// A lane loads its source records first (two 16-B loads each, all issued before
// any is used; the trace is read by every replica, so after the first from L2 /
// the Infinity Cache), then
//   STAGED   the workgroup copies its replica's two rows into LDS once and the
//            lanes look up place[core] and skew[core] there (rows up to
//            kStageCapBytes, trace_place_step.h);
//   gathered the lanes read the rows in global memory (wider configurations,
//            and sets without rows: nothing to look up),
// and stores each record with one (pu_req16) or two (pu_req) 16-B stores.  All
// output addressing is 64-bit.  No atomics, no loop that depends on data.
// Which of the two is launched where the rows fit is decided by measurement
// (gathered), and PRIMEUNCORE_TRACE_ROWS = lds | global overrides
// it for that measurement (tools/trace_place_bench.py) and for the tests; lds is
// honoured only where the rows fit.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/primeuncore.h"
#include "common.h"
#include "device_set.h"
#include "trace_place_step.h"

using namespace pu_trace_step;
using pu::round16;

namespace {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
static_assert(sizeof(pu_req) == 2 * sizeof(u64x2), "a pu_req is one 16-B load pair");

template <int FMT, bool STAGED>
__global__ __launch_bounds__(kLanes) __attribute__((amdgpu_waves_per_eu(8))) void dtrace_place_kernel(const u64x2* __restrict__ src, const int32_t* __restrict__ place,
                                                              const int32_t* __restrict__ skew, int num_cores,
                                                              u64x2* __restrict__ out, uint64_t got, uint64_t stride,
                                                              uint64_t tiles, uint64_t wg_base, uint64_t* d_got) {
    extern __shared__ __attribute__((aligned(16))) int32_t s_rows[];   // STAGED: placement row | skew row

    const uint64_t wg = wg_base + blockIdx.x;
    const uint64_t replica = wg_replica(wg, tiles), tile = wg_tile(wg, tiles);
    const int lane = (int)threadIdx.x;
    const int32_t* const prow = place ? place + replica * (uint64_t)num_cores : nullptr;
    const int32_t* const srow = skew ? skew + replica * (uint64_t)num_cores : nullptr;

    uint64_t k[kRecsPerLane];
    u64x2 lo[kRecsPerLane], hi[kRecsPerLane];
#pragma unroll
    for (int u = 0; u < kRecsPerLane; u++) {
        k[u] = tile_record(tile, lane, u);
        lo[u] = hi[u] = u64x2{0ull, 0ull};
        if (record_live(k[u], got)) {
            lo[u] = src[2 * k[u]];
            hi[u] = src[2 * k[u] + 1];
        }
    }
    if (STAGED) {
        for (int c = lane; c < num_cores; c += kLanes) {
            s_rows[c] = placed_core(prow, c);
            s_rows[num_cores + c] = skew_of(srow, c);
        }
        __syncthreads();
    }
    if (d_got && tile == 0 && lane == 0) d_got[replica] = got;

#pragma unroll
    for (int u = 0; u < kRecsPerLane; u++) {
        if (!record_live(k[u], got)) continue;
        const uint64_t in[4] = {lo[u].x, lo[u].y, hi[u].x, hi[u].y};
        const int32_t core = word_core(in[2]);
        const int32_t core2 = STAGED ? s_rows[core] : placed_core(prow, core);
        const int32_t sk = STAGED ? s_rows[num_cores + core] : skew_of(srow, core);
        const int64_t timer2 = skewed_timer((int64_t)in[1], sk);
        const uint64_t o = out_index(replica, stride, k[u]);
        if (FMT == PU_REQ_FMT_16) {
            uint64_t w[2];
            place_words16(in, core2, timer2, w);
            out[o] = u64x2{w[0], w[1]};
        } else {
            uint64_t w[4];
            place_words32(in, core2, timer2, w);
            out[2 * o] = u64x2{w[0], w[1]};
            out[2 * o + 1] = u64x2{w[2], w[3]};
        }
    }
}

// at 7,168 replicas x 1,024 cores the gathered kernel writes 5.9 TB/s (pu_req) and 4.5 TB/s
// (pu_req16), the staged one 3.5 and 2.8 TB/s
constexpr bool kDefaultStaged = false;

// lds: rows staged wherever they fit; global: never; unset: the default above, wherever they fit.
bool stage_rows(int num_cores, bool has_rows) {
    if (!has_rows || !rows_fit_lds(num_cores)) return false;
    const char* e = std::getenv("PRIMEUNCORE_TRACE_ROWS");
    if (e && !std::strcmp(e, "lds")) return true;
    if (e && !std::strcmp(e, "global")) return false;
    return kDefaultStaged;
}

void load_words(const pu_req& q, uint64_t w[4]) { std::memcpy(w, &q, sizeof q); }

// A row pair as pu_dtrace_open and pu_trace_place take it: `who` names the replica in the message.
int check_rows(const char* fn, const std::string& who, const int32_t* place, const int32_t* skew, int num_cores,
               std::vector<uint8_t>& seen) {
    if (place) {
        seen.assign((size_t)num_cores, 0);
        for (int c = 0; c < num_cores; c++) {
            const int32_t p = place[c];
            if (p < 0 || p >= num_cores)
                return pu::set_error(PU_EINVAL, std::string(fn) + ": the placement" + who + " is no permutation: entry " +
                                                    std::to_string(c) + " (" + std::to_string(p) + ") is out of range");
            if (seen[(size_t)p])
                return pu::set_error(PU_EINVAL, std::string(fn) + ": the placement" + who + " is no permutation: entry " +
                                                    std::to_string(c) + " repeats core " + std::to_string(p));
            seen[(size_t)p] = 1;
        }
    }
    if (skew)
        for (int c = 0; c < num_cores; c++)
            if (skew[c] < 0)
                return pu::set_error(PU_EINVAL, std::string(fn) + ": the skew" + who + " of core " + std::to_string(c) +
                                                    " is negative (" + std::to_string(skew[c]) + ")");
    return 0;
}

bool cores_ok(const char* fn, int num_cores) {
    if (num_cores >= 1 && num_cores <= kMaxCores) return true;
    pu::set_error(PU_EINVAL, std::string(fn) + ": num_cores " + std::to_string(num_cores) + " is outside 1 .. 65536");
    return false;
}

}  // namespace

struct pu_dtrace : pu::DeviceSet {
    size_t n = 0;
    int num_cores = 0, count = 0;
    int64_t pos = 0;
    std::string refuse16;   // why the set has no format 16 ("" = it fits)
    const u64x2* trace = nullptr;
    const int32_t* place = nullptr;   // NULL: identity
    const int32_t* skew = nullptr;    // NULL: zeros
};

extern "C" {

pu_dtrace* pu_dtrace_open(const pu_req* trace, size_t n, int num_cores, int count, const int32_t* placement,
                          const int32_t* skew, int device) {
    const char* const fn = "pu_dtrace_open";
    if (!trace || n == 0 || n > (size_t)INT64_MAX / sizeof(pu_req) || count <= 0) {
        pu::set_error(PU_EINVAL, "pu_dtrace_open: no trace or no replicas");
        return nullptr;
    }
    if (!cores_ok(fn, num_cores)) return nullptr;

    // the trace: every core inside the configuration; what format 16 needs to know
    int64_t tmax = INT64_MIN;
    std::string unfit;
    for (size_t i = 0; i < n; i++) {
        const pu_req& q = trace[i];
        if (q.core < 0 || q.core >= num_cores) {
            pu::set_error(PU_ERANGE, "pu_dtrace_open: record " + std::to_string(i) + " has core " + std::to_string(q.core) +
                                         ", outside [0, " + std::to_string(num_cores) + ")");
            return nullptr;
        }
        if (q.timer > tmax) tmax = q.timer;
        if (unfit.empty()) {
            uint64_t w[4];
            load_words(q, w);
            if (!words_fit16(w, q.timer < 0 ? q.timer : 0))   // the timer's upper end is judged with the skew, below
                unfit = "record " + std::to_string(i) + " does not fit pu_req16";
        }
    }
    // the rows
    int32_t smax = 0;
    std::vector<uint8_t> seen;
    for (int r = 0; r < count; r++) {
        const size_t at = (size_t)r * (size_t)num_cores;
        if (check_rows(fn, " of replica " + std::to_string(r), placement ? placement + at : nullptr, skew ? skew + at : nullptr,
                       num_cores, seen) != 0)
            return nullptr;
        if (skew)
            for (int c = 0; c < num_cores; c++)
                if (skew[at + (size_t)c] > smax) smax = skew[at + (size_t)c];
    }
    if (tmax > INT64_MAX - (int64_t)smax) {
        pu::set_error(PU_ERANGE, "pu_dtrace_open: timer " + std::to_string(tmax) + " plus skew " + std::to_string(smax) +
                                     " overflows int64");
        return nullptr;
    }
    if (unfit.empty() && tmax + (int64_t)smax >= (int64_t)1 << PU_REQ16_TIMER_BITS)
        unfit = "the largest timer " + std::to_string(tmax) + " plus the largest skew " + std::to_string(smax) +
                " is not below 2^40";

    if (pu::device_check(device, "the device replay has no CPU fallback; pu_trace_place places host arrays") != 0)
        return nullptr;
    pu_dtrace* s = pu::new_set<pu_dtrace>();
    if (!s) return nullptr;
    s->n = n;
    s->num_cores = num_cores;
    s->count = count;
    if (!unfit.empty()) s->refuse16 = "pu_dtrace_next: the set does not fit pu_req16: " + unfit;

    // layout: trace | placement | skew
    const size_t trace_bytes = n * sizeof(pu_req);
    const size_t row_bytes = round16((size_t)count * (size_t)num_cores * sizeof(int32_t));
    const size_t off_place = trace_bytes, off_skew = off_place + (placement ? row_bytes : 0);
    const size_t bytes = off_skew + (skew ? row_bytes : 0);
    if (s->open(device, bytes, "pu_dtrace_open: a trace of " + std::to_string(n) + " records and the rows of " +
                                   std::to_string(count) + " replicas (" + std::to_string(num_cores) + " cores)") != 0)
        return pu::drop_set(s);
    const size_t rows = (size_t)count * (size_t)num_cores * sizeof(int32_t);
    bool ok = hipMemcpyAsync(s->base, trace, trace_bytes, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (ok && placement)
        ok = hipMemcpyAsync(s->base + off_place, placement, rows, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (ok && skew) ok = hipMemcpyAsync(s->base + off_skew, skew, rows, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(s->stream) != hipSuccess)   // the arrays are the caller's
        return pu::drop_set(s, PU_EIO, "pu_dtrace_open: upload failed");
    s->trace = (const u64x2*)s->base;
    s->place = placement ? (const int32_t*)(s->base + off_place) : nullptr;
    s->skew = skew ? (const int32_t*)(s->base + off_skew) : nullptr;
    return s;
}

void pu_dtrace_close(pu_dtrace* s) { pu::close_set(s); }

int pu_dtrace_next(pu_dtrace* s, void* d_out, size_t n_each, size_t stride, int fmt, uint64_t* d_got, void* hip_stream) {
    if (!s || !pu::req_fmt_ok(fmt) || stride < n_each || (!d_out && n_each) || ((uintptr_t)d_out & 15))
        return pu::set_error(PU_EINVAL, "pu_dtrace_next: bad arguments");
    if (fmt == PU_REQ_FMT_16 && !s->refuse16.empty()) return pu::set_error(PU_ERANGE, s->refuse16);
    const uint64_t left = (uint64_t)s->n - (uint64_t)s->pos;
    const uint64_t got = n_each < left ? n_each : left;
    if (got == 0 && !d_got) return 0;
    int rc = s->use();
    if (rc) return rc;
    hipStream_t st = s->pick(hip_stream);
    rc = s->order_before(st);
    if (rc) return rc;

    const bool staged = stage_rows(s->num_cores, s->place || s->skew);
    const unsigned lds = staged ? (unsigned)rows_lds_bytes(s->num_cores) : 0u;
    const uint64_t tiles = launch_tiles(got), total = (uint64_t)s->count * tiles;
    const u64x2* const src = s->trace + 2 * (uint64_t)s->pos;
    for (uint64_t sl = 0; sl < slices_of(total); sl++) {
        const dim3 grid((unsigned)slice_size(total, sl));
        const uint64_t base = sl * kMaxGridX;
#define PU_DTRACE_LAUNCH(F, S)                                                                                      \
    hipLaunchKernelGGL((dtrace_place_kernel<F, S>), grid, dim3(kLanes), lds, st, src, s->place, s->skew, s->num_cores, \
                       (u64x2*)d_out, got, (uint64_t)stride, tiles, base, d_got)
        if (fmt == PU_REQ_FMT_16) {
            if (staged) PU_DTRACE_LAUNCH(PU_REQ_FMT_16, true);
            else PU_DTRACE_LAUNCH(PU_REQ_FMT_16, false);
        } else {
            if (staged) PU_DTRACE_LAUNCH(PU_REQ_FMT_32, true);
            else PU_DTRACE_LAUNCH(PU_REQ_FMT_32, false);
        }
#undef PU_DTRACE_LAUNCH
    }
    rc = s->record_after(st, "pu_dtrace_next");
    if (rc) return rc;
    s->pos += (int64_t)got;
    return 0;
}

int pu_dtrace_seek(pu_dtrace* s, int64_t position) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dtrace_seek: no set");
    if (position < 0 || (uint64_t)position > (uint64_t)s->n)
        return pu::set_error(PU_ERANGE, "pu_dtrace_seek: position " + std::to_string(position) + " is outside [0, " +
                                            std::to_string(s->n) + "]");
    int rc = s->use();
    if (!rc) rc = s->wait_outstanding();
    if (rc) return rc;
    s->pos = position;
    return 0;
}

int64_t pu_dtrace_position(pu_dtrace* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dtrace_position: no set");
    int rc = s->use();
    if (!rc) rc = s->wait_outstanding();
    return rc ? rc : s->pos;
}

int pu_dtrace_fits_req16(const pu_dtrace* s) {
    if (!s) return pu::set_error(PU_EINVAL, "pu_dtrace_fits_req16: no set");
    return s->refuse16.empty() ? 0 : pu::set_error(PU_ERANGE, s->refuse16);
}

uint64_t pu_dtrace_state_bytes(const pu_dtrace* s) { return s ? (uint64_t)s->bytes : 0; }

int pu_trace_place(const pu_req* in, size_t n, const int32_t* place_row, const int32_t* skew_row, int num_cores, int fmt,
                   void* out) {
    const char* const fn = "pu_trace_place";
    if (!pu::req_fmt_ok(fmt) || (n && (!in || !out))) return pu::set_error(PU_EINVAL, "pu_trace_place: bad arguments");
    if (!cores_ok(fn, num_cores)) return PU_EINVAL;
    std::vector<uint8_t> seen;
    int rc = check_rows(fn, "", place_row, skew_row, num_cores, seen);
    if (rc) return rc;
    uint64_t* const o = (uint64_t*)out;
    for (size_t i = 0; i < n; i++) {
        const pu_req& q = in[i];
        if (q.core < 0 || q.core >= num_cores)
            return pu::set_error(PU_ERANGE, "pu_trace_place: record " + std::to_string(i) + " has core " +
                                                std::to_string(q.core) + ", outside [0, " + std::to_string(num_cores) + ")");
        const int32_t sk = skew_of(skew_row, q.core);
        if (q.timer > INT64_MAX - (int64_t)sk)
            return pu::set_error(PU_ERANGE, "pu_trace_place: record " + std::to_string(i) + ": timer plus skew overflows int64");
        uint64_t w[4];
        load_words(q, w);
        const int32_t core2 = placed_core(place_row, q.core);
        const int64_t timer2 = skewed_timer(q.timer, sk);
        if (fmt == PU_REQ_FMT_16) {
            if (!words_fit16(w, timer2))
                return pu::set_error(PU_ERANGE, "pu_trace_place: request " + std::to_string(i) + " does not fit pu_req16");
            place_words16(w, core2, timer2, o + 2 * i);
        } else {
            place_words32(w, core2, timer2, o + 4 * i);
        }
    }
    return 0;
}

int pu_placement_shuffle(int32_t* row, int num_cores, uint64_t seed) {
    if (!row) return pu::set_error(PU_EINVAL, "pu_placement_shuffle: no row");
    if (!cores_ok("pu_placement_shuffle", num_cores)) return PU_EINVAL;
    placement_shuffle(row, num_cores, seed);
    return 0;
}

}  // extern "C"
