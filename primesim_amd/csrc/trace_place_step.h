// trace_place_step.h — one record's step of a recorded trace replayed under a
// replica's thread placement and start skew (pu_dtrace_*, pu_trace_place;
// trace_place.hip), written once: the rule itself, the shuffle that draws a
// placement, how a call's records are cut into tiles and where a record of a
// replica lands in the output.  Plain C++ on the host (PU_HD is empty there),
// __host__ __device__ under hipcc, so the host twin, the kernel and the
// stand-alone check (tests/cpp/trace_place_check.cpp) run the same arithmetic.
//
// The rule, for a source record q of a replica with placement row `place` and
// skew row `skew` (both int32[num_cores]; NULL = identity / zeros):
//   core'  = place[q.core]
//   timer' = q.timer + skew[q.core]        (the trace's core, not the placed one)
//   addr, prog_id, mem_type, batch_start, tag: unchanged.
// As pu_req all 32 bytes are written, _pad1 = 0; as pu_req16 the fields go
// through PU_REQ16_B (tag is not part of that layout).  q.core is inside
// [0, num_cores): the callers have checked it.
//
// A record is handled as its four little-endian 64-bit words
//   w0 = addr   w1 = timer   w2 = core | prog_id << 32
//   w3 = mem_type | batch_start << 8 | tag << 16 | _pad1 << 32
// which is how the kernel loads it (two 16-B loads) and stores it.
//
// Tiles.  A call writes records [0, got) of every replica.  A workgroup of
// kLanes owns one tile of kTileRecs consecutive records of one replica; lane l
// takes records tile*kTileRecs + l, + kLanes, ... (kRecsPerLane of them), so the
// 64 lanes of a wave store 64 consecutive records: whole 128-B lines in either
// format.  Replica and tile fold into one linear workgroup index
// (wg = replica * tiles + tile), launched in slices of at most kMaxGridX, so
// neither the y grid limit nor 2^31 workgroups bounds a set.  Record k of
// replica i lands at record index i * stride + k: 64-bit, a row may start past
// 2^32 bytes.
//
// The LDS cap.  The staged kernel keeps a replica's two rows (8 B per core) in
// LDS.  A CU has 160 KiB of LDS and holds at most 8 workgroups of 256 lanes
// (32 waves); the kernel is bound by its stores, and eight resident workgroups
// are what keeps stores in flight while others wait at their barrier.  160 KiB
// / 8 = 20 KiB = 16 allocation granules of 1,280 B, so rows of up to
// kStageCapBytes = 20,480 B (2,560 cores) cost no occupancy; wider rows are
// gathered from global memory (L2) instead.
#pragma once

#include <cstdint>

#include "../../include/primeuncore_records.h"
#include "pu_hd.h"
#include "stream_step.h"

namespace pu_trace_step {

constexpr int kMaxCores = 1 << PU_REQ16_CORE_BITS;   // 65,536: a placed core always fits pu_req16

// ---------------------------------------------------------------- the rule
PU_HD inline int32_t word_core(uint64_t w2) { return (int32_t)(uint32_t)w2; }
PU_HD inline int32_t word_prog(uint64_t w2) { return (int32_t)(uint32_t)(w2 >> 32); }

PU_HD inline int32_t placed_core(const int32_t* place, int32_t core) { return place ? place[core] : core; }
// unsigned addition: pu_dtrace_open and pu_trace_place refuse what would overflow
PU_HD inline int64_t skewed_timer(int64_t timer, int32_t skew) { return (int64_t)((uint64_t)timer + (uint64_t)(int64_t)skew); }
PU_HD inline int32_t skew_of(const int32_t* skew, int32_t core) { return skew ? skew[core] : 0; }

// The placed record as pu_req words.
PU_HD inline void place_words32(const uint64_t in[4], int32_t core2, int64_t timer2, uint64_t out[4]) {
    out[0] = in[0];
    out[1] = (uint64_t)timer2;
    out[2] = (in[2] & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)core2;
    out[3] = in[3] & 0xFFFFFFFFull;   // mem_type, batch_start, tag; _pad1 = 0
}
// The placed record as pu_req16 words.
PU_HD inline void place_words16(const uint64_t in[4], int32_t core2, int64_t timer2, uint64_t out[2]) {
    out[0] = in[0];
    out[1] = PU_REQ16_B(timer2, core2, word_prog(in[2]), in[3] & 0xFFu, (in[3] >> 8) & 0xFFu);
}

// What pu_pack_req16 accepts of a placed record (its core fits: kMaxCores).
PU_HD inline bool words_fit16(const uint64_t in[4], int64_t timer2) {
    const int32_t prog = word_prog(in[2]);
    return timer2 >= 0 && timer2 < (int64_t)1 << PU_REQ16_TIMER_BITS && prog >= 0 && prog < 1 << PU_REQ16_PROG_BITS &&
           (in[3] & 0xFFu) <= 1 && ((in[3] >> 8) & 0xFFu) <= 1 && ((in[3] >> 16) & 0xFFFFu) == 0;
}

// ---------------------------------------------------------------- placements
// pu_placement_shuffle: the identity for seed 0; otherwise the identity
// shuffled by Fisher-Yates from the top, i = num_cores - 1 .. 1 swapping row[i]
// with row[j], j = draw % (i + 1), the draws being SplitMix64{seed}.next()
// (stream_step.h) in order.
inline void placement_shuffle(int32_t* row, int num_cores, uint64_t seed) {
    for (int c = 0; c < num_cores; c++) row[c] = c;
    if (seed == 0) return;
    pu_stream_step::SplitMix64 rng{seed};
    for (int i = num_cores - 1; i >= 1; i--) {
        const int j = (int)(rng.next() % (uint64_t)(i + 1));
        const int32_t t = row[i];
        row[i] = row[j];
        row[j] = t;
    }
}

// ---------------------------------------------------------------- tiles and offsets
constexpr int kLanes = 256;
constexpr int kRecsPerLane = 4;
constexpr uint64_t kTileRecs = (uint64_t)kLanes * kRecsPerLane;   // 1,024 records: 32 KiB of pu_req, 16 KiB of pu_req16
constexpr uint64_t kMaxGridX = 1ull << 30;                         // workgroups of one launch
constexpr uint64_t kStageCapBytes = 20480;                         // see above
constexpr uint64_t kRowBytesPerCore = 8;                           // one placement and one skew entry

static_assert(kTileRecs == 1024, "a tile is 1,024 records");
static_assert(kStageCapBytes % 1280 == 0 && 8 * kStageCapBytes == 160 * 1024, "eight workgroups' rows fill a CU's LDS");

PU_HD inline bool rows_fit_lds(int num_cores) { return (uint64_t)num_cores * kRowBytesPerCore <= kStageCapBytes; }
PU_HD inline uint64_t rows_lds_bytes(int num_cores) { return ((uint64_t)num_cores * kRowBytesPerCore + 15) & ~15ull; }

PU_HD inline uint64_t tiles_of(uint64_t got) { return (got + kTileRecs - 1) / kTileRecs; }
// Tiles a call launches per replica: a call at the end of the trace still has one, whose
// lanes are all masked, to write d_got.
PU_HD inline uint64_t launch_tiles(uint64_t got) { return got ? tiles_of(got) : 1; }
PU_HD inline uint64_t wg_replica(uint64_t wg, uint64_t tiles) { return wg / tiles; }
PU_HD inline uint64_t wg_tile(uint64_t wg, uint64_t tiles) { return wg % tiles; }
// Record (within the call) that `lane` takes as its u-th of `tile`, and whether the call has it.
PU_HD inline uint64_t tile_record(uint64_t tile, int lane, int u) {
    return tile * kTileRecs + (uint64_t)u * kLanes + (uint64_t)lane;
}
PU_HD inline bool record_live(uint64_t k, uint64_t got) { return k < got; }
// Index, in records of the chosen format, of record k of replica i in the output.
PU_HD inline uint64_t out_index(uint64_t replica, uint64_t stride, uint64_t k) { return replica * stride + k; }
// Slices of a launch of `total` workgroups: slice s covers [s * kMaxGridX, ...) and has slice_size of them.
PU_HD inline uint64_t slices_of(uint64_t total) { return (total + kMaxGridX - 1) / kMaxGridX; }
PU_HD inline uint64_t slice_size(uint64_t total, uint64_t s) {
    const uint64_t left = total - s * kMaxGridX;
    return left < kMaxGridX ? left : kMaxGridX;
}

}  // namespace pu_trace_step
