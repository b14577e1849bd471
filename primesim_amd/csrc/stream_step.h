// stream_step.h — one core's step of the synthetic request streams, shared by
// the host generator (stream.cpp) and the device generator (stream_gen.hip):
// the splitmix64 draws, the address patterns, the gap rule, and the rule that
// cuts a group of cores at the end of a chunk.  Everything here compiles as
// plain C++ on the host (PU_HD is empty there) and as __host__ __device__
// under hipcc's HIP mode, so both generators run the same arithmetic.
#pragma once

#include <cstdint>

#include "../../include/primeuncore.h"
#include "pu_hd.h"

namespace pu_stream_step {

constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;

struct SplitMix64 {
    uint64_t s;
    PU_HD static uint64_t mix(uint64_t z) {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    PU_HD uint64_t next() { return mix(s += kGamma); }
};

constexpr uint64_t kLine = 64;
constexpr uint64_t kMB = 1ull << 20;
// draws a request takes: two for its address and type (make_request), one for the gap after it
constexpr uint64_t kDrawsPerRequest = 3;

PU_HD inline int default_write_pct(int kind) {
    switch (kind) {
        case PU_STREAM_PRIVATE_STREAMING: return 10;
        case PU_STREAM_SHARED_UNIFORM: return 30;
        case PU_STREAM_MULTIPROGRAM: return 20;
        case PU_STREAM_UNIFORM_HOTSPOT: return 25;
        case PU_STREAM_PRODUCER_CONSUMER: return 50;
        case PU_STREAM_UNIFORM: return 25;
        default: return -1;
    }
}

PU_HD inline int prog_of(const pu_stream_params* p, int core) {
    int np = p->num_progs > 0 ? p->num_progs : 1;
    return 1 + (int)((int64_t)core * np / p->num_cores);
}

// The rule of pu_stream_open / pu_dstream_open.
inline bool params_ok(const pu_stream_params* p) {
    if (!p) return false;
    if (p->kind < PU_STREAM_PRIVATE_STREAMING || p->kind > PU_STREAM_UNIFORM) return false;
    if (p->num_cores <= 0 || p->quantum <= 0 || p->num_quanta < 0 || p->max_msg <= 0) return false;
    return true;
}

// The gap rule: cycles a core advances after a request, from the draw that follows it.
PU_HD inline int64_t gap_of(uint64_t draw) { return 1 + (int64_t)(draw & 3); }

// One request's address and type for core `c`.  G is the core's generator
// state: rng, stream_pos, n_recent, recent_head and the C2 re-use ring behind
// recent_get(i) / recent_set(i, a) (an array on the host, device memory in
// the kernel).
template <class G>
PU_HD inline void make_request(const pu_stream_params* p, int c, G& g, int wpct, uint64_t* addr, uint8_t* type) {
    uint64_t r0 = g.rng.next();
    uint64_t r1 = g.rng.next();
    uint64_t word = (r1 >> 20) & 7;  // 8-byte word within the line
    bool wr = (int)(r1 % 100) < wpct;
    uint64_t a = 0;
    switch (p->kind) {
        case PU_STREAM_PRIVATE_STREAMING: {
            if (r0 % 100 < 5) {  // shared read-mostly table
                a = 0x10000000ull + (r0 >> 8) % (64 * 1024 / 8) * 8;
                wr = false;
            } else {
                uint64_t base = 0x100000000ull + (uint64_t)c * 16 * kMB;
                a = base + (g.stream_pos * 8) % (2 * kMB);
                g.stream_pos++;
            }
            break;
        }
        case PU_STREAM_SHARED_UNIFORM: {
            if (r0 % 100 < 30 && g.n_recent > 0) {
                a = g.recent_get((r0 >> 8) % (uint64_t)g.n_recent);
            } else {
                a = 0x40000000ull + (r0 >> 8) % (64 * kMB / 8) * 8;
                g.recent_set(g.recent_head, a);
                g.recent_head = (g.recent_head + 1) & 15;
                if (g.n_recent < 16) g.n_recent++;
            }
            break;
        }
        case PU_STREAM_MULTIPROGRAM: {
            int prog = prog_of(p, c);
            uint64_t fp_mb = 4;
            switch ((prog - 1) & 3) {
                case 1: fp_mb = 16; break;
                case 2: fp_mb = 32; break;
                case 3: fp_mb = 64; break;
                default: break;
            }
            uint64_t fp = fp_mb * kMB;
            uint64_t base = 0x80000000ull;
            if (r0 % 100 < 50) {
                int np = p->num_progs > 0 ? p->num_progs : 1;
                int per = p->num_cores / np > 0 ? p->num_cores / np : 1;
                uint64_t slice = fp / (uint64_t)per;
                if (slice < kLine) slice = kLine;
                uint64_t first = (uint64_t)(c % per) * slice;
                a = base + (first + (g.stream_pos * 8) % slice) % fp;
                g.stream_pos++;
            } else {
                a = base + (r0 >> 8) % (fp / 8) * 8;
            }
            break;
        }
        case PU_STREAM_UNIFORM_HOTSPOT: {
            if (r0 % 100 < 20) {
                a = 0x20000000ull + ((r0 >> 8) % 64) * kLine + word * 8;
            } else {
                a = 0x40000000ull + ((r0 >> 8) % (1ull << 20)) * kLine + word * 8;
            }
            break;
        }
        case PU_STREAM_PRODUCER_CONSUMER: {
            int half = p->num_cores / 2 > 0 ? p->num_cores / 2 : 1;
            int pair = c % half;
            a = 0x100000000ull + (uint64_t)pair * 1024 * kLine + ((r0 >> 8) % 1024) * kLine + word * 8;
            break;
        }
        case PU_STREAM_UNIFORM:
        default: {
            a = 0x40000000ull + ((r0 >> 8) % (1ull << 20)) * kLine + word * 8;
            break;
        }
    }
    *addr = a;
    *type = wr ? PU_WR : PU_RD;
}

// How many requests a core in state (rng s, cycle) issues before `barrier`,
// counted up to `cap` (the caller needs no more than "above what it takes").
// Only the gap draws matter: a request takes kDrawsPerRequest draws and the
// state after k draws is s + k*gamma, so the count costs one mix per request.
PU_HD inline uint64_t count_before(uint64_t s, int64_t cycle, int64_t barrier, uint64_t cap) {
    uint64_t n = 0;
    while (cycle < barrier && n < cap) {
        n++;
        s += kDrawsPerRequest * kGamma;
        cycle += gap_of(SplitMix64::mix(s));
    }
    return n;
}

// ---------------------------------------------------------------- scan and cut
// The device generator takes a stream's cores a group at a time, in core
// order from the cursor: core cur.c + i has cnt[i] requests left before the
// barrier of quantum cur.q and excl[i] = cnt[0] + .. + cnt[i-1].  A call that
// still takes `want` records cuts the group at the first core whose inclusive
// sum exceeds want: cores before it write all their requests, the cut core
// writes the remainder and stays part-way through its quantum, later cores
// are untouched.  (The host generator leaves its cursor on a core that has
// just reached the barrier and moves on at the next call; moving on at once
// gives the same requests.)  cnt may be capped at want + 1: the first core
// whose inclusive sum exceeds want is the same, and so is every take.
struct Cursor {
    int32_t q;       // current quantum
    int32_t c;       // current core within the quantum
    int32_t in_msg;  // requests already in core c's open message
    int64_t n;       // requests produced so far
};

// Records a call may still write: what is left of its chunk and of the stream's limit.
PU_HD inline uint64_t chunk_want(uint64_t n_each, uint64_t k, int64_t limit, int64_t n) {
    uint64_t a = n_each - k, b = (uint64_t)(limit - n);
    return a < b ? a : b;
}

// Requests the core writes in this trip.
PU_HD inline uint64_t cut_take(uint64_t excl, uint64_t cnt, uint64_t want) {
    if (excl >= want) return 0;
    return cnt < want - excl ? cnt : want - excl;
}

// True for the first core of the group that does not finish its quantum.
PU_HD inline bool cut_here(uint64_t excl, uint64_t cnt, uint64_t want) { return excl <= want && cnt > want - excl; }

// in_msg a core starts the trip with: only the cursor's own core may be inside a message.
PU_HD inline int32_t start_in_msg(const Cursor& cur, int lane) { return lane == 0 ? cur.in_msg : 0; }

// The cursor after a trip over `group` cores that wrote `written` records;
// cut_lane < 0: every core of the group finished, else the cut core wrote cut_taken.
PU_HD inline void cursor_advance(Cursor& cur, int group, int cut_lane, uint64_t cut_taken, uint64_t written,
                                 int num_cores, int max_msg) {
    cur.n += (int64_t)written;
    if (cut_lane >= 0) {
        int32_t im = start_in_msg(cur, cut_lane);
        cur.c += cut_lane;
        cur.in_msg = (int32_t)(((uint64_t)im + cut_taken) % (uint64_t)max_msg);
        return;
    }
    cur.in_msg = 0;
    cur.c += group;
    if (cur.c >= num_cores) {
        cur.c = 0;
        cur.q++;
    }
}

// ------------------------------------------------------------------------ fork
// pu_stream_fork / pu_dstream_fork: the destination continues from the source's
// position (a warmed replica's clocks stand at the source's cycles, not at 0)
// with the source's random draws or, reseeded, with those of another seed.
//   * cursor (q, c, in_msg, n) and limit: the source's;
//   * every core's cycle and streaming position, and for
//     PU_STREAM_SHARED_UNIFORM the re-use ring with its two counters: the
//     source's (copied by the caller: plain copies);
//   * a core's generator state: the source's, or seed_state(seed, k) reseeded;
//   * params.seed: the source's, or `seed` reseeded; nothing else changes.

// The generator state a stream of `seed` opens core k with.
PU_HD inline uint64_t seed_state(uint64_t seed, int k) { return seed * 0x100000000ull + (uint64_t)k; }

PU_HD inline uint64_t fork_rng(uint64_t src_state, bool reseed, uint64_t seed, int k) {
    return reseed ? seed_state(seed, k) : src_state;
}

// The header's part; D and S have p, q, c, in_msg, n and limit (StreamGen, DsHdr).
template <class D, class S>
PU_HD inline void fork_cursor(D& d, const S& s, bool reseed, uint64_t seed) {
    d.q = s.q;
    d.c = s.c;
    d.in_msg = s.in_msg;
    d.n = s.n;
    d.limit = s.limit;
    d.p.seed = reseed ? seed : s.p.seed;
}

// A destination is sized for its own shape: it takes a fork only from a source
// whose parameters equal its own in every field but the seed.
inline bool fork_params_match(const pu_stream_params& a, const pu_stream_params& b) {
    return a.kind == b.kind && a.num_cores == b.num_cores && a.quantum == b.quantum && a.num_quanta == b.num_quanta &&
           a.max_msg == b.max_msg && a.num_progs == b.num_progs && a.max_requests == b.max_requests &&
           a.write_pct == b.write_pct;
}

}  // namespace pu_stream_step
