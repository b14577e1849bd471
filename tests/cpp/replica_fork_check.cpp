// replica_fork_check.cpp — the index rules of pu_replica_fork
// (primesim_amd/csrc/replica_fork_step.h) and the stream fork rule
// (primesim_amd/csrc/stream_step.h) on the host, as a stand-alone program for the
// address and undefined-behaviour sanitizers:
//   * for each replica size the lane ranges of all tiles cover [0, replica_bytes)
//     exactly once (sizes that are a tile, less than a tile, a tile and a tail,
//     17 MiB + 4 KiB, and past 2^33, where a 32-bit offset would wrap);
//   * for random (R, src, first, n, G) the groups' destination lists together are
//     [first, first + n) without src, each replica once;
//   * fork_cursor / fork_rng / fork_params_match against a field-by-field
//     restatement.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../primesim_amd/csrc/replica_fork_step.h"
#include "../../primesim_amd/csrc/stream_step.h"

using namespace pu_fork_step;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint64_t rnd_state = 0x1234567;
static uint64_t rnd() { return pu_stream_step::SplitMix64::mix(rnd_state += pu_stream_step::kGamma); }

// Every piece of every tile: live pieces are consecutive from 0 and end at replica_bytes.
// One bit per 16-B piece would be 64 MiB at 2^33 bytes; the pieces of a tile are instead
// checked to be a permutation of the tile's consecutive piece indices (one small bitmap per
// tile), and tiles to follow each other without a gap.
static int cover(uint64_t bytes, uint64_t* pieces_out) {
    const uint64_t tiles = tiles_of(bytes);
    CHECK(tiles * kTileBytes >= bytes && (tiles - 1) * kTileBytes < bytes);
    const uint64_t per_tile = (uint64_t)kLanes * kPieces;
    uint64_t live = 0;
    std::vector<uint8_t> seen(per_tile);
    for (uint64_t t = 0; t < tiles; t++) {
        std::fill(seen.begin(), seen.end(), 0);
        const uint64_t lo = t * kTileBytes;
        const uint64_t want = (bytes - lo < kTileBytes ? bytes - lo : kTileBytes) / kPieceBytes;   // live pieces of this tile
        uint64_t got = 0;
        for (int lane = 0; lane < kLanes; lane++)
            for (int u = 0; u < kPieces; u++) {
                const uint64_t off = piece_offset(t, lane, u);
                CHECK(off >= lo && off < lo + kTileBytes && off % kPieceBytes == 0);
                const uint64_t k = (off - lo) / kPieceBytes;
                CHECK(!seen[k]);
                seen[k] = 1;
                const bool is_live = piece_live(off, bytes);
                CHECK(is_live == (k < want));                 // the live pieces are the tile's first `want`
                if (is_live) {
                    CHECK(off + kPieceBytes <= bytes);
                    got++;
                }
            }
        CHECK(got == want);
        live += got;
    }
    CHECK(live * kPieceBytes == bytes);
    *pieces_out = live;
    return 0;
}

static int groups(int rounds) {
    for (int it = 0; it < rounds; it++) {
        const int R = 1 + (int)(rnd() % 9000);
        const int src = (int)(rnd() % (uint64_t)R);
        const int first = (int)(rnd() % (uint64_t)R);
        const int n = (int)(rnd() % (uint64_t)(R - first + 1));
        int G = (it & 1) ? groups_of(n) : 1 + (int)(rnd() % 200);   // the launch's G, and any other
        if (n == 0) {
            CHECK(groups_of(n) == 0 && dest_count(src, first, n) == 0);
            continue;
        }
        CHECK(groups_of(n) >= 1 && groups_of(n) <= kMaxGroups && groups_of(n) <= n);
        std::vector<int> hits((size_t)R, 0);
        int total = 0;
        for (int g = 0; g < G; g++)
            for (int64_t d = dest_begin(first, g); d < dest_end(first, n); d += G)
                if (dest_taken(d, src)) {
                    CHECK(d >= 0 && d < R);
                    hits[(size_t)d]++;
                    total++;
                }
        for (int r = 0; r < R; r++) CHECK(hits[(size_t)r] == ((r >= first && r < first + n && r != src) ? 1 : 0));
        CHECK(total == dest_count(src, first, n));
    }
    return 0;
}

struct Hdr {   // the fields fork_cursor touches, and two it must not
    pu_stream_params p;
    int32_t wpct, q, c, in_msg;
    int64_t n, limit;
    uint64_t core0, ring_off;
};

static int stream_rule(int rounds) {
    using namespace pu_stream_step;
    for (int it = 0; it < rounds; it++) {
        Hdr s{}, d{};
        s.p = pu_stream_params{1 + (int32_t)(rnd() % 6), 1 + (int32_t)(rnd() % 2000), rnd(), 1 + (int32_t)(rnd() % 1000),
                               (int32_t)(rnd() % 100), 1 + (int32_t)(rnd() % 100), (int32_t)(rnd() % 8),
                               (int64_t)(rnd() % 100000), (int32_t)(rnd() % 101) - 1, 0};
        d.p = s.p;
        d.p.seed = rnd();
        s.wpct = d.wpct = 17;
        s.q = (int32_t)(rnd() % 50);
        s.c = (int32_t)(rnd() % (uint64_t)s.p.num_cores);
        s.in_msg = (int32_t)(rnd() % (uint64_t)s.p.max_msg);
        s.n = (int64_t)(rnd() % 1000000);
        s.limit = (it & 1) ? INT64_MAX : (int64_t)(rnd() % 1000000);
        s.core0 = 11;
        s.ring_off = 4096;
        d.core0 = 5000;
        d.ring_off = 8192;
        d.q = d.c = d.in_msg = 99;
        d.n = d.limit = 77;
        CHECK(fork_params_match(d.p, s.p) && fork_params_match(s.p, d.p));
        const bool reseed = (it & 2) != 0;
        const uint64_t seed = rnd();
        const Hdr s0 = s;
        fork_cursor(d, s, reseed, seed);
        CHECK(d.q == s0.q && d.c == s0.c && d.in_msg == s0.in_msg && d.n == s0.n && d.limit == s0.limit);
        CHECK(d.p.seed == (reseed ? seed : s0.p.seed));
        CHECK(d.core0 == 5000 && d.ring_off == 8192 && d.wpct == 17);
        CHECK(d.p.kind == s0.p.kind && d.p.num_cores == s0.p.num_cores && d.p.quantum == s0.p.quantum &&
              d.p.num_quanta == s0.p.num_quanta && d.p.max_msg == s0.p.max_msg && d.p.num_progs == s0.p.num_progs &&
              d.p.max_requests == s0.p.max_requests && d.p.write_pct == s0.p.write_pct);
        CHECK(s.q == s0.q && s.n == s0.n && s.p.seed == s0.p.seed);   // the source is read only
        const int k = (int)(rnd() % (uint64_t)s.p.num_cores);
        const uint64_t state = rnd();
        CHECK(fork_rng(state, false, seed, k) == state);
        CHECK(fork_rng(state, true, seed, k) == (seed << 32) + (uint64_t)k);
        CHECK(seed_state(seed, k) == (seed << 32) + (uint64_t)k);
        // one differing field at a time is a mismatch; the seed alone is not
        pu_stream_params m = s.p;
        m.seed ^= 1;
        CHECK(fork_params_match(m, s.p));
        m = s.p; m.kind = m.kind % 6 + 1;       CHECK(!fork_params_match(m, s.p));
        m = s.p; m.num_cores++;                 CHECK(!fork_params_match(m, s.p));
        m = s.p; m.quantum++;                   CHECK(!fork_params_match(m, s.p));
        m = s.p; m.num_quanta++;                CHECK(!fork_params_match(m, s.p));
        m = s.p; m.max_msg++;                   CHECK(!fork_params_match(m, s.p));
        m = s.p; m.num_progs++;                 CHECK(!fork_params_match(m, s.p));
        m = s.p; m.max_requests++;              CHECK(!fork_params_match(m, s.p));
        m = s.p; m.write_pct++;                 CHECK(!fork_params_match(m, s.p));
    }
    return 0;
}

int main() {
    const uint64_t MiB = 1ull << 20;
    const uint64_t sizes[] = {4096, 12288, 16384, 20480, 17 * MiB + 4096, (1ull << 33) + 4096};
    uint64_t pieces = 0;
    for (uint64_t b : sizes) {
        uint64_t p = 0;
        if (cover(b, &p)) return 1;
        pieces += p;
    }
    const int rounds = 2000;
    if (groups(rounds)) return 1;
    if (stream_rule(rounds)) return 1;
    std::printf("OK %zu sizes %llu pieces, %d ranges, %d forks\n", sizeof sizes / sizeof sizes[0], (unsigned long long)pieces,
                rounds, rounds);
    return 0;
}
