// trace_place_check.cpp — the step of a recorded trace replayed under a replica's
// placement and skew (primesim_amd/csrc/trace_place_step.h) on the host, as a
// stand-alone program for the address and undefined-behaviour sanitizers:
//   * place_words32 / place_words16 against an independent field-by-field loop,
//     for every edge combination (timer 0 and 2^40 - 1 - skew; core 0, the last and
//     65,535; program 1 and 63; both types; both batch bits; a non-zero tag) and for
//     100,000 random records, in both formats, with rows and with NULL rows;
//   * the tile and offset arithmetic against plain loops, for record counts around
//     every tile and workgroup edge, for more replicas than a grid's y limit, for
//     launches around the slice size, and for a stride that puts a row's start past
//     2^32 bytes;
//   * placement_shuffle: permutations for 1, 2, 64 and 1,030 cores over 1,000 seeds,
//     seed 0 the identity, the draws those of SplitMix64.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/primeuncore_records.h"
#include "../../primesim_amd/csrc/trace_place_step.h"

using namespace pu_trace_step;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint64_t rnd_state = 0x7ace;
static uint64_t rnd() { return pu_stream_step::SplitMix64::mix(rnd_state += pu_stream_step::kGamma); }

// One record through the step in both formats, against the fields written out one by one.
static int one(const pu_req& q, const int32_t* place, const int32_t* skew) {
    uint64_t w[4], o32[4], o16[2];
    static_assert(sizeof(pu_req) == sizeof w, "a pu_req is four words");
    std::memcpy(w, &q, sizeof q);
    CHECK(word_core(w[2]) == q.core && word_prog(w[2]) == q.prog_id);
    const int32_t core2 = placed_core(place, q.core);
    const int64_t timer2 = skewed_timer(q.timer, skew_of(skew, q.core));

    // the independent statement
    const int32_t want_core = place ? place[q.core] : q.core;
    const int64_t want_timer = q.timer + (skew ? (int64_t)skew[q.core] : 0);
    CHECK(core2 == want_core && timer2 == want_timer);

    place_words32(w, core2, timer2, o32);
    pu_req r;
    std::memset(&r, 0xA5, sizeof r);
    std::memcpy(&r, o32, sizeof r);
    CHECK(r.addr == q.addr && r.timer == want_timer && r.core == want_core && r.prog_id == q.prog_id);
    CHECK(r.mem_type == q.mem_type && r.batch_start == q.batch_start && r.tag == q.tag && r._pad1 == 0);

    const bool fits = want_timer >= 0 && want_timer < ((int64_t)1 << 40) && q.prog_id >= 0 && q.prog_id < 64 &&
                      q.mem_type <= 1 && q.batch_start <= 1 && q.tag == 0;
    CHECK(words_fit16(w, timer2) == fits);
    if (fits) {
        place_words16(w, core2, timer2, o16);
        const uint64_t b = (uint64_t)want_timer | (uint64_t)want_core << 40 | (uint64_t)q.prog_id << 56 |
                           (uint64_t)q.mem_type << 62 | (uint64_t)q.batch_start << 63;
        CHECK(o16[0] == q.addr && o16[1] == b);
        CHECK(PU_REQ16_TIMER(o16[1]) == want_timer && PU_REQ16_CORE(o16[1]) == want_core &&
              PU_REQ16_PROG(o16[1]) == q.prog_id && PU_REQ16_TYPE(o16[1]) == q.mem_type &&
              PU_REQ16_BATCH(o16[1]) == q.batch_start);
    }
    return 0;
}

static int edges(int* count) {
    const int nc = kMaxCores;
    std::vector<int32_t> place((size_t)nc), skew((size_t)nc);
    for (int c = 0; c < nc; c++) {
        place[(size_t)c] = nc - 1 - c;
        skew[(size_t)c] = c % 1000;
    }
    skew[0] = 0x7FFFFFFF;   // the largest skew there is, on a core the edge cases use
    const int32_t cores[] = {0, nc - 2, 65535};      // 65,535 is also num_cores - 1 here; nc - 2 stands for "another late core"
    const int32_t progs[] = {1, 63};
    const uint16_t tags[] = {0, 0x1234};
    for (int rows = 0; rows < 4; rows++) {
        const int32_t* const p = (rows & 1) ? place.data() : nullptr;
        const int32_t* const s = (rows & 2) ? skew.data() : nullptr;
        for (int32_t core : cores)
            for (int hi = 0; hi < 2; hi++)
                for (int32_t prog : progs)
                    for (int type = 0; type < 2; type++)
                        for (int batch = 0; batch < 2; batch++)
                            for (uint16_t tag : tags) {
                                pu_req q;
                                std::memset(&q, 0xA5, sizeof q);   // _pad1 holds rubbish: the step must clear it
                                q.addr = 0xFEDCBA9876543210ull ^ (uint64_t)*count;
                                q.timer = hi ? ((int64_t)1 << 40) - 1 - (s ? (int64_t)s[core] : 0) : 0;
                                q.core = core;
                                q.prog_id = prog;
                                q.mem_type = (uint8_t)type;
                                q.batch_start = (uint8_t)batch;
                                q.tag = tag;
                                if (one(q, p, s)) return 1;
                                ++*count;
                            }
    }
    // a smaller configuration's last core
    for (int nc2 : {1, 2, 48, 1030}) {
        std::vector<int32_t> pl((size_t)nc2), sk((size_t)nc2, 7);
        placement_shuffle(pl.data(), nc2, 99);
        pu_req q{};
        q.addr = 64;
        q.timer = ((int64_t)1 << 40) - 1 - 7;
        q.core = nc2 - 1;
        q.prog_id = 63;
        q.mem_type = 1;
        q.batch_start = 1;
        if (one(q, pl.data(), sk.data())) return 1;
        ++*count;
    }
    return 0;
}

static int randoms(int n) {
    const int nc = 1030;
    std::vector<int32_t> place((size_t)nc), skew((size_t)nc);
    placement_shuffle(place.data(), nc, 5);
    for (int c = 0; c < nc; c++) skew[(size_t)c] = (int32_t)(rnd() % 100000);
    for (int i = 0; i < n; i++) {
        pu_req q;
        q.addr = rnd();
        q.timer = (int64_t)(rnd() >> ((i & 3) == 3 ? 2 : 25));   // mostly below 2^39, every fourth up to 2^62
        q.core = (int32_t)(rnd() % (uint64_t)nc);
        q.prog_id = (int32_t)(rnd() % ((i & 7) == 7 ? 70 : 64));
        q.mem_type = (uint8_t)(rnd() & 1);
        q.batch_start = (uint8_t)(rnd() & 1);
        q.tag = (i & 15) == 15 ? (uint16_t)rnd() : 0;
        q._pad1 = (int32_t)rnd();
        const int rows = i & 3;
        if (one(q, (rows & 1) ? place.data() : nullptr, (rows & 2) ? skew.data() : nullptr)) return 1;
    }
    return 0;
}

// The lanes of all tiles cover [0, got) exactly once, tile by tile, and a wave's lanes take consecutive records.
static int cover(uint64_t got, uint64_t* live_out) {
    const uint64_t tiles = tiles_of(got);
    CHECK(tiles * kTileRecs >= got && (got == 0 ? tiles == 0 : (tiles - 1) * kTileRecs < got));
    CHECK(launch_tiles(got) == (got ? tiles : 1));
    std::vector<uint8_t> seen((size_t)kTileRecs);
    uint64_t live = 0;
    for (uint64_t t = 0; t < launch_tiles(got); t++) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int lane = 0; lane < kLanes; lane++)
            for (int u = 0; u < kRecsPerLane; u++) {
                const uint64_t k = tile_record(t, lane, u);
                CHECK(k >= t * kTileRecs && k < (t + 1) * kTileRecs);
                CHECK(!seen[(size_t)(k - t * kTileRecs)]);
                seen[(size_t)(k - t * kTileRecs)] = 1;
                if (lane > 0) CHECK(k == tile_record(t, lane - 1, u) + 1);   // neighbours store neighbours
                CHECK(record_live(k, got) == (k < got));
                live += record_live(k, got) ? 1 : 0;
            }
    }
    CHECK(live == got);
    *live_out += live;
    return 0;
}

static int folding() {
    // (replica, tile) from the linear index, for more replicas than the 65,535 of a grid's y
    const uint64_t shapes[][2] = {{1, 1}, {5, 3}, {70000, 1}, {66000, 2}, {7168, 40}};
    for (auto& sh : shapes) {
        const uint64_t count = sh[0], tiles = sh[1];
        uint64_t wg = 0;
        for (uint64_t r = 0; r < count; r++)
            for (uint64_t t = 0; t < tiles; t++, wg++) CHECK(wg_replica(wg, tiles) == r && wg_tile(wg, tiles) == t);
    }
    // slices of a launch
    const uint64_t totals[] = {1, kMaxGridX - 1, kMaxGridX, kMaxGridX + 1, 3 * kMaxGridX, 3 * kMaxGridX + 7, 1ull << 40};
    for (uint64_t total : totals) {
        uint64_t sum = 0;
        for (uint64_t s = 0; s < slices_of(total); s++) {
            const uint64_t z = slice_size(total, s);
            CHECK(z >= 1 && z <= kMaxGridX && z <= 0x7FFFFFFFull);
            CHECK(s + 1 == slices_of(total) || z == kMaxGridX);
            sum += z;
        }
        CHECK(sum == total);
    }
    // offsets: 64-bit, a row may start past 2^32 bytes
    const uint64_t stride = (1ull << 28) + 1;
    for (uint64_t k : {0ull, 1ull, 99ull}) {
        CHECK(out_index(0, stride, k) == k);
        CHECK(out_index(1, stride, k) == stride + k);
        CHECK(out_index(1, stride, k) * sizeof(pu_req16) > (1ull << 32));
        CHECK(out_index(7167, 40960, k) * sizeof(pu_req) == (7167ull * 40960 + k) * 32);
    }
    CHECK(out_index(7167, 40960, 40959) * sizeof(pu_req) + sizeof(pu_req) == 7168ull * 40960 * 32);   // the bench's 9.4 GB
    // the LDS cap
    CHECK(rows_fit_lds(1) && rows_fit_lds(2560) && !rows_fit_lds(2561) && !rows_fit_lds(kMaxCores));
    for (int nc : {1, 2, 3, 48, 1030, 2560}) CHECK(rows_lds_bytes(nc) % 16 == 0 && rows_lds_bytes(nc) >= (uint64_t)nc * 8 && rows_lds_bytes(nc) < (uint64_t)nc * 8 + 16);
    return 0;
}

static int shuffles(int seeds, int* rows_out) {
    for (int nc : {1, 2, 64, 1030}) {
        std::vector<int32_t> row((size_t)nc), again((size_t)nc);
        std::vector<uint8_t> seen((size_t)nc);
        int moved = 0;
        for (int seed = 0; seed < seeds; seed++) {
            std::fill(row.begin(), row.end(), -1);
            placement_shuffle(row.data(), nc, (uint64_t)seed);
            std::fill(seen.begin(), seen.end(), 0);
            bool identity = true;
            for (int c = 0; c < nc; c++) {
                CHECK(row[(size_t)c] >= 0 && row[(size_t)c] < nc && !seen[(size_t)row[(size_t)c]]);
                seen[(size_t)row[(size_t)c]] = 1;
                identity = identity && row[(size_t)c] == c;
            }
            if (seed == 0) CHECK(identity);
            moved += identity ? 0 : 1;
            placement_shuffle(again.data(), nc, (uint64_t)seed);
            CHECK(row == again);
            ++*rows_out;
        }
        if (nc >= 64) CHECK(moved == seeds - 1);
    }
    // the stated rule, restated: Fisher-Yates from the top with SplitMix64's draws
    const int nc = 9;
    int32_t a[nc], b[nc];
    placement_shuffle(a, nc, 0xC0FFEE);
    for (int c = 0; c < nc; c++) b[c] = c;
    uint64_t s = 0xC0FFEE;
    for (int i = nc - 1; i >= 1; i--) {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const int j = (int)(z % (uint64_t)(i + 1));
        const int32_t t = b[i];
        b[i] = b[j];
        b[j] = t;
    }
    CHECK(std::memcmp(a, b, sizeof a) == 0);
    return 0;
}

int main() {
    int n_edges = 0, n_rows = 0;
    const int n_random = 100000, seeds = 1000;
    if (edges(&n_edges)) return 1;
    if (randoms(n_random)) return 1;
    uint64_t live = 0;
    const uint64_t gots[] = {0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2051, 40960, 100003};
    for (uint64_t g : gots)
        if (cover(g, &live)) return 1;
    if (folding()) return 1;
    if (shuffles(seeds, &n_rows)) return 1;
    std::printf("OK %d edge records, %d random records, %zu counts %llu tile records, %d placements\n", n_edges, n_random,
                sizeof gots / sizeof gots[0], (unsigned long long)live, n_rows);
    return 0;
}
