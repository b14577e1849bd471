// queue_header_check.cpp — the rules of the end-of-run results
// (primesim_amd/csrc/run_results_step.h) against literal arithmetic: the decode
// of a queue header's visit counts for every ring cursor value, the fold of the
// completion cycles and the tie rule of the busiest queue against sequential
// loops, the empty set included.  Host only (tests/test_dres_abi.py builds it
// with the host's address and undefined-behaviour sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/run_results_step.h"

using namespace pu_run_results;

// The engine's encoding (engine.hip: q_store_hdr): the count as a double, the
// cursor or-ed into the low dword.
static void encode(uint64_t n, uint32_t cursor, uint32_t* lo, uint32_t* hi) {
    const double d = (double)n;
    uint64_t bits;
    std::memcpy(&bits, &d, sizeof bits);
    *lo = (uint32_t)bits | cursor;
    *hi = (uint32_t)(bits >> 32);
}

static bool decode_ok(uint64_t n, uint32_t cursor) {
    uint32_t lo, hi;
    encode(n, cursor, &lo, &hi);
    const uint64_t got = count_of(lo, hi);
    if (got != n) std::printf("FAIL decode n %llu cursor %u: got %llu\n", (unsigned long long)n, cursor, (unsigned long long)got);
    return got == n;
}

static bool same(const Completion& a, const Completion& b) {
    return a.done == b.done && a.max == b.max && a.min == b.min && a.sum == b.sum;
}

int main() {
    if (kHdrBytes != 32 || kHdrCursor != 0x7Fu || kNoCycle != -1) {
        std::printf("FAIL constants\n");
        return 1;
    }
    long checked = 0;
    const uint64_t edges[] = {0, 1, 127, 128, (1ull << 32) - 1, (1ull << 32) + 1, (1ull << 45) - 1};
    for (uint64_t n : edges)
        for (uint32_t cur = 0; cur < 128; cur++) {
            if (!decode_ok(n, cur)) return 1;
            checked++;
        }
    std::mt19937_64 rng(20240607);
    for (int i = 0; i < 100000; i++) {
        // half of the draws shifted down so that small counts are met too
        uint64_t n = rng() & ((1ull << 45) - 1);
        if (i & 1) n >>= rng() % 45;
        if (!decode_ok(n, (uint32_t)(rng() & 127))) return 1;
        checked++;
    }

    // the completion fold: any split merged equals the sequential loop; idle cores do not count
    {
        Completion e = completion_init();
        if (e.done != 0 || e.max != INT64_MIN || e.min != INT64_MAX || e.sum != 0) {
            std::printf("FAIL completion_init\n");
            return 1;
        }
        Completion idle = completion_init();
        for (int i = 0; i < 9; i++) completion_fold(idle, kNoCycle);
        if (!same(idle, e)) {
            std::printf("FAIL idle cores\n");
            return 1;
        }
        std::vector<int64_t> cyc = {kNoCycle, 0, 5, kNoCycle, INT64_MAX, -2, INT64_MIN, 7, 7, kNoCycle, 1ll << 40};
        for (int i = 0; i < 1000; i++) cyc.push_back((i % 7 == 0) ? kNoCycle : (int64_t)(rng() >> (rng() % 64)));
        int32_t done = 0;
        int64_t mx = INT64_MIN, mn = INT64_MAX;
        uint64_t sum = 0;
        for (int64_t c : cyc) {
            if (c == -1) continue;
            done++;
            if (c > mx) mx = c;
            if (c < mn) mn = c;
            sum += (uint64_t)c;
        }
        const Completion want{done, mx, mn, (int64_t)sum};
        for (size_t parts : {(size_t)1, (size_t)3, (size_t)4, (size_t)256}) {
            std::vector<Completion> p(parts, completion_init());
            for (size_t k = 0; k < cyc.size(); k++) completion_fold(p[k % parts], cyc[k]);
            Completion all = completion_init();
            for (size_t k = parts; k-- > 0;) completion_merge(all, p[k]);   // any order
            if (!same(all, want)) {
                std::printf("FAIL completion fold in %zu parts\n", parts);
                return 1;
            }
        }
    }

    // the busiest queue: the largest count, the lowest id among equals, -1 for the empty range
    {
        Busiest e = busiest_init();
        if (e.id != -1 || e.visits != 0) {
            std::printf("FAIL busiest_init\n");
            return 1;
        }
        Busiest z = busiest_init();
        for (int32_t id = 24; id < 30; id++) busiest_take(z, 0, id);   // none visited: 0 at the lowest id
        Busiest m = z;
        busiest_take(m, 0, -1);                                        // "no queue" never wins
        busiest_take(m, 99, -1);
        if (z.id != 24 || z.visits != 0 || m.id != 24 || m.visits != 0) {
            std::printf("FAIL busiest of unvisited queues\n");
            return 1;
        }
        for (int round = 0; round < 200; round++) {
            const int nq = 1 + (int)(rng() % 300);
            std::vector<uint64_t> v((size_t)nq);
            for (auto& x : v) x = rng() % (round % 2 ? 4 : 1000);      // many ties every other round
            int32_t want_id = -1;
            uint64_t want_v = 0;
            for (int q = 0; q < nq; q++)
                if (want_id < 0 || v[(size_t)q] > want_v) {
                    want_id = q;
                    want_v = v[(size_t)q];
                }
            // lanes take strided queues, the lanes then meet in a butterfly, as the kernel does
            Busiest lane[64];
            for (auto& b : lane) b = busiest_init();
            for (int q = nq; q-- > 0;) busiest_take(lane[q % 64], v[(size_t)q], q);
            for (int step = 32; step >= 1; step >>= 1) {
                Busiest next[64];
                for (int l = 0; l < 64; l++) {
                    next[l] = lane[l];
                    busiest_take(next[l], lane[l ^ step].visits, lane[l ^ step].id);
                }
                for (int l = 0; l < 64; l++) lane[l] = next[l];
            }
            for (int l = 0; l < 64; l++)
                if (lane[l].id != want_id || lane[l].visits != want_v) {
                    std::printf("FAIL busiest round %d lane %d: (%llu, %d), expected (%llu, %d)\n", round, l,
                                (unsigned long long)lane[l].visits, lane[l].id, (unsigned long long)want_v, want_id);
                    return 1;
                }
        }
    }
    std::printf("OK %ld headers\n", checked);
    return 0;
}
