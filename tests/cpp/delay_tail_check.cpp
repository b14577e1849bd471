// delay_tail_check.cpp — the rule of the slowest-request lists
// (primesim_amd/csrc/delay_tail_step.h) against plain statements of it: the order
// predicate is a strict total order on a grid of edge values; sorted insertion equals
// std::stable_sort of everything offered plus truncation, on 10^5 random sequences;
// and folding a stream chunk by chunk equals folding it whole, in both record formats.
// Host only (tests/test_dtail_abi.py builds it with the host's address and
// undefined-behaviour sanitizers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/delay_tail_step.h"

using namespace pu_delay_tail;

static bool same(const pu_dtail_entry& a, const pu_dtail_entry& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// delay descending by stable_sort over entries given in ascending position: equal delays keep their order
static std::vector<pu_dtail_entry> by_stable_sort(std::vector<pu_dtail_entry> v, int k) {
    std::stable_sort(v.begin(), v.end(), [](const pu_dtail_entry& a, const pu_dtail_entry& b) { return a.delay > b.delay; });
    if (v.size() > (size_t)k) v.resize((size_t)k);
    return v;
}

int main() {
    long checked = 0;

    // a strict total order on the grid: irreflexive, exactly one way between two different keys, transitive
    const int32_t ds[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7000, INT32_MAX - 1, INT32_MAX};
    const uint64_t ps[] = {0, 1, 2, 1ull << 31, 1ull << 32, (1ull << 63) - 1, 1ull << 63, UINT64_MAX};
    struct Key { int32_t d; uint64_t p; };
    std::vector<Key> grid;
    for (int32_t d : ds)
        for (uint64_t p : ps) grid.push_back({d, p});
    for (const Key& x : grid) {
        if (better(x.d, x.p, x.d, x.p)) {
            std::printf("FAIL better(x, x) at (%d, %llu)\n", x.d, (unsigned long long)x.p);
            return 1;
        }
        for (const Key& y : grid) {
            const bool xy = better(x.d, x.p, y.d, y.p), yx = better(y.d, y.p, x.d, x.p);
            const bool differ = x.d != y.d || x.p != y.p;
            if ((xy && yx) || (differ && !xy && !yx)) {
                std::printf("FAIL not exactly one way between (%d, %llu) and (%d, %llu)\n", x.d, (unsigned long long)x.p, y.d,
                            (unsigned long long)y.p);
                return 1;
            }
            // the definition, spelled out in wider integers
            if (xy != ((int64_t)x.d > (int64_t)y.d || (x.d == y.d && x.p < y.p))) {
                std::printf("FAIL the definition at (%d, %llu), (%d, %llu)\n", x.d, (unsigned long long)x.p, y.d,
                            (unsigned long long)y.p);
                return 1;
            }
            for (const Key& z : grid)
                if (xy && better(y.d, y.p, z.d, z.p) && !better(x.d, x.p, z.d, z.p)) {
                    std::printf("FAIL not transitive\n");
                    return 1;
                }
            checked++;
        }
    }

    // sorted insertion against stable_sort plus truncation
    std::mt19937 rng(2024);
    for (int round = 0; round < 100000; round++) {
        const int k = round % 3 == 0 ? 1 + (int)(rng() % PU_DTAIL_MAX_K) : round % 3 == 1 ? 5 : (round % 2 ? 1 : PU_DTAIL_MAX_K);
        const int n = (int)(rng() % 90);
        const int kind = (int)(rng() % 5);   // few values (ties), all equal, ascending, descending, anything
        const uint64_t at = round % 7 == 0 ? UINT64_MAX - 200 : rng() % 1000;
        std::vector<pu_dtail_entry> all;
        pu_dtail_entry list[PU_DTAIL_MAX_K];
        std::memset(list, 0, sizeof list);
        uint32_t count = 0;
        for (int i = 0; i < n; i++) {
            int32_t d;
            switch (kind) {
                case 0: d = (int32_t)(rng() % 4) - 1; break;
                case 1: d = INT32_MIN; break;
                case 2: d = INT32_MAX - n + i; break;
                case 3: d = INT32_MIN + n - i; break;
                default: d = (int32_t)rng(); break;
            }
            const pu_dtail_entry e = {rng(), (int64_t)rng(), at + (uint64_t)i, d, (int32_t)(rng() % 70)};
            all.push_back(e);
            insert(list, &count, k, e);
        }
        const std::vector<pu_dtail_entry> want = by_stable_sort(all, k);
        if (count != want.size()) {
            std::printf("FAIL round %d: count %u, expected %zu\n", round, count, want.size());
            return 1;
        }
        for (size_t j = 0; j < want.size(); j++)
            if (!same(list[j], want[j])) {
                std::printf("FAIL round %d (k %d, n %d, kind %d): entry %zu\n", round, k, n, kind, j);
                return 1;
            }
        for (int j = (int)count; j < PU_DTAIL_MAX_K; j++) {
            const pu_dtail_entry zero = {};
            if (!same(list[j], zero)) {
                std::printf("FAIL round %d: entry %d past the count was written\n", round, j);
                return 1;
            }
        }
        checked++;
    }

    // chunked folding against whole folding, both formats; only PU_WR is a write
    for (int round = 0; round < 200; round++) {
        const int k = round % 2 ? 5 : 1 + (int)(rng() % PU_DTAIL_MAX_K);
        const size_t n = rng() % 700;
        std::vector<pu_req> r32(n);
        std::vector<pu_req16> r16(n);
        std::vector<int32_t> delays(n);
        std::memset(r32.data(), 0, n * sizeof(pu_req));
        for (size_t i = 0; i < n; i++) {
            r32[i].addr = ((uint64_t)rng() << 8) | rng() % 256;
            r32[i].timer = (int64_t)(rng() % 100000);
            r32[i].core = (int32_t)(rng() % 70);
            r32[i].prog_id = 1;
            const uint8_t types[] = {PU_RD, PU_WR, PU_WB, 3, 255};
            r32[i].mem_type = round % 4 == 3 ? types[rng() % 5] : (uint8_t)(rng() % 2);
            r16[i].a = r32[i].addr;
            r16[i].b = PU_REQ16_B(r32[i].timer, r32[i].core, 1, r32[i].mem_type == PU_WR ? 1 : 0, 0);
            delays[i] = round % 5 == 0 ? (int32_t)(rng() % 3) : (int32_t)(rng() >> (rng() % 32));
        }
        std::vector<pu_dtail_entry> whole((size_t)2 * k), parts((size_t)2 * k), packed((size_t)2 * k);
        uint32_t cw[2] = {0, 0}, cp[2] = {0, 0}, c16[2] = {0, 0};
        uint64_t sw = 0, sp = 0, s16 = 0;
        fold(whole.data(), cw, &sw, k, r32.data(), PU_REQ_FMT_32, delays.data(), n);
        fold(packed.data(), c16, &s16, k, r16.data(), PU_REQ_FMT_16, delays.data(), n);
        for (size_t at = 0; at < n;) {
            const size_t step = std::min(n - at, (size_t)(rng() % 130));
            fold(parts.data(), cp, &sp, k, r32.data() + at, PU_REQ_FMT_32, delays.data() + at, step);
            at += step;
        }
        if (sw != n || sp != n || s16 != n || cw[0] != cp[0] || cw[1] != cp[1] || cw[0] != c16[0] || cw[1] != c16[1]) {
            std::printf("FAIL fold round %d: counts or seen differ\n", round);
            return 1;
        }
        size_t writes = 0;
        for (size_t i = 0; i < n; i++) writes += r32[i].mem_type == PU_WR;
        if (cw[1] != std::min(writes, (size_t)k) || cw[0] != std::min(n - writes, (size_t)k)) {
            std::printf("FAIL fold round %d: %u reads and %u writes kept of %zu and %zu\n", round, cw[0], cw[1], n - writes, writes);
            return 1;
        }
        for (size_t j = 0; j < (size_t)2 * k; j++)
            if (!same(whole[j], parts[j]) || !same(whole[j], packed[j])) {
                std::printf("FAIL fold round %d: entry %zu (chunked or pu_req16 vs whole)\n", round, j);
                return 1;
            }
        checked++;
    }
    std::printf("OK %ld checks\n", checked);
    return 0;
}
