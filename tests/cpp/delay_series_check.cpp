// delay_series_check.cpp — the rule of the epoch series
// (primesim_amd/csrc/delay_series_step.h) against plain statements of it: epoch_of
// against the definition in 128-bit integers at every epoch edge (t0 - 1, t0,
// t0 + 2^shift - 1, t0 + 2^shift, the last epoch's first cycle and the one before it,
// INT64_MIN and INT64_MAX) for t0 = INT64_MIN, 0, INT64_MAX and some between, the
// shifts 0, 1, 40, 62 and E = 1, 2, 512; fold_one against a count, a 128-bit sum, a
// count of the non-positive and a maximum taken over the delays kept; merge against
// folding both halves into one cell; and folding a stream chunk by chunk against folding
// it whole, in both record formats.  Host only (tests/test_dseries_abi.py builds it with
// the host's address and undefined-behaviour sanitizers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/delay_series_step.h"

using namespace pu_delay_series;
typedef __int128 i128;

static bool same(const pu_dseries_cell& a, const pu_dseries_cell& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the definition, in integers wide enough for any distance
static int plain_epoch(int64_t timer, int E, int64_t t0, int shift) {
    if (timer < t0) return 0;
    const i128 e = ((i128)timer - (i128)t0) >> shift;
    return e < (i128)(E - 1) ? (int)e : E - 1;
}

static pu_dseries_cell plain_cell(const std::vector<int32_t>& ds) {
    pu_dseries_cell c = {};
    i128 sum = 0;
    for (int32_t d : ds) {
        c.count++;
        sum += d;
        if (d <= 0) c.nonpos++;
        c.max = std::max(c.max, std::max(d, (int32_t)0));
    }
    c.sum = (int64_t)sum;
    return c;
}

int main() {
    long checked = 0;

    const int64_t t0s[] = {INT64_MIN, INT64_MIN + 1, -1000, -1, 0, 1, 500, (int64_t)1 << 40, INT64_MAX - 1, INT64_MAX};
    const int shifts[] = {0, 1, 40, 62};
    const int Es[] = {1, 2, 512};
    for (int64_t t0 : t0s)
        for (int shift : shifts)
            for (int E : Es) {
                const i128 width = (i128)1 << shift, last = (i128)t0 + (i128)(E - 1) * width;
                const i128 edges[] = {(i128)t0 - 1, t0, (i128)t0 + width - 1, (i128)t0 + width, last - 1, last, last + 1,
                                      (i128)t0 + 3 * width, INT64_MIN, INT64_MAX, 0, -1};
                for (i128 t : edges) {
                    if (t < INT64_MIN || t > INT64_MAX) continue;
                    const int got = epoch_of((int64_t)t, E, t0, shift), want = plain_epoch((int64_t)t, E, t0, shift);
                    if (got != want || got < 0 || got >= E) {
                        std::printf("FAIL epoch_of(%lld, E %d, t0 %lld, shift %d) = %d, expected %d\n", (long long)t, E,
                                    (long long)t0, shift, got, want);
                        return 1;
                    }
                    checked++;
                }
                // what the edges mean
                if (epoch_of(t0, E, t0, shift) != 0 || (t0 > INT64_MIN && epoch_of(t0 - 1, E, t0, shift) != 0) ||
                    epoch_of(INT64_MIN, E, t0, shift) != 0) {
                    std::printf("FAIL epoch 0 does not hold t0, t0 - 1 and INT64_MIN (t0 %lld)\n", (long long)t0);
                    return 1;
                }
                if (last <= INT64_MAX && E > 1) {
                    if (epoch_of((int64_t)last, E, t0, shift) != E - 1 || epoch_of((int64_t)(last - 1), E, t0, shift) != E - 2 ||
                        epoch_of(INT64_MAX, E, t0, shift) != E - 1) {
                        std::printf("FAIL the last epoch's first cycle (t0 %lld, shift %d, E %d)\n", (long long)t0, shift, E);
                        return 1;
                    }
                    checked++;
                }
            }
    if (epoch_of(INT64_MAX, 512, INT64_MIN, 62) != 3 || epoch_of(INT64_MAX, 512, INT64_MIN, 0) != 511 ||
        epoch_of(INT64_MAX, 2, INT64_MAX, 0) != 0 || epoch_of(INT64_MIN, 512, INT64_MAX, 0) != 0) {
        std::printf("FAIL the extremes\n");
        return 1;
    }

    // random timers against the definition
    std::mt19937_64 rng(2025);
    for (int i = 0; i < 200000; i++) {
        const int shift = (int)(rng() % 63), E = 1 + (int)(rng() % PU_DSERIES_MAX_EPOCHS);
        const int64_t t0 = (int64_t)rng() >> (rng() % 64), timer = (int64_t)rng() >> (rng() % 64);
        if (epoch_of(timer, E, t0, shift) != plain_epoch(timer, E, t0, shift)) {
            std::printf("FAIL epoch_of(%lld, E %d, t0 %lld, shift %d)\n", (long long)timer, E, (long long)t0, shift);
            return 1;
        }
        checked++;
    }

    // fold_one and merge against plain statements
    const int32_t edge[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7000, INT32_MAX - 1, INT32_MAX};
    for (int round = 0; round < 2000; round++) {
        const int n = (int)(rng() % 200), kind = (int)(rng() % 4);
        std::vector<int32_t> a, b;
        pu_dseries_cell ca = {}, cb = {}, call = {};
        for (int i = 0; i < n; i++) {
            const int32_t d = kind == 0   ? edge[rng() % 8]
                              : kind == 1 ? INT32_MAX
                              : kind == 2 ? INT32_MIN
                                          : (int32_t)(uint32_t)rng();
            const bool first = rng() & 1;
            (first ? a : b).push_back(d);
            fold_one(first ? &ca : &cb, d);
            fold_one(&call, d);
        }
        std::vector<int32_t> all(a);
        all.insert(all.end(), b.begin(), b.end());
        pu_dseries_cell m = ca;
        merge(&m, cb);
        if (!same(ca, plain_cell(a)) || !same(cb, plain_cell(b)) || !same(call, plain_cell(all)) || !same(m, call)) {
            std::printf("FAIL fold_one / merge round %d\n", round);
            return 1;
        }
        checked++;
    }
    {   // an empty cell is zeros, and only non-positive delays leave max 0
        pu_dseries_cell c = {};
        fold_one(&c, -5);
        fold_one(&c, 0);
        fold_one(&c, INT32_MIN);
        if (c.count != 3 || c.nonpos != 3 || c.max != 0 || c.sum != (int64_t)INT32_MIN - 5 || c._pad != 0) {
            std::printf("FAIL non-positive delays\n");
            return 1;
        }
    }

    // chunked folding against whole folding, both formats; only PU_WR is a write
    for (int round = 0; round < 200; round++) {
        const int E = round % 3 == 0 ? 1 : round % 3 == 1 ? 1 + (int)(rng() % PU_DSERIES_MAX_EPOCHS) : 7;
        const int shift = (int)(rng() % 12);
        const int64_t t0 = (int64_t)(rng() % 3000) - 1000;
        const size_t n = rng() % 700;
        std::vector<pu_req> r32(n);
        std::vector<pu_req16> r16(n);
        std::vector<int32_t> delays(n);
        if (n) std::memset(r32.data(), 0, n * sizeof(pu_req));
        for (size_t i = 0; i < n; i++) {
            r32[i].timer = (int64_t)(rng() % 100000);
            r32[i].core = (int32_t)(rng() % 70);
            r32[i].prog_id = 1;
            const uint8_t types[] = {PU_RD, PU_WR, PU_WB, 3, 255};
            r32[i].mem_type = round % 4 == 3 ? types[rng() % 5] : (uint8_t)(rng() % 2);
            r16[i].a = 0;
            r16[i].b = PU_REQ16_B(r32[i].timer, r32[i].core, 1, r32[i].mem_type == PU_WR ? 1 : 0, 0);
            delays[i] = round % 5 == 0 ? (int32_t)(rng() % 3) - 1 : (int32_t)((uint32_t)rng() >> (rng() % 32));
        }
        std::vector<pu_dseries_cell> whole((size_t)2 * E), parts((size_t)2 * E), packed((size_t)2 * E), plain((size_t)2 * E);
        fold(whole.data(), E, t0, shift, r32.data(), PU_REQ_FMT_32, delays.data(), n);
        fold(packed.data(), E, t0, shift, r16.data(), PU_REQ_FMT_16, delays.data(), n);
        for (size_t at = 0; at < n;) {
            const size_t step = std::min(n - at, (size_t)(rng() % 130));
            fold(parts.data(), E, t0, shift, r32.data() + at, PU_REQ_FMT_32, delays.data() + at, step);
            at += step;
        }
        std::vector<std::vector<int32_t>> kept((size_t)2 * E);
        for (size_t i = 0; i < n; i++)
            kept[(size_t)(r32[i].mem_type == PU_WR ? E : 0) + (size_t)plain_epoch(r32[i].timer, E, t0, shift)].push_back(delays[i]);
        uint64_t total = 0;
        for (size_t k = 0; k < (size_t)2 * E; k++) {
            plain[k] = plain_cell(kept[k]);
            total += whole[k].count;
            if (!same(whole[k], plain[k]) || !same(whole[k], parts[k]) || !same(whole[k], packed[k])) {
                std::printf("FAIL fold round %d: cell %zu (plain, chunked or pu_req16 vs whole)\n", round, k);
                return 1;
            }
        }
        if (total != n) {
            std::printf("FAIL fold round %d: %llu records in the cells of %zu\n", round, (unsigned long long)total, n);
            return 1;
        }
        checked++;
    }
    std::printf("OK %ld checks\n", checked);
    return 0;
}
