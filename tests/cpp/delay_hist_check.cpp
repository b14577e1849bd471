// delay_hist_check.cpp — the rule of the log-linear delay histograms
// (primesim_amd/csrc/delay_hist_step.h) against plain statements of it: bucket_of
// against a loop of comparisons over the 864 bounds, at every bucket edge and on 10^6
// random int32; the bounds as the inverse of bucket_of; the coarse fold against the
// delay summaries' bucket; the rank rule against unsigned __int128 arithmetic; and the
// quantile walk against a sequential scan.  Host only (tests/test_dhist_abi.py builds
// it with the host's address and undefined-behaviour sanitizers).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/delay_hist_step.h"

using namespace pu_delay_hist;

static int64_t g_lo[PU_DHIST_BUCKETS], g_hi[PU_DHIST_BUCKETS];

// the bounds from the definition: a bucket per value below 64, then octaves in 32 equal parts
static void build_bounds() {
    g_lo[0] = INT32_MIN;
    g_hi[0] = 0;
    int k = 1;
    for (; k < 64; k++) g_lo[k] = g_hi[k] = k;
    for (int o = 6; o <= 30; o++) {
        const int64_t width = ((int64_t)1 << o) / 32;
        for (int part = 0; part < 32; part++, k++) {
            g_lo[k] = ((int64_t)1 << o) + part * width;
            g_hi[k] = g_lo[k] + width - 1;
        }
    }
}

// by comparisons only
static int bucket_by_comparisons(int32_t d) {
    for (int k = 0; k < PU_DHIST_BUCKETS; k++)
        if ((int64_t)d >= g_lo[k] && (int64_t)d <= g_hi[k]) return k;
    return -1;
}

static uint64_t rank_by_int128(uint64_t count, uint32_t ppm) {
    const unsigned __int128 p = (unsigned __int128)count * ppm;
    const unsigned __int128 r = (p + 999999u) / 1000000u;
    return r ? (uint64_t)r : 1;
}

static int walk_sequential(const std::vector<uint64_t>& h, uint32_t ppm) {
    unsigned __int128 n = 0;
    for (uint64_t v : h) n += v;
    if (n == 0) return -1;
    const uint64_t rank = rank_by_int128((uint64_t)n, ppm);
    unsigned __int128 run = 0;
    for (int k = 0; k < PU_DHIST_BUCKETS; k++) {
        run += h[(size_t)k];
        if (run >= rank) return k;
    }
    return -1;
}

int main() {
    build_bounds();
    long checked = 0;

    // the bounds tile [INT32_MIN, INT32_MAX], each bucket from 64 on is at most lo / 32 wide
    if (g_hi[PU_DHIST_BUCKETS - 1] != INT32_MAX) {
        std::printf("FAIL the last bucket ends at %lld\n", (long long)g_hi[PU_DHIST_BUCKETS - 1]);
        return 1;
    }
    for (int k = 1; k < PU_DHIST_BUCKETS; k++)
        if (g_lo[k] != g_hi[k - 1] + 1 || (k >= 64 && (g_hi[k] - g_lo[k] + 1) * 32 > g_lo[k])) {
            std::printf("FAIL bounds of bucket %d\n", k);
            return 1;
        }

    // every edge: lo - 1, lo, hi, hi + 1 of every bucket, and the values the header names
    std::vector<int32_t> edges = {INT32_MIN, -1, 0, INT32_MAX};
    for (int k = 0; k < PU_DHIST_BUCKETS; k++)
        for (int64_t v : {g_lo[k] - 1, g_lo[k], g_hi[k], g_hi[k] + 1})
            if (v >= INT32_MIN && v <= INT32_MAX) edges.push_back((int32_t)v);
    for (int32_t d : edges) {
        if (bucket_of(d) != bucket_by_comparisons(d)) {
            std::printf("FAIL edge %d: bucket_of %d, comparisons %d\n", d, bucket_of(d), bucket_by_comparisons(d));
            return 1;
        }
        checked++;
    }
    const struct { int32_t d; int b; } table[] = {{INT32_MIN, 0}, {-1, 0}, {0, 0}, {1, 1}, {63, 63}, {64, 64}, {65, 64},
                                                  {66, 65}, {127, 95}, {128, 96}, {131, 96}, {132, 97}, {INT32_MAX, 863}};
    for (const auto& t : table)
        if (bucket_of(t.d) != t.b) {
            std::printf("FAIL table %d: bucket_of %d, expected %d\n", t.d, bucket_of(t.d), t.b);
            return 1;
        }
    std::mt19937 rng(12345);
    for (int i = 0; i < 1000000; i++) {
        const int32_t d = (int32_t)rng();
        // half of the draws shifted down so that every octave is met, not only the top ones
        const int32_t v = (i & 1) ? d : (int32_t)(d >> (rng() % 32));
        const int b = bucket_of(v);
        if (b < 0 || b >= PU_DHIST_BUCKETS || b != bucket_by_comparisons(v)) {
            std::printf("FAIL random %d: bucket_of %d, comparisons %d\n", v, b, bucket_by_comparisons(v));
            return 1;
        }
        // the fine bucket lies inside the delay summaries' bucket of the same delay
        if (coarse_of(b) != pu_delay_sum::bucket_of(v)) {
            std::printf("FAIL coarse random %d: fine %d -> %d, pu_dsum %d\n", v, b, coarse_of(b), pu_delay_sum::bucket_of(v));
            return 1;
        }
        checked++;
    }

    // the bounds are the inverse of bucket_of, and the coarse fold is the delay summaries' bucket of both ends
    for (int k = 0; k < PU_DHIST_BUCKETS; k++) {
        int32_t lo = 1, hi = -1;
        bucket_bounds(k, &lo, &hi);
        if (lo != g_lo[k] || hi != g_hi[k] || bucket_of(lo) != k || bucket_of(hi) != k) {
            std::printf("FAIL bounds of %d: [%d, %d], expected [%lld, %lld]\n", k, lo, hi, (long long)g_lo[k], (long long)g_hi[k]);
            return 1;
        }
        if (coarse_of(k) != pu_delay_sum::bucket_of(lo) || coarse_of(k) != pu_delay_sum::bucket_of(hi)) {
            std::printf("FAIL coarse of %d: %d, pu_dsum %d .. %d\n", k, coarse_of(k), pu_delay_sum::bucket_of(lo),
                        pu_delay_sum::bucket_of(hi));
            return 1;
        }
    }

    // the rank rule
    const uint64_t counts[] = {0, 1, 2, 999999, 1000000, 1000001, 1ull << 32, 1ull << 44, 1ull << 63, UINT64_MAX};
    const uint32_t ppms[] = {0, 1, 500000, 990000, 999999, 1000000};
    for (uint64_t c : counts)
        for (uint32_t p : ppms)
            if (rank_of(c, p) != rank_by_int128(c, p)) {
                std::printf("FAIL rank_of(%llu, %u) = %llu, expected %llu\n", (unsigned long long)c, p,
                            (unsigned long long)rank_of(c, p), (unsigned long long)rank_by_int128(c, p));
                return 1;
            }
    for (int i = 0; i < 100000; i++) {
        const uint64_t c = (((uint64_t)rng() << 32) | rng()) >> (rng() % 64);
        const uint32_t p = rng() % 1000001u;
        if (rank_of(c, p) != rank_by_int128(c, p)) {
            std::printf("FAIL rank_of(%llu, %u)\n", (unsigned long long)c, p);
            return 1;
        }
    }
    if (rank_of(1000000, 1) != 1 || rank_of(1000001, 1) != 2 || rank_of(0, 1000000) != 1 || rank_of(7, 0) != 1 ||
        rank_of(1ull << 63, 1000000) != 1ull << 63) {
        std::printf("FAIL rank_of on the values spelled out\n");
        return 1;
    }

    // the quantile walk: random sparse histograms, a one-bucket class, an empty class
    const uint32_t qs[] = {0, 1, 500000, 900000, 990000, 999000, 999999, 1000000};
    for (int round = 0; round < 300; round++) {
        std::vector<uint64_t> h(PU_DHIST_BUCKETS, 0);
        const int filled = round == 0 ? 0 : round == 1 ? 1 : 1 + (int)(rng() % 40);
        for (int f = 0; f < filled; f++) h[rng() % PU_DHIST_BUCKETS] += (round % 3 == 0) ? ((uint64_t)rng() << 20) : 1 + rng() % 1000;
        const uint64_t n = class_count(h.data());
        for (uint32_t p : qs) {
            const int got = quantile_bucket(h.data(), n, p), want = walk_sequential(h, p);
            if (got != want) {
                std::printf("FAIL quantile walk, round %d, ppm %u: %d, expected %d\n", round, p, got, want);
                return 1;
            }
            if (filled == 0 && got != -1) {
                std::printf("FAIL an empty class answers %d\n", got);
                return 1;
            }
        }
    }
    // the class's first and last bucket answer ppm 0 and 10^6
    {
        std::vector<uint64_t> h(PU_DHIST_BUCKETS, 0);
        h[13] = 1;
        h[500] = 5;
        h[863] = 1;
        if (quantile_bucket(h.data(), 7, 0) != 13 || quantile_bucket(h.data(), 7, 1000000) != 863 ||
            quantile_bucket(h.data(), 7, 500000) != 500 || key_of(1, INT32_MAX) != 2 * PU_DHIST_BUCKETS - 1 || key_of(0, -3) != 0) {
            std::printf("FAIL quantiles of a three-bucket class\n");
            return 1;
        }
    }
    std::printf("OK %ld delays\n", checked);
    return 0;
}
