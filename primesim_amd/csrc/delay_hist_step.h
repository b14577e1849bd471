// delay_hist_step.h — the rule of the log-linear delay histograms (pu_dhist_*,
// include/primeuncore.h), shared by the host fold (pu_dhist_host_add,
// pu_dhist_host_quantiles) and the device kernels (delay_hist.hip): a delay's
// fine bucket and its inverse, the fold of a fine bucket down to the power-of-two
// bucket of the delay summaries, the rank of a quantile and the walk that answers
// it.  A record's class is delay_record_step.h's.
// Everything here compiles as plain C++ on the host (PU_HD is empty there) and as
// __host__ __device__ under hipcc's HIP mode.  All of it is integer and
// independent of order, so any split of the work gives the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/primeuncore.h"
#include "delay_record_step.h"
#include "delay_sum_step.h"   // pu_delay_sum::bucket_of, the bucket coarse_of folds down to
#include "pu_hd.h"

namespace pu_delay_hist {

constexpr int kSub = 1 << PU_DHIST_SUB_BITS;        // 32 sub-buckets per octave
constexpr int kExact = 2 * kSub;                    // delays below 64 have a bucket each
constexpr uint32_t kPpmOne = 1000000u;
static_assert(PU_DHIST_BUCKETS == kExact + (31 - (PU_DHIST_SUB_BITS + 1)) * kSub, "octaves 6..30, 32 buckets each");

// d <= 0 -> 0; 1 <= d < 64 -> d; otherwise the octave o = 31 - clz(d) (6..30) cut
// into 32 equal parts: 64 + (o - 6) * 32 + ((d >> (o - 5)) - 32).  INT32_MAX -> 863.
PU_HD inline int bucket_of(int32_t d) {
    if (d < kExact) return d <= 0 ? 0 : d;
    const int o = 31 - __builtin_clz((uint32_t)d);
    return kExact + (o - (PU_DHIST_SUB_BITS + 1)) * kSub + (int)(((uint32_t)d >> (o - PU_DHIST_SUB_BITS)) - (uint32_t)kSub);
}

// The delays bucket k (0 .. PU_DHIST_BUCKETS - 1) holds: [*lo, *hi], both inclusive.
PU_HD inline void bucket_bounds(int k, int32_t* lo, int32_t* hi) {
    if (k <= 0) {
        *lo = INT32_MIN;
        *hi = 0;
    } else if (k < kExact) {
        *lo = *hi = k;
    } else {
        const int j = k - kExact, sh = 1 + j / kSub;           // sh = o - 5
        const uint32_t m = (uint32_t)(kSub + j % kSub);
        *lo = (int32_t)(m << sh);
        *hi = (int32_t)(((m + 1) << sh) - 1u);                 // the last bucket: 2^31 - 1
    }
}

// The bucket of the delay summaries (pu_delay_sum::bucket_of) that contains fine bucket k.
PU_HD inline int coarse_of(int k) {
    if (k <= 0) return 0;
    if (k < kExact) return 32 - __builtin_clz((uint32_t)k);
    return (PU_DHIST_SUB_BITS + 2) + (k - kExact) / kSub;      // o + 1
}

// The high half of a 64 x 64 -> 128-bit product: one function for both sides.
PU_HD inline uint64_t mul_hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Nearest rank: max(1, ceil(count * ppm / 10^6)) for ppm <= 10^6, exactly.  The
// product's high half is below 10^6 < 2^20, so dividing it by 10^6 takes two steps
// of a 52-bit dividend.
PU_HD inline uint64_t rank_of(uint64_t count, uint32_t ppm) {
    const uint64_t lo = count * (uint64_t)ppm, hi = mul_hi(count, (uint64_t)ppm);
    const uint64_t a = (hi << 32) | (lo >> 32);
    const uint64_t b = ((a % kPpmOne) << 32) | (lo & 0xFFFFFFFFull);
    const uint64_t q = ((a / kPpmOne) << 32) | (b / kPpmOne);
    const uint64_t rank = q + (b % kPpmOne ? 1u : 0u);
    return rank ? rank : 1;
}

PU_HD inline uint64_t class_count(const uint64_t* hist) {
    uint64_t n = 0;
    for (int k = 0; k < PU_DHIST_BUCKETS; k++) n += hist[k];
    return n;
}

// The lowest bucket whose inclusive running count reaches `rank` (1 .. the class's count).
PU_HD inline int bucket_at_rank(const uint64_t* hist, uint64_t rank) {
    uint64_t run = 0;
    for (int k = 0; k < PU_DHIST_BUCKETS; k++) {
        run += hist[k];
        if (run >= rank) return k;
    }
    return -1;   // rank beyond the count: an empty class
}

// The quantile `ppm` of one class's histogram: its bucket, or -1 for an empty class.
PU_HD inline int quantile_bucket(const uint64_t* hist, uint64_t count, uint32_t ppm) {
    return count ? bucket_at_rank(hist, rank_of(count, ppm)) : -1;
}

// The counter of (class, bucket) in a replica's uint64_t hist[2][PU_DHIST_BUCKETS].
PU_HD inline int key_of(int cls, int32_t d) { return cls * PU_DHIST_BUCKETS + bucket_of(d); }

}  // namespace pu_delay_hist
