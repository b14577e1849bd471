// delay_bucket_check.cpp — the bucket rule of the delay summaries
// (primesim_amd/csrc/delay_sum_step.h: bucket_of) against a loop of comparisons,
// at every bucket edge and on 10^6 random int32; and fold_one / replica_init on the
// edge values against sums kept by hand.  Host only (tests/test_dsum_abi.py builds
// it with the host's address and undefined-behaviour sanitizers).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/delay_sum_step.h"

using namespace pu_delay_sum;

// 0 for d <= 0, else the k in 1..31 with 2^(k-1) <= d < 2^k, by comparisons only
static int bucket_by_comparisons(int32_t d) {
    if (d <= 0) return 0;
    int k = 1;
    while (k < 31 && (int64_t)d >= ((int64_t)1 << k)) k++;
    return k;
}

int main() {
    std::vector<int32_t> edges = {INT32_MIN, -1, 0, 1, 2, 3, 4, INT32_MAX};
    for (int k = 1; k <= 30; k++) {
        edges.push_back((int32_t)(((int64_t)1 << k) - 1));
        edges.push_back((int32_t)((int64_t)1 << k));
    }
    long checked = 0;
    for (int32_t d : edges) {
        if (bucket_of(d) != bucket_by_comparisons(d)) {
            std::printf("FAIL edge %d: bucket_of %d, comparisons %d\n", d, bucket_of(d), bucket_by_comparisons(d));
            return 1;
        }
        checked++;
    }
    // the table of the header comment, spelled out
    const struct { int32_t d; int b; } table[] = {{INT32_MIN, 0}, {-1, 0}, {0, 0}, {1, 1}, {2, 2}, {3, 2}, {4, 3}, {7, 3},
                                                  {8, 4}, {1 << 30, 31}, {INT32_MAX, 31}, {(1 << 30) - 1, 30}};
    for (const auto& t : table)
        if (bucket_of(t.d) != t.b) {
            std::printf("FAIL table %d: bucket_of %d, expected %d\n", t.d, bucket_of(t.d), t.b);
            return 1;
        }
    std::mt19937 rng(12345);
    for (int i = 0; i < 1000000; i++) {
        const int32_t d = (int32_t)rng();
        // half of the draws shifted down so that every bucket is met, not only the top ones
        const int32_t v = (i & 1) ? d : (int32_t)(d >> (rng() % 32));
        const int b = bucket_of(v);
        if (b < 0 || b >= PU_DSUM_BUCKETS || b != bucket_by_comparisons(v)) {
            std::printf("FAIL random %d: bucket_of %d, comparisons %d\n", v, b, bucket_by_comparisons(v));
            return 1;
        }
        checked++;
    }

    // fold_one over the edges: count, exact sum, min, max and the histogram
    pu_dsum_replica r;
    replica_init(&r);
    if (r.cls[0].min != INT32_MAX || r.cls[0].max != INT32_MIN || r.cls[1].count != 0 || r.core_out_of_range != 0) {
        std::printf("FAIL replica_init\n");
        return 1;
    }
    int64_t sum = 0;
    uint64_t hist[PU_DSUM_BUCKETS] = {0};
    for (int32_t d : edges) {
        fold_one(&r.cls[1], d);
        sum += d;
        hist[bucket_by_comparisons(d)]++;
    }
    bool ok = r.cls[1].count == edges.size() && r.cls[1].sum == sum && r.cls[1].min == INT32_MIN &&
              r.cls[1].max == INT32_MAX && r.cls[0].count == 0;
    for (int b = 0; b < PU_DSUM_BUCKETS; b++) ok = ok && r.cls[1].hist[b] == hist[b] && r.cls[0].hist[b] == 0;
    if (!ok) {
        std::printf("FAIL fold_one over the edges\n");
        return 1;
    }

    // class and core of a record, and the range rule
    ok = class_of_mem_type(PU_RD) == 0 && class_of_mem_type(PU_WR) == 1 && class_of_mem_type(PU_WB) == 0 &&
         class_of_mem_type(255) == 0 && class_of_req16_b(1ull << 62) == 1 && class_of_req16_b(~(1ull << 62)) == 0 &&
         core_of_req16_b(0xFFFFull << 40) == 65535 && core_of_req16_b(~(0xFFFFull << 40)) == 0 &&
         core_out_of_range(-1, core_limit(4)) && core_out_of_range(4, core_limit(4)) && !core_out_of_range(3, core_limit(4)) &&
         !core_out_of_range(0, core_limit(1)) && core_out_of_range(INT32_MAX, core_limit(INT32_MAX)) &&
         core_out_of_range(INT32_MIN, core_limit(0)) && !core_out_of_range(INT32_MAX, core_limit(0));
    if (!ok) {
        std::printf("FAIL class / core rule\n");
        return 1;
    }
    std::printf("OK %ld delays\n", checked);
    return 0;
}
