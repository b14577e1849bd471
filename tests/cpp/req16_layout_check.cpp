// req16_layout_check — the pu_req16 macros of include/primeuncore.h against the
// layout written out here with literal shifts: b = timer (bits 0-39) | core
// (40-55) | prog_id (56-61) | mem_type (62) | batch_start (63).  Every field
// takes 0, 1, max-1 and max in all combinations, then 100,000 random records
// follow; PU_REQ16_B must give the literal word, every extract macro must give
// its field back, and each macro must evaluate each argument exactly once.
// A stand-alone program (the test builds it with the host's sanitizers); prints
// "OK <n> records".
#include <cstdint>
#include <cstdio>
#include <random>

#include "primeuncore.h"

namespace {

uint64_t n_records = 0;
uint64_t evals[6] = {0, 0, 0, 0, 0, 0};   // timer, core, prog_id, mem_type, batch_start, b

template <class T>
T once(int arg, T v) {
    evals[arg]++;
    return v;
}

bool check(int64_t timer, int32_t core, int32_t prog, uint8_t type, uint8_t batch) {
    const uint64_t want = (uint64_t)timer | (uint64_t)core << 40 | (uint64_t)prog << 56 | (uint64_t)type << 62 |
                          (uint64_t)batch << 63;
    const uint64_t b = PU_REQ16_B(once(0, timer), once(1, core), once(2, prog), once(3, type), once(4, batch));
    n_records++;
    bool ok = b == want;
    ok = ok && PU_REQ16_TIMER(once(5, b)) == timer;
    ok = ok && PU_REQ16_CORE(once(5, b)) == core;
    ok = ok && PU_REQ16_PROG(once(5, b)) == prog;
    ok = ok && PU_REQ16_TYPE(once(5, b)) == type;
    ok = ok && PU_REQ16_BATCH(once(5, b)) == batch;
    if (!ok)
        std::printf("FAIL timer %lld core %d prog %d type %d batch %d: b %016llx, literal %016llx\n", (long long)timer,
                    core, prog, type, batch, (unsigned long long)b, (unsigned long long)want);
    return ok;
}

}  // namespace

int main() {
    const int64_t timer_max = (1ll << 40) - 1;
    const int64_t timers[4] = {0, 1, timer_max - 1, timer_max};
    const int32_t cores[4] = {0, 1, 65534, 65535};
    const int32_t progs[4] = {0, 1, 62, 63};
    const uint8_t bits[2] = {0, 1};   // max-1 and max of a one-bit field are 0 and 1
    for (int64_t t : timers)
        for (int32_t c : cores)
            for (int32_t p : progs)
                for (uint8_t ty : bits)
                    for (uint8_t bs : bits)
                        if (!check(t, c, p, ty, bs)) return 1;
    std::mt19937_64 rng(20260131);
    for (int i = 0; i < 100000; i++) {
        const uint64_t r = rng(), r2 = rng();
        if (!check((int64_t)(r & (uint64_t)timer_max), (int32_t)(r >> 40 & 0xFFFF), (int32_t)(r >> 56 & 63),
                   (uint8_t)(r2 & 1), (uint8_t)(r2 >> 1 & 1)))
            return 1;
    }
    for (int a = 0; a < 5; a++)
        if (evals[a] != n_records) {
            std::printf("FAIL PU_REQ16_B evaluated argument %d %llu times for %llu records\n", a,
                        (unsigned long long)evals[a], (unsigned long long)n_records);
            return 1;
        }
    if (evals[5] != 5 * n_records) {
        std::printf("FAIL the extract macros evaluated b %llu times in %llu uses\n", (unsigned long long)evals[5],
                    (unsigned long long)(5 * n_records));
        return 1;
    }
    std::printf("OK %llu records\n", (unsigned long long)n_records);
    return 0;
}
