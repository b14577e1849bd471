// stream_cut_check.cpp — the device generator's scan-and-cut rule
// (primesim_amd/csrc/stream_step.h: chunk_want, cut_take, cut_here,
// start_in_msg, cursor_advance) against the obvious sequential loop of the
// host generator, on randomly drawn per-(quantum, core) request counts.
//
// The trip loop below is the kernel's (stream_gen.hip) with its lanes run one
// after another; the sequential loop is StreamGen::next (stream.cpp) with a
// cell's remaining count in place of the core's cycle.  Both produce, call by
// call, the (quantum, core, batch_start) of every record; they must agree on
// every record, on every call's count and on the final position, for any group
// width, chunk size, limit and max_msg.  Host only (tests/test_dstream_abi.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../primesim_amd/csrc/stream_step.h"

using namespace pu_stream_step;

struct Rec {
    int q, c, bs;
    bool operator==(const Rec& o) const { return q == o.q && c == o.c && bs == o.bs; }
};

struct Shape {
    int cores, quanta, max_msg;
    int64_t limit;
    std::vector<uint64_t> cnt;   // [quanta][cores]
};

// StreamGen::next: one record or one step of the cursor per trip.
struct Sequential {
    const Shape& sh;
    std::vector<uint64_t> rem;
    int q = 0, c = 0, in_msg = 0;
    int64_t n = 0;
    explicit Sequential(const Shape& s) : sh(s), rem(s.cnt) {}
    uint64_t next(std::vector<Rec>& out, uint64_t cap) {
        uint64_t k = 0;
        while (q < sh.quanta && n < sh.limit && k < cap) {
            uint64_t& r = rem[(size_t)q * sh.cores + c];
            if (r == 0) {
                in_msg = 0;
                if (++c == sh.cores) {
                    c = 0;
                    q++;
                }
                continue;
            }
            out.push_back({q, c, in_msg == 0});
            r--;
            k++;
            n++;
            in_msg = (in_msg + 1) % sh.max_msg;
        }
        return k;
    }
};

// The kernel's per-call loop, `width` lanes wide.
struct Grouped {
    const Shape& sh;
    std::vector<uint64_t> rem;
    Cursor cur{0, 0, 0, 0};
    int width;
    bool cap_counts;
    long trips = 0;
    Grouped(const Shape& s, int w, bool cap) : sh(s), rem(s.cnt), width(w), cap_counts(cap) {}
    // returns the records written, or UINT64_MAX on a broken invariant
    uint64_t next(std::vector<Rec>& out, uint64_t n_each) {
        uint64_t k = 0;
        const size_t at = out.size();
        while (cur.q < sh.quanta && cur.n < sh.limit && k < n_each) {
            trips++;
            const uint64_t want = chunk_want(n_each, k, sh.limit, cur.n);
            const int left = sh.cores - cur.c;
            const int group = left < width ? left : width;
            std::vector<uint64_t> cnt((size_t)group), excl((size_t)group);
            uint64_t total = 0;
            for (int i = 0; i < group; i++) {
                uint64_t v = rem[(size_t)cur.q * sh.cores + cur.c + i];
                if (cap_counts && v > want + 1) v = want + 1;
                cnt[(size_t)i] = v;
                excl[(size_t)i] = total;
                total += v;
            }
            const uint64_t written = total < want ? total : want;
            int cut = -1;
            uint64_t cut_taken = 0;
            out.resize(at + k + written, Rec{-1, -1, -1});
            for (int i = 0; i < group; i++) {
                const uint64_t take = cut_take(excl[(size_t)i], cnt[(size_t)i], want);
                if (cut_here(excl[(size_t)i], cnt[(size_t)i], want)) {
                    if (cut >= 0) return std::fprintf(stderr, "two cores cut in one trip\n"), UINT64_MAX;
                    cut = i;
                    cut_taken = take;
                }
                if (take && excl[(size_t)i] + take > written) return std::fprintf(stderr, "a take passes the chunk\n"), UINT64_MAX;
                int im = start_in_msg(cur, i);
                for (uint64_t j = 0; j < take; j++) {
                    out[at + k + excl[(size_t)i] + j] = {cur.q, cur.c + i, im == 0};
                    if (++im == sh.max_msg) im = 0;
                }
                rem[(size_t)cur.q * sh.cores + cur.c + i] -= take;
            }
            const Cursor before = cur;
            cursor_advance(cur, group, cut, cut_taken, written, sh.cores, sh.max_msg);
            k += written;
            // bounded: a trip writes a record or moves the cursor forward
            const bool moved = cur.q > before.q || (cur.q == before.q && cur.c > before.c);
            if (written == 0 && !moved) return std::fprintf(stderr, "a trip made no progress\n"), UINT64_MAX;
            if (cur.c < 0 || (cur.q < sh.quanta && cur.c >= sh.cores) || cur.in_msg < 0 || cur.in_msg >= sh.max_msg)
                return std::fprintf(stderr, "cursor out of range\n"), UINT64_MAX;
        }
        return k;
    }
};

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20240607);
    auto upto = [&](uint64_t hi) { return (uint64_t)(rng() % (hi + 1)); };
    long records = 0, calls = 0;
    for (int round = 0; round < rounds; round++) {
        Shape sh;
        sh.cores = 1 + (int)upto(round % 7 == 0 ? 600 : 40);
        sh.quanta = (int)upto(6);
        sh.max_msg = 1 + (int)upto(round % 3 == 0 ? 2 : 12);
        const int style = (int)upto(3);   // dense, sparse (many empty cells), mostly empty, one heavy core
        sh.cnt.resize((size_t)sh.cores * sh.quanta);
        uint64_t sum = 0;
        for (uint64_t& v : sh.cnt) {
            switch (style) {
                case 0: v = upto(9); break;
                case 1: v = upto(3) ? 0 : upto(5); break;
                case 2: v = upto(20) ? 0 : 1; break;
                default: v = upto(15) ? upto(2) : upto(300); break;
            }
            sum += v;
        }
        sh.limit = upto(2) ? INT64_MAX : (int64_t)upto(sum + 3);   // a limit of 0 means "no requests" here
        const int widths[] = {1, 2, 3, 64, 256, 1024};
        const int width = widths[upto(5)];
        Sequential a(sh);
        Grouped b(sh, width, upto(1) != 0);
        const uint64_t chunk_hi = upto(3) ? 1 + upto(40) : 1 + sum + upto(5);
        for (int call = 0;; call++) {
            const uint64_t n_each = upto(9) ? 1 + upto(chunk_hi - 1) : 0;
            std::vector<Rec> ra, rb;
            const uint64_t ka = a.next(ra, n_each);
            const uint64_t kb = b.next(rb, n_each);
            calls++;
            records += (long)ka;
            if (kb == UINT64_MAX || ka != kb || !(ra == rb) || a.n != b.cur.n) {
                std::fprintf(stderr,
                             "round %d call %d: cores %d quanta %d max_msg %d limit %lld width %d n_each %llu: "
                             "sequential wrote %llu (position %lld), grouped %llu (position %lld)\n",
                             round, call, sh.cores, sh.quanta, sh.max_msg, (long long)sh.limit, width,
                             (unsigned long long)n_each, (unsigned long long)ka, (long long)a.n,
                             (unsigned long long)kb, (long long)b.cur.n);
                for (size_t i = 0; i < ra.size() && i < rb.size(); i++)
                    if (!(ra[i] == rb[i])) {
                        std::fprintf(stderr, "  record %zu: sequential (q %d, core %d, start %d), grouped (q %d, core %d, start %d)\n",
                                     i, ra[i].q, ra[i].c, ra[i].bs, rb[i].q, rb[i].c, rb[i].bs);
                        break;
                    }
                return 1;
            }
            if (n_each && ka == 0) break;   // exhausted (both)
            if (call > 100000) return std::fprintf(stderr, "round %d does not end\n", round), 1;
        }
        const int64_t whole = (int64_t)sum < sh.limit ? (int64_t)sum : sh.limit;
        if (a.n != whole) return std::fprintf(stderr, "round %d: %lld of %lld requests\n", round, (long long)a.n, (long long)whole), 1;
    }
    std::printf("OK %d rounds, %ld calls, %ld records\n", rounds, calls, records);
    return 0;
}
