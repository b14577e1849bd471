"""An independent numpy statement of the delay summaries' rule (pu_dsum_*,
include/primeuncore.h), for tests/test_dsum_host.py and tests/test_gpu_dsum.py:
the bucket from integer comparisons, the histogram from np.bincount, the sums in
int64.  It shares no code with primesim_amd/csrc/delay_sum_step.h."""
from __future__ import annotations

import numpy as np

from primesim_amd import _abi as A

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

# every bucket edge: INT32_MIN, -1, 0, 1, 2, 3, 4, 2^k - 1 and 2^k for k up to 30, 2^31 - 1
EDGE_DELAYS = np.array(sorted({I32_MIN, -1, 0, 1, 2, 3, 4, I32_MAX} |
                              {(1 << k) - 1 for k in range(1, 31)} | {1 << k for k in range(1, 31)}), dtype=np.int32)


def buckets(d: np.ndarray) -> np.ndarray:
    """0 for d <= 0, else the number of thresholds 2^0 .. 2^30 that d reaches."""
    d = d.astype(np.int64)
    b = np.zeros(d.shape, dtype=np.int64)
    for k in range(31):
        b += d >= (1 << k)
    return b


def fields(reqs: np.ndarray, fmt: int) -> tuple[np.ndarray, np.ndarray]:
    """(class, core) of every record: REQ_DTYPE records, or [n, 2] uint64 pu_req16 records."""
    if fmt == A.PU_REQ_FMT_16:
        b = reqs[:, 1]
        return ((b >> np.uint64(62)) & np.uint64(1)).astype(np.int64), \
            ((b >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int64)
    return (reqs["mem_type"] == A.PU_WR).astype(np.int64), reqs["core"].astype(np.int64)


def fold(reqs: np.ndarray, delays: np.ndarray, num_cores=None, fmt: int = A.PU_REQ_FMT_32, acc=None):
    """(summary, core_count, core_sum) of the records, added to acc (a triple from an
    earlier call) when given; the per-core arrays are None without num_cores."""
    cls, core = fields(reqs, fmt)
    d = delays.astype(np.int64)
    bk = buckets(delays)
    if acc is None:
        s = np.zeros((), dtype=A.DSUM_DTYPE)
        s["cls"]["min"], s["cls"]["max"] = I32_MAX, I32_MIN
        cnt = sm = None
        if num_cores is not None:
            cnt, sm = np.zeros(num_cores, dtype=np.uint64), np.zeros(num_cores, dtype=np.int64)
    else:
        s, cnt, sm = acc[0].copy(), None if acc[1] is None else acc[1].copy(), None if acc[2] is None else acc[2].copy()
    k = s["cls"]          # field first: views into s
    for c in (0, 1):
        m = cls == c
        k["count"][c] += np.uint64(m.sum())
        k["sum"][c] += np.int64(d[m].sum())
        if m.any():
            k["min"][c] = min(int(k["min"][c]), int(d[m].min()))
            k["max"][c] = max(int(k["max"][c]), int(d[m].max()))
        k["hist"][c] += np.bincount(bk[m], minlength=A.PU_DSUM_BUCKETS).astype(np.uint64)
    out = core < 0
    if num_cores is not None:
        out = out | (core >= num_cores)
        ok = ~out
        cnt += np.bincount(core[ok], minlength=num_cores).astype(np.uint64)
        # exact: int64 partial sums per core (np.bincount's weights would go through float64)
        np.add.at(sm, core[ok], d[ok])
    s["core_out_of_range"] += int(out.sum())
    return s, cnt, sm


def assert_same(got, want, what=""):
    """Summaries (records or arrays of A.DSUM_DTYPE) equal field by field, with a readable message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    for f in ("count", "sum", "min", "max", "hist"):
        np.testing.assert_array_equal(got["cls"][f], want["cls"][f], err_msg=f"{what}: {f} (device/host vs numpy)")
    np.testing.assert_array_equal(got["core_out_of_range"], want["core_out_of_range"],
                                  err_msg=f"{what}: core_out_of_range")


def synth(n: int, num_cores: int, seed: int, cores=None, delays=None, write_pct: int = 30) -> tuple[np.ndarray, np.ndarray]:
    """n REQ_DTYPE records that fit pu_req16, and n delays: cores in message-like runs of
    1..100 (or the given array), about write_pct percent writes, delays mostly positive and
    small with zeros, -1 and a few large values mixed in (or the given array)."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=A.REQ_DTYPE)
    if cores is None:
        runs = rng.integers(1, 101, size=n + 1)
        ids = rng.integers(0, num_cores, size=n + 1)
        cores = np.repeat(ids, runs)[:n]
    r["core"] = cores
    r["addr"] = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    r["timer"] = np.arange(n)
    r["prog_id"] = 1
    r["mem_type"] = (rng.integers(0, 100, size=n) < write_pct).astype(np.uint8)
    if delays is None:
        delays = rng.integers(1, 600, size=n)
        pick = rng.integers(0, 40, size=n)
        delays = np.where(pick == 0, 0, delays)
        delays = np.where(pick == 1, -1, delays)
        delays = np.where(pick == 2, rng.integers(1 << 20, I32_MAX, size=n), delays)
    return r, np.ascontiguousarray(delays, dtype=np.int32)
