"""An independent numpy statement of the log-linear delay histograms' rule (pu_dhist_*,
include/primeuncore.h), for tests/test_dhist_host.py and tests/test_gpu_dhist.py: the
bucket from np.searchsorted over the 864 lower bounds built from the definition, the
histogram from np.bincount, a quantile from the sorted delays themselves (never from a
histogram).  It shares no code with primesim_amd/csrc/delay_hist_step.h."""
from __future__ import annotations

import numpy as np

from primesim_amd import _abi as A
from dsum_fold import I32_MAX, I32_MIN, fields

NB = 864


def _bounds() -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of every bucket, from the definition: bucket 0 is everything up to 0, a bucket per
    value below 64, then every octave [2^o, 2^(o+1)) for o = 6 .. 30 in 32 equal parts."""
    lo, hi = [I32_MIN], [0]
    for v in range(1, 64):
        lo.append(v)
        hi.append(v)
    for o in range(6, 31):
        width = (1 << o) // 32
        for part in range(32):
            lo.append((1 << o) + part * width)
            hi.append((1 << o) + (part + 1) * width - 1)
    return np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)


LO, HI = _bounds()
assert len(LO) == NB == A.PU_DHIST_BUCKETS and HI[-1] == I32_MAX
assert (LO[1:] == HI[:-1] + 1).all()          # no gap, no overlap

# lo and hi of every bucket, and the non-positive values
EDGE_DELAYS_FINE = np.array(sorted(set(LO.tolist()) | set(HI.tolist()) | {I32_MIN, -1, 0}), dtype=np.int32)


def buckets(d: np.ndarray) -> np.ndarray:
    """The number of lower bounds LO[1:] that d reaches."""
    return np.searchsorted(LO[1:], np.asarray(d).astype(np.int64), side="right")


def fold(reqs: np.ndarray, delays: np.ndarray, fmt: int = A.PU_REQ_FMT_32, acc=None) -> np.ndarray:
    """[2, 864] uint64 histogram of the records, added to acc when given."""
    cls, _ = fields(reqs, fmt)
    bk = buckets(delays)
    out = np.zeros((2, NB), dtype=np.uint64) if acc is None else acc.copy()
    for c in (0, 1):
        out[c] += np.bincount(bk[cls == c], minlength=NB).astype(np.uint64)
    return out


def rank(count: int, ppm: int) -> int:
    """max(1, ceil(count * ppm / 10^6)) in Python's integers."""
    return max(1, -(-count * ppm // 1000000))


def sorted_quantile(d: np.ndarray, ppm: int):
    """The nearest-rank quantile of the delays themselves, or None for no delay."""
    if len(d) == 0:
        return None
    return int(np.sort(np.asarray(d).astype(np.int64))[rank(len(d), ppm) - 1])


def quantile_buckets(reqs: np.ndarray, delays: np.ndarray, ppms, fmt: int = A.PU_REQ_FMT_32) -> np.ndarray:
    """int32 [2, len(ppms)]: per class the bucket of the sort-based quantile, -1 for an empty class."""
    cls, _ = fields(reqs, fmt)
    out = np.full((2, len(ppms)), -1, dtype=np.int32)
    for c in (0, 1):
        d = np.sort(np.asarray(delays)[cls == c].astype(np.int64))
        if len(d):
            out[c] = [buckets(d[rank(len(d), int(p)) - 1]) for p in ppms]
    return out


def coarse(hist: np.ndarray) -> np.ndarray:
    """A fine histogram [..., 864] folded down to the 32 power-of-two buckets of the delay summaries:
    fine bucket k goes where its lower bound goes (0 for bucket 0, else the bit length of LO[k])."""
    to = np.array([0] + [int(v).bit_length() for v in LO[1:]], dtype=np.int64)
    out = np.zeros(hist.shape[:-1] + (A.PU_DSUM_BUCKETS,), dtype=np.uint64)
    np.add.at(out, (..., to), hist)
    return out
