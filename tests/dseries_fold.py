"""An independent numpy statement of the epoch series' rule (pu_dseries_*,
include/primeuncore.h), for tests/test_dseries_host.py and tests/test_gpu_dseries.py: the
epoch is the number of epoch boundaries t0 + j * 2^shift (j = 1 .. E - 1, in Python integers,
those beyond int64 left out) that the timer has reached, clipped into [0, E - 1]; counts and
sums by np.add.at in 64 bits, the maximum by np.maximum.at.  It shares no code with
primesim_amd/csrc/delay_series_step.h."""
from __future__ import annotations

import numpy as np

from primesim_amd import _abi as A

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FIELDS = ("count", "sum", "nonpos", "max")


def fields(reqs: np.ndarray, fmt: int) -> tuple[np.ndarray, np.ndarray]:
    """(class, timer) of every record: REQ_DTYPE records, or [n, 2] uint64 pu_req16 records."""
    if fmt == A.PU_REQ_FMT_16:
        b = reqs[:, 1]
        return ((b >> np.uint64(62)) & np.uint64(1)).astype(np.int64), (b & np.uint64((1 << 40) - 1)).astype(np.int64)
    return (reqs["mem_type"] == A.PU_WR).astype(np.int64), reqs["timer"].astype(np.int64)


def epochs_of(timer: np.ndarray, E: int, t0: int, shift: int) -> np.ndarray:
    bounds = [t0 + (j << shift) for j in range(1, E)]
    bounds = np.array([b for b in bounds if b <= I64_MAX], dtype=np.int64)
    reached = np.searchsorted(bounds, np.asarray(timer, dtype=np.int64), side="right")   # boundaries <= timer
    return np.clip(reached, 0, E - 1).astype(np.int64)


def fold(reqs: np.ndarray, delays: np.ndarray, E: int, t0: int = 0, shift: int = 0, fmt: int = A.PU_REQ_FMT_32, acc=None):
    """A.DSERIES_DTYPE [2, E] of the records, added to acc (an earlier result) when given."""
    out = np.zeros((2, E), dtype=A.DSERIES_DTYPE) if acc is None else acc.copy()
    cls, timer = fields(reqs, fmt)
    ep = epochs_of(timer, E, t0, shift)
    d = np.asarray(delays).astype(np.int64)
    count, total, nonpos = (np.zeros((2, E), dtype=np.int64) for _ in range(3))
    top = np.zeros((2, E), dtype=np.int64)
    np.add.at(count, (cls, ep), 1)
    np.add.at(total, (cls, ep), d)
    np.add.at(nonpos, (cls, ep), (d <= 0).astype(np.int64))
    np.maximum.at(top, (cls, ep), np.maximum(d, 0))
    out["count"] += count.astype(np.uint64)
    out["sum"] += total
    out["nonpos"] += nonpos.astype(np.uint64)
    out["max"] = np.maximum(out["max"], top.astype(np.int32))
    return out


def merged(cells: np.ndarray) -> np.ndarray:
    """Cells [R, 2, E] merged over the replicas: count, sum and nonpos added, max the largest."""
    E = cells.shape[-1]
    out = np.zeros((2, E), dtype=A.DSERIES_DTYPE)
    if len(cells):
        for f in ("count", "sum", "nonpos"):
            out[f] = cells[f].sum(axis=0, dtype=cells[f].dtype)
        out["max"] = cells["max"].max(axis=0)
    return out


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == A.DSERIES_DTYPE, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f} (device/host vs numpy)")
    assert not got["_pad"].any(), f"{what}: padding written"
