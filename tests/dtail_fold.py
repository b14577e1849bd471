"""An independent numpy statement of the rule of the slowest-request lists (pu_dtail_*,
include/primeuncore.h), for tests/test_dtail_host.py and tests/test_gpu_dtail.py: split
the records by class, order each class by np.lexsort over (position, -delay) with the
delays widened to int64, take the first k.  Folding chunk after chunk re-sorts the
concatenation of what is kept and what comes.  The ensemble total sorts the replicas'
lists by (-delay, replica, position).  It shares no code with
primesim_amd/csrc/delay_tail_step.h."""
from __future__ import annotations

import numpy as np

from primesim_amd import _abi as A
from dsum_fold import fields

FIELDS = ("addr", "timer", "position", "delay", "core")


def records(reqs: np.ndarray, delays: np.ndarray, fmt: int = A.PU_REQ_FMT_32, first_position: int = 0):
    """(class, entries): every record as an A.DTAIL_DTYPE entry, positions counted from first_position."""
    cls, core = fields(reqs, fmt)
    e = np.zeros(len(delays), dtype=A.DTAIL_DTYPE)
    if fmt == A.PU_REQ_FMT_16:
        e["addr"] = reqs[:, 0]
        e["timer"] = (reqs[:, 1] & np.uint64((1 << 40) - 1)).astype(np.int64)
    else:
        e["addr"] = reqs["addr"]
        e["timer"] = reqs["timer"]
    e["core"] = core
    e["delay"] = delays
    e["position"] = np.arange(len(delays), dtype=np.uint64) + np.uint64(first_position)
    return cls, e


def best(entries: np.ndarray, k: int) -> np.ndarray:
    """The first k of the entries by delay descending, then position ascending."""
    order = np.lexsort((entries["position"], -entries["delay"].astype(np.int64)))
    return entries[order[:k]]


def fold(reqs: np.ndarray, delays: np.ndarray, k: int, fmt: int = A.PU_REQ_FMT_32, acc=None):
    """(entries [2, k], counts [2], seen) of the records, continued from acc (a triple from an earlier call)."""
    if acc is None:
        acc = (np.zeros((2, k), dtype=A.DTAIL_DTYPE), np.zeros(2, dtype=np.uint32), 0)
    old, old_counts, seen = acc
    cls, e = records(reqs, delays, fmt, first_position=seen)
    out = np.zeros((2, k), dtype=A.DTAIL_DTYPE)
    counts = np.zeros(2, dtype=np.uint32)
    for c in (0, 1):
        kept = best(np.concatenate([old[c][:int(old_counts[c])], e[cls == c]]), k)
        out[c][:len(kept)] = kept
        counts[c] = len(kept)
    return out, counts, seen + len(delays)


def total(entries: np.ndarray, counts: np.ndarray, k: int):
    """(entries [2, k], replicas [2, k], counts [2]) of lists entries [n, 2, k] with counts [n, 2], whose
    replica indices start at 0: by delay descending, then replica, then position."""
    out = np.zeros((2, k), dtype=A.DTAIL_DTYPE)
    reps = np.full((2, k), -1, dtype=np.int32)
    cnt = np.zeros(2, dtype=np.uint32)
    for c in (0, 1):
        e = np.concatenate([entries[r][c][:int(counts[r][c])] for r in range(len(entries))] or
                           [np.zeros(0, dtype=A.DTAIL_DTYPE)])
        rep = np.concatenate([np.full(int(counts[r][c]), r, dtype=np.int32) for r in range(len(entries))] or
                             [np.zeros(0, dtype=np.int32)])
        order = np.lexsort((e["position"], rep, -e["delay"].astype(np.int64)))[:k]
        out[c][:len(order)] = e[order]
        reps[c][:len(order)] = rep[order]
        cnt[c] = len(order)
    return out, reps, cnt


def assert_same(got, want, what=""):
    """(entries, counts[, seen]) equal field by field, with a readable message."""
    assert got[0].shape == want[0].shape and got[0].dtype == A.DTAIL_DTYPE, f"{what}: shape {got[0].shape} vs {want[0].shape}"
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: counts")
    for f in FIELDS:
        np.testing.assert_array_equal(got[0][f], want[0][f], err_msg=f"{what}: {f}")
    if len(want) > 2 and len(got) > 2:
        assert int(got[2]) == int(want[2]), f"{what}: seen {got[2]} vs {want[2]}"
