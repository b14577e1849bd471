"""Recorded traces: one trace placed per replica, on the host (pu_trace_place) and across an
ensemble on the device (pu_dtrace_*)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi as A
from ._native import UncoreError, _as, _DeviceSet, call, counted, lib


def _rows(a, shape: tuple, what: str) -> Optional[np.ndarray]:
    """A placement or skew table as the contiguous int32 array of `shape` the library takes (None stays None)."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.shape != shape or a.dtype.kind not in "iu" or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
        raise UncoreError(f"{what}: an integer array of shape {shape} in int32 range, not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.int32)


def place_trace(reqs: np.ndarray, placement=None, skew=None, num_cores: Optional[int] = None,
                fmt: int = A.PU_REQ_FMT_32) -> np.ndarray:
    """A recorded trace under one replica's rows (pu_trace_place; the rule is in
    include/primeuncore.h): core' = placement[core], timer' = timer + skew[core], everything
    else unchanged.  Returns REQ_DTYPE records, or with fmt = PU_REQ_FMT_16 the [n, 2] uint64
    array pack_req16 gives for them.  num_cores defaults to the rows' length, or without rows
    to the trace's largest core + 1.  Needs no device."""
    assert reqs.dtype == A.REQ_DTYPE and reqs.ndim == 1
    reqs = np.ascontiguousarray(reqs)
    if num_cores is None:
        given = placement if placement is not None else skew
        num_cores = len(given) if given is not None else (int(reqs["core"].max()) + 1 if len(reqs) else 1)
    place = _rows(placement, (num_cores,), "place_trace: placement")
    sk = _rows(skew, (num_cores,), "place_trace: skew")
    out = np.zeros((len(reqs), 2), dtype=np.uint64) if fmt == A.PU_REQ_FMT_16 else np.zeros(len(reqs), dtype=A.REQ_DTYPE)
    call("pu_trace_place", reqs.ctypes.data, len(reqs), _as(place, C.c_int32), _as(sk, C.c_int32), num_cores, fmt,
         out.ctypes.data)
    return out


_MASK64 = (1 << 64) - 1


def placement_seed(seed: int, r: int) -> int:
    """The pu_placement_shuffle seed of row r of random_placements(.., seed): 0 (the identity) for
    r = 0; otherwise the splitmix64 output function of (seed + r * 0x9E3779B97F4A7C15) mod 2^64,
    with 1 in place of a 0 (which would be the identity again)."""
    if r == 0:
        return 0
    z = (seed + r * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return (z ^ (z >> 31)) or 1


def random_placements(count: int, num_cores: int, seed: int) -> np.ndarray:
    """int32[count][num_cores]: row r is pu_placement_shuffle of placement_seed(seed, r), so row 0
    is the identity and every row is a permutation; deterministic.  Needs no device."""
    out = np.zeros((count, num_cores), dtype=np.int32)
    for r in range(count):
        call("pu_placement_shuffle", _as(out[r], C.c_int32), num_cores, placement_seed(seed, r))
    return out


class DeviceTraceSet(_DeviceSet):
    """One recorded trace replayed across `count` replicas on the device (pu_dtrace_*): the
    trace lives in device memory once, with the rows (`state_bytes`), and `next_into` writes its
    next chunk into every replica's window under that replica's placement and skew rows
    ([count][num_cores], or None), byte for byte what place_trace gives.  One cursor for the
    whole set.  `next_into` has DeviceStreamSet's signature, so a driver can hold either.
    Pointers are plain integers (tensor.data_ptr()).  Needs a GPU: place_trace is the host path."""
    _prefix = "pu_dtrace"

    def __init__(self, reqs: np.ndarray, num_cores: int, count: int, placements=None, skews=None, device: int = 0):
        assert reqs.dtype == A.REQ_DTYPE and reqs.ndim == 1
        reqs = np.ascontiguousarray(reqs)
        self._n, self._len = count, len(reqs)
        shape = (max(count, 0), max(num_cores, 0))
        place = _rows(placements, shape, "DeviceTraceSet: placements")
        sk = _rows(skews, shape, "DeviceTraceSet: skews")
        self._open(reqs.ctypes.data if len(reqs) else None, len(reqs), num_cores, count, _as(place, C.c_int32),
                   _as(sk, C.c_int32), device)

    @property
    def trace_len(self) -> int:
        """Records of the trace."""
        return self._len

    def next_into(self, d_out_ptr: int, n_each: int, stride: Optional[int] = None, fmt: int = A.PU_REQ_FMT_32,
                  d_got_ptr: int = 0, stream_ptr: int = 0) -> None:
        """The next got = min(n_each, what the trace has left) records, placed for replica i, into
        records [i*stride, i*stride + got) of d_out (pu_req, or pu_req16 with fmt =
        PU_REQ_FMT_16); got goes to d_got[i] (device uint64) when given.  Asynchronous on
        stream_ptr (a hipStream_t as an integer); 0 is the set's own stream, which is not
        ordered with torch's default stream: position() waits for it."""
        self._call("next", d_out_ptr or None, n_each, n_each if stride is None else stride, fmt, d_got_ptr or None,
                   stream_ptr or None)

    def seek(self, position: int) -> None:
        """Move the set's cursor (0 .. trace_len); seek(0) replays the trace.  Waits for the set's outstanding calls."""
        self._call("seek", position)

    def position(self) -> int:
        """Records of the trace served so far (waits for the set's outstanding calls)."""
        return counted("pu_dtrace_position", self._handle())

    def fits_req16(self) -> bool:
        """True when next_into serves PU_REQ_FMT_16 (decided at open; last_error() has the reason when not)."""
        return lib().pu_dtrace_fits_req16(self._handle()) == 0
