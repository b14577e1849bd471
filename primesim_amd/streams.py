"""Synthetic request streams: their parameters, the host generators (pu_stream_*), the
generators on the device (pu_dstream_*) and the 16-byte request format (pu_req16)."""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi as A
from ._native import UncoreError, _as, _DeviceSet, _to_end, call, counted, last_error, lib, opened


@dataclass
class StreamSpec:
    kind: int
    num_cores: int
    seed: int = 1
    quantum: int = 1000
    num_quanta: int = 1
    max_msg: int = 100
    num_progs: int = 1
    max_requests: int = 0
    write_pct: int = -1

    def params(self) -> A.StreamParams:
        return A.StreamParams(self.kind, self.num_cores, self.seed, self.quantum, self.num_quanta,
                              self.max_msg, self.num_progs, self.max_requests, self.write_pct, 0)


def pack_req16(reqs: np.ndarray) -> np.ndarray:
    """REQ_DTYPE records -> 16-B pu_req16 records (uint64 pairs, primeuncore.h);
    raises UncoreError naming the first record that does not fit."""
    assert reqs.dtype == A.REQ_DTYPE and reqs.flags.c_contiguous
    out = np.empty(reqs.shape + (2,), dtype=np.uint64)
    call("pu_pack_req16", reqs.ctypes.data, reqs.size, out.ctypes.data)
    return out


def generate_stream(spec: StreamSpec) -> np.ndarray:
    """Deterministic synthetic request stream in canonical order (REQ_DTYPE)."""
    p = spec.params()
    n = counted("pu_stream_count", C.byref(p))
    out = np.zeros(n, dtype=A.REQ_DTYPE)
    if n:
        got = lib().pu_stream_generate(C.byref(p), out.ctypes.data, n)
        if got != n:
            raise UncoreError(f"stream generation returned {got}, expected {n}")
    return out


def stream_threads(spec: StreamSpec) -> list[tuple[int, int]]:
    """(prog_id, thread_id) of every core, in allocation order."""
    p = spec.params()
    res = []
    for c in range(spec.num_cores):
        pr, th = C.c_int(), C.c_int()
        call("pu_stream_thread_of", C.byref(p), c, C.byref(pr), C.byref(th))
        res.append((pr.value, th.value))
    return res


def stream_fits_req16(spec: StreamSpec) -> bool:
    """True when every record of the stream fits pu_req16, decided from the
    parameters alone (pu_stream_fits_req16): never True for a stream that
    pack_req16 would refuse."""
    p = spec.params()
    rc = lib().pu_stream_fits_req16(C.byref(p))
    if rc not in (0, -34):
        raise UncoreError(f"pu_stream_fits_req16: {last_error()} ({rc})")
    return rc == 0


def _fork_range(count: int, first: int, n: Optional[int], seeds):
    """(n, seeds) of a fork over `count` members: n = None is "to the end"; seeds,
    where given, one uint64 per member of the range."""
    n = _to_end(count, first, n)
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (max(n, 0),):
            raise UncoreError(f"fork: {seeds.shape} seeds for a range of {n}")
    return n, seeds


class StreamSet:
    """Resumable generators for several streams (pu_stream_open/next_many):
    `next(n)` returns the next n requests of every stream as an [count, n]
    array; the chunks concatenate to exactly generate_stream's output."""

    def __init__(self, specs: list[StreamSpec]):
        self._h = []
        self._specs = list(specs)
        for sp in specs:
            p = sp.params()
            try:
                self._h.append(opened("pu_stream_open", C.byref(p)))
            except UncoreError:
                self.close()
                raise
        self._arr = (C.c_void_p * len(self._h))(*self._h)

    def __len__(self) -> int:
        return len(self._h)

    def next_into(self, out: np.ndarray, threads: int = 0) -> int:
        """Fill out[i, :] with stream i's next out.shape[1] requests; returns the
        smallest number produced (short only at the end of a stream)."""
        assert out.dtype == A.REQ_DTYPE and out.ndim == 2 and out.shape[0] == len(self._h)
        assert out.flags.c_contiguous
        return counted("pu_stream_next_many", self._arr, len(self._h), out.ctypes.data, out.shape[1], out.shape[1],
                       threads)

    def next(self, n: int, threads: int = 0) -> np.ndarray:
        out = np.zeros((len(self._h), n), dtype=A.REQ_DTYPE)
        got = self.next_into(out, threads)
        return out[:, :got]

    def position(self, i: int = 0) -> int:
        return int(lib().pu_stream_position(self._h[i]))

    def fork(self, src: int, first: int = 0, n: Optional[int] = None, seeds=None) -> None:
        """Streams [first, first + n) continue from stream src's position (pu_stream_fork):
        exact clones without seeds, else stream first + i draws as a stream of seeds[i]
        does.  src inside the range is left as it is.  A stream whose parameters differ
        from src's in more than the seed is refused, before any stream is changed."""
        n, seeds = _fork_range(len(self._h), first, n, seeds)
        if not (0 <= src < len(self._h) and 0 <= first and 0 <= n and first + n <= len(self._h)):
            raise UncoreError(f"pu_stream_fork: source {src} or range [{first}, {first + n}) outside the set")
        shape = dataclasses.replace(self._specs[src], seed=0)
        for d in range(first, first + n):   # all or nothing: pu_stream_fork itself refuses stream by stream
            if dataclasses.replace(self._specs[d], seed=0) != shape:
                raise UncoreError(f"pu_stream_fork: the parameters of stream {d} differ from those of stream {src} "
                                  "in more than the seed")
        for i in range(n):
            d = first + i
            if d == src:
                continue
            seed = int(seeds[i]) if seeds is not None else 0
            call("pu_stream_fork", self._h[d], self._h[src], int(seeds is not None), seed, context=f"stream {d}: ")
            self._specs[d] = dataclasses.replace(self._specs[d], seed=seed if seeds is not None
                                                 else self._specs[src].seed)

    def close(self) -> None:
        for h in self._h:
            lib().pu_stream_close(h)
        self._h = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceStreamSet(_DeviceSet):
    """StreamSet on the device (pu_dstream_*): the generator state of every
    stream lives in device memory (`state_bytes`) and `next_into` writes each stream's
    next chunk into device memory, ready for run_device / run_device_sliced /
    run_device_pool, byte for byte what StreamSet produces.  Pointers are plain
    integers (tensor.data_ptr()).  Needs a GPU: there is no host fallback."""
    _prefix = "pu_dstream"

    def __init__(self, specs: list[StreamSpec], device: int = 0):
        self._n = len(specs)
        arr = (A.StreamParams * max(1, len(specs)))(*[sp.params() for sp in specs])
        self._open(arr, len(specs), device)

    def next_into(self, d_out_ptr: int, n_each: int, stride: Optional[int] = None, fmt: int = A.PU_REQ_FMT_32,
                  d_got_ptr: int = 0, stream_ptr: int = 0) -> None:
        """Stream i's next up to n_each requests into records [i*stride, i*stride + got_i)
        of d_out (pu_req, or pu_req16 with fmt = PU_REQ_FMT_16); got_i goes to
        d_got[i] (device uint64) when given.  Asynchronous on stream_ptr (a hipStream_t as an
        integer, e.g. torch.cuda.Stream().cuda_stream); 0 is the set's own stream, which is
        not ordered with torch's default stream: positions() waits for it."""
        self._call("next", d_out_ptr or None, n_each, n_each if stride is None else stride, fmt, d_got_ptr or None,
                   stream_ptr or None)

    def fork(self, src: int, first: int = 0, n: Optional[int] = None, seeds=None, stream_ptr: int = 0) -> None:
        """StreamSet.fork on the device (pu_dstream_fork), asynchronous on stream_ptr like
        next_into: streams [first, first + n) continue from stream src's position, as exact
        clones without seeds, else stream first + i with the draws of a stream of seeds[i]."""
        n, seeds = _fork_range(self._n, first, n, seeds)
        self._call("fork", src, first, n, _as(seeds, C.c_uint64), stream_ptr or None)

    def positions(self) -> np.ndarray:
        """Requests produced so far per stream (waits for the set's outstanding calls)."""
        out = np.zeros(self._n, dtype=np.int64)
        self._call("positions", out.ctypes.data, self._n)
        return out
