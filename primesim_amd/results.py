"""End-of-run results of an engine's replicas: by plain copies on the host
(pu_dres_host_gather) and gathered on the device (pu_dres_*)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi as A
from ._native import _as, _DeviceSet, call, lib

QUEUE_KINDS = ("x", "y", "z", "bus")     # pu_config_queue_ends: kind 0 .. 3


def queue_ends(cfg: A.SimCfg, q: int) -> tuple[int, int, int]:
    """(kind, a, b) of queue q of a configuration (pu_config_queue_ends; no device):
    kind 0 / 1 / 2 a link along x / y / z between nodes a < b, 3 the bus of cache b of
    level a, -1 (with a = b = -1) where q names no queue."""
    kind, a, b = C.c_int(), C.c_int(), C.c_int()
    call("pu_config_queue_ends", C.byref(cfg), q, C.byref(kind), C.byref(a), C.byref(b))
    return kind.value, a.value, b.value


def host_run_results(um: "UncoreManager", replica: int = 0, queues: bool = False):
    """One replica's end-of-run record by plain copies (pu_dres_host_gather), as an
    A.DRES_DTYPE record; with queues also the n and n1 of every queue."""
    out = np.zeros(1, dtype=A.DRES_DTYPE)
    nq = int(lib().pu_num_queues(um._handle())) if queues else 0
    n = np.zeros(nq, dtype=np.uint64) if queues else None
    n1 = np.zeros(nq, dtype=np.uint64) if queues else None
    call("pu_dres_host_gather", um._handle(), replica, _as(out, A.DresReplica), _as(n, C.c_uint64),
         _as(n1, C.c_uint64), nq)
    return (out[0], n, n1) if queues else out[0]


class DeviceRunResults(_DeviceSet):
    """The end-of-run results of an UncoreManager's replicas gathered on the device
    (pu_dres_*): `gather` snapshots every replica of a range in one launch -- the
    counters of stats(), the fold of completion(), the run state and the visit counts
    of the links and buses -- and `read` brings the records (A.DRES_DTYPE) to the host
    in one copy.  queues=True keeps the per-queue map (16 B per queue and replica).
    Close it before the UncoreManager.  Needs a GPU: host_run_results is the host path."""
    _prefix = "pu_dres"

    def __init__(self, um: "UncoreManager", queues: bool = False):
        self._um = um                      # the set reads the manager's replicas: keep it alive
        self._n = int(lib().pu_num_replicas(um._handle()))
        self._open(um._handle(), A.PU_DRES_QUEUES if queues else 0)
        self._nq = int(lib().pu_dres_nqueues(self._h))

    @property
    def num_queues(self) -> int:
        """Queues per replica: the links first, then the buses."""
        return self._nq

    @property
    def num_links(self) -> int:
        return int(lib().pu_num_links(self._um._handle()))

    def gather(self, first: int = 0, n: Optional[int] = None, stream_ptr: int = 0) -> None:
        """Asynchronous on stream_ptr (a hipStream_t as an integer; 0 is the set's own
        stream).  The caller orders it after the run it wants to see: the run's stream,
        or synchronize() first."""
        self._um._handle()                 # the set reads the manager's replicas: it must still be open
        self._call("gather", first, self._count(first, n), stream_ptr or None)

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records of replicas [first, first + n) as of their last gather (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros(max(n, 0), dtype=A.DRES_DTYPE)
        self._call("read", first, n, _as(out, A.DresReplica))
        return out

    def queues(self, replica: int) -> tuple[np.ndarray, np.ndarray]:
        """(n, n1) per queue of one replica; raises for a set opened without queues=True."""
        n, n1 = np.zeros(self._nq, dtype=np.uint64), np.zeros(self._nq, dtype=np.uint64)
        self._call("read_queues", replica, _as(n, C.c_uint64), _as(n1, C.c_uint64), self._nq)
        return n, n1

    def queue_totals(self) -> tuple[np.ndarray, np.ndarray]:
        """(n, n1) per queue summed over the replicas of the last gather.  A set opened with
        queues=True sums its map: a snapshot, like the records.  A set without it sums the queue
        headers as they are at this call, so after another run the two kinds of set answer
        differently for the same gather: read the totals before the next run, or keep the map."""
        self._um._handle()                 # without the map the totals are read from the manager's replicas
        n, n1 = np.zeros(self._nq, dtype=np.uint64), np.zeros(self._nq, dtype=np.uint64)
        self._call("read_queue_totals", _as(n, C.c_uint64), _as(n1, C.c_uint64), self._nq)
        return n, n1
