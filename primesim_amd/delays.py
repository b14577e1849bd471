"""What an ensemble's (request, delay) pairs fold into: summaries (pu_dsum_*), log-linear
histograms (pu_dhist_*), the slowest requests (pu_dtail_*) and series over simulated time
(pu_dseries_*), each as a host fold and as a set kept on the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi as A
from ._native import UncoreError, _as, _DeviceSet, call, counted, lib


def _records(reqs: np.ndarray, delays: np.ndarray, fmt: int) -> tuple[np.ndarray, np.ndarray]:
    """(reqs, delays) of a host fold, contiguous: one request per delay, REQ_DTYPE records or
    with fmt = PU_REQ_FMT_16 the [n, 2] uint64 array of pack_req16; the delays as int32."""
    n = len(delays)
    if fmt == A.PU_REQ_FMT_16:
        assert reqs.dtype == np.uint64 and reqs.shape == (n, 2)
    else:
        assert reqs.dtype == A.REQ_DTYPE and reqs.shape == (n,)
    return np.ascontiguousarray(reqs), np.ascontiguousarray(delays, dtype=np.int32)


class _DelayStage(_DeviceSet):
    """What the four delay stages share: the entries `<_prefix>_add` and `<_prefix>_reset`."""

    def add(self, d_reqs_ptr: int, d_delay_ptr: int, d_begin_ptr: int, d_end_ptr: int, fmt: int = A.PU_REQ_FMT_32,
            stream_ptr: int = 0) -> None:
        """Asynchronous on stream_ptr (a hipStream_t as an integer); 0 is the set's own
        stream, which is not ordered with torch's streams.  d_begin / d_end: device uint64,
        one entry per replica, in records (d_off and d_off + 1 after run_device)."""
        self._call("add", d_reqs_ptr or None, fmt, d_delay_ptr or None, d_begin_ptr or None, d_end_ptr or None,
                   stream_ptr or None)

    def reset(self) -> None:
        self._call("reset")


# ---------------------------------------------------------------- delay summaries
def summarize_delays(reqs: np.ndarray, delays: np.ndarray, num_cores: Optional[int] = None,
                     fmt: int = A.PU_REQ_FMT_32):
    """The host fold of (request, delay) pairs (pu_dsum_host_add; the rule is in
    include/primeuncore.h): returns (summary, core_count, core_sum), where summary is
    one A.DSUM_DTYPE record and the per-core arrays (num_cores entries) are None
    without num_cores.  reqs: REQ_DTYPE records, or with fmt = PU_REQ_FMT_16 the
    [n, 2] uint64 array of pack_req16.  Needs no device."""
    reqs, delays = _records(reqs, delays, fmt)
    out = np.zeros(1, dtype=A.DSUM_DTYPE)
    lib().pu_dsum_host_init(_as(out, A.DsumReplica))
    cnt = sm = None
    if num_cores is not None:
        # (at least one entry, so that the library sees tables and refuses a num_cores below 1)
        cnt, sm = np.zeros(max(num_cores, 1), dtype=np.uint64), np.zeros(max(num_cores, 1), dtype=np.int64)
    call("pu_dsum_host_add", _as(out, A.DsumReplica), _as(cnt, C.c_uint64), _as(sm, C.c_int64),
         0 if num_cores is None else num_cores, reqs.ctypes.data, fmt, _as(delays, C.c_int32), len(delays))
    return out[0], cnt, sm


class DeviceDelaySummary(_DelayStage):
    """Per-replica delay summaries kept on the device (pu_dsum_*): `add` folds every
    replica's records [begin[r], end[r]) of device request and delay arrays into its
    running summary, bit for bit what summarize_delays gives.  num_cores (one entry per
    replica) adds per-core (count, sum) tables.  Pointers are plain integers
    (tensor.data_ptr()).  Needs a GPU: there is no host fallback."""
    _prefix = "pu_dsum"

    def __init__(self, count: int, num_cores=None, device: int = 0):
        self._n = count
        self._nc = None
        arr = None
        if num_cores is not None:
            self._nc = [int(c) for c in num_cores]
            if len(self._nc) != count:
                raise UncoreError(f"DeviceDelaySummary: {len(self._nc)} num_cores entries for {count} replicas")
            arr = (C.c_int32 * max(1, count))(*self._nc)
        self._open(count, arr, device)

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Summaries of replicas [first, first + n) as A.DSUM_DTYPE records (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros(max(n, 0), dtype=A.DSUM_DTYPE)
        self._call("read", first, n, _as(out, A.DsumReplica))
        return out

    def cores(self, replica: int) -> tuple[np.ndarray, np.ndarray]:
        """(count, sum) per core of one replica; raises for a set opened without num_cores."""
        nc = self._nc[replica] if self._nc is not None and 0 <= replica < self._n else 0
        cnt, sm = np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.int64)
        self._call("read_cores", replica, _as(cnt, C.c_uint64), _as(sm, C.c_int64), nc)
        return cnt, sm


# ---------------------------------------------------------------- delay histograms
def _ppm_array(ppm) -> np.ndarray:
    """Quantiles in parts per million as the uint32 array the library takes (it checks count and range)."""
    a = np.atleast_1d(np.asarray(ppm, dtype=np.int64))
    if a.ndim != 1 or (a < 0).any() or (a > 0xFFFFFFFF).any():
        raise UncoreError("quantiles: ppm is a list of integers in [0, 1000000]")
    return np.ascontiguousarray(a, dtype=np.uint32)


def dhist_bucket_of(d: int) -> int:
    """The log-linear bucket of a delay (pu_dhist_bucket_of; the rule is in include/primeuncore.h)."""
    return int(lib().pu_dhist_bucket_of(int(d)))


def dhist_bucket_bounds(k: int) -> tuple[int, int]:
    """(lo, hi), both inclusive, of the delays bucket k holds (pu_dhist_bucket_bounds)."""
    lo, hi = C.c_int32(), C.c_int32()
    call("pu_dhist_bucket_bounds", int(k), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def delay_histogram(reqs: np.ndarray, delays: np.ndarray, fmt: int = A.PU_REQ_FMT_32) -> np.ndarray:
    """The host fold of (request, delay) pairs into a [2, PU_DHIST_BUCKETS] uint64 log-linear
    histogram, reads and writes apart (pu_dhist_host_add).  reqs as for summarize_delays.
    Needs no device."""
    reqs, delays = _records(reqs, delays, fmt)
    out = np.zeros((2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
    call("pu_dhist_host_add", _as(out, C.c_uint64), reqs.ctypes.data, fmt, _as(delays, C.c_int32), len(delays))
    return out


def histogram_quantiles(hist: np.ndarray, ppm) -> tuple[np.ndarray, np.ndarray]:
    """(count, bucket) of log-linear histograms [..., PU_DHIST_BUCKETS]: per histogram its count
    (uint64 [...]) and the bucket of every quantile of ppm (int32 [..., len(ppm)]; -1 for an
    empty histogram), by the nearest-rank rule (pu_dhist_host_quantiles).  Needs no device."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.ndim < 1 or h.shape[-1] != A.PU_DHIST_BUCKETS:
        raise UncoreError(f"histogram_quantiles: the last axis holds {A.PU_DHIST_BUCKETS} buckets")
    q = _ppm_array(ppm)
    flat = h.reshape(-1, A.PU_DHIST_BUCKETS)
    count = np.zeros(len(flat), dtype=np.uint64)
    bucket = np.full((len(flat), max(len(q), 1)), -1, dtype=np.int32)
    for i in range(len(flat)):
        call("pu_dhist_host_quantiles", _as(flat[i], C.c_uint64), _as(q, C.c_uint32), len(q),
             _as(count[i:], C.c_uint64), _as(bucket[i], C.c_int32))
    return count.reshape(h.shape[:-1]), bucket.reshape(h.shape[:-1] + (bucket.shape[1],))


class DeviceDelayHistogram(_DelayStage):
    """Per-replica log-linear delay histograms kept on the device (pu_dhist_*): `add` counts
    every replica's records [begin[r], end[r]) of device request and delay arrays into its
    [2, PU_DHIST_BUCKETS] histogram, bit for bit what delay_histogram gives; `quantiles`
    and `total` are formed on the device.  Pointers are plain integers (tensor.data_ptr()).
    Needs a GPU: there is no host fallback."""
    _prefix = "pu_dhist"

    def __init__(self, count: int, device: int = 0):
        self._n = count
        self._open(count, device)

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Histograms of replicas [first, first + n): uint64 [n, 2, PU_DHIST_BUCKETS] (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros((max(n, 0), 2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
        self._call("read", first, n, _as(out, C.c_uint64))
        return out

    def quantiles(self, ppm, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray]:
        """(count, bucket) of replicas [first, first + n), formed on the device: count uint64 [n, 2],
        bucket int32 [n, 2, len(ppm)] (-1 for an empty class); ppm: up to PU_DHIST_MAX_Q quantiles
        in parts per million.  dhist_bucket_bounds gives the delays a bucket holds."""
        n = self._count(first, n)
        q = _ppm_array(ppm)
        out = np.zeros((max(n, 0), 2), dtype=A.DHIST_Q_DTYPE)
        self._call("quantiles", first, n, _as(q, C.c_uint32), len(q), _as(out, A.DhistQuantile))
        return out["count"].copy(), out["bucket"][:, :, :len(q)].copy()

    def total(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The histogram summed over replicas [first, first + n): uint64 [2, PU_DHIST_BUCKETS].
        Histograms add elementwise, so ranks sum what this returns."""
        out = np.zeros((2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
        self._call("read_total", first, self._count(first, n), _as(out, C.c_uint64))
        return out


# ---------------------------------------------------------------- slowest requests
def delay_tail(reqs: np.ndarray, delays: np.ndarray, k: int, fmt: int = A.PU_REQ_FMT_32, acc=None):
    """The host fold of (request, delay) pairs into one replica's lists of slowest requests
    (pu_dtail_host_add; the rule is in include/primeuncore.h): returns (entries, counts, seen),
    entries A.DTAIL_DTYPE [2, k] (reads and writes apart, best first, zero past the count),
    counts uint32 [2] and seen, the records added so far.  acc, a triple an earlier call
    returned for the same k, is continued (and left unchanged).  reqs as for
    summarize_delays.  Needs no device."""
    reqs, delays = _records(reqs, delays, fmt)
    k = int(k)
    if acc is None:
        entries, counts, seen = np.zeros((2, max(k, 1)), dtype=A.DTAIL_DTYPE), np.zeros(2, dtype=np.uint32), C.c_uint64(0)
    else:
        entries, counts, seen = acc[0].copy(), acc[1].copy(), C.c_uint64(int(acc[2]))
        if entries.shape != (2, k) or entries.dtype != A.DTAIL_DTYPE or counts.shape != (2,) or counts.dtype != np.uint32:
            raise UncoreError(f"delay_tail: acc is not the result of a call with k = {k}")
    call("pu_dtail_host_add", _as(entries, A.DtailEntry), _as(counts, C.c_uint32), C.byref(seen), k,
         reqs.ctypes.data, fmt, _as(delays, C.c_int32), len(delays))
    return entries, counts, int(seen.value)


class DeviceDelayTail(_DelayStage):
    """Per-replica lists of the k slowest reads and the k slowest writes kept on the device
    (pu_dtail_*): `add` offers every replica's records [begin[r], end[r]) of device request and
    delay arrays to its lists, bit for bit what delay_tail gives; `total` is the best k of the
    ensemble, formed on the device.  Pointers are plain integers (tensor.data_ptr()).
    Needs a GPU: there is no host fallback."""
    _prefix = "pu_dtail"

    def __init__(self, count: int, k: int = 16, device: int = 0):
        self._n, self._k = count, k
        self._open(count, k, device)

    @property
    def k(self) -> int:
        """Entries a list holds at most."""
        return int(lib().pu_dtail_k(self._handle()))

    def read(self, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray]:
        """(entries, counts) of replicas [first, first + n): A.DTAIL_DTYPE [n, 2, k], best first and zero
        past the count, and uint32 [n, 2] (waits for the set's calls)."""
        n = self._count(first, n)
        entries = np.zeros((max(n, 0), 2, self._k), dtype=A.DTAIL_DTYPE)
        counts = np.zeros((max(n, 0), 2), dtype=np.uint32)
        self._call("read", first, n, _as(entries, A.DtailEntry), _as(counts, C.c_uint32))
        return entries, counts

    def total(self, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(entries, replicas, counts) of the best k over replicas [first, first + n), per class:
        A.DTAIL_DTYPE [2, k], int32 [2, k] (-1 past the count) and uint32 [2]; by delay descending,
        then replica, then position.  Lists of different ranks merge by the same order on the host."""
        entries = np.zeros((2, self._k), dtype=A.DTAIL_DTYPE)
        replicas = np.full((2, self._k), -1, dtype=np.int32)
        counts = np.zeros(2, dtype=np.uint32)
        self._call("read_total", first, self._count(first, n), _as(entries, A.DtailEntry), _as(replicas, C.c_int32),
                   _as(counts, C.c_uint32))
        return entries, replicas, counts


# ---------------------------------------------------------------- epoch series
def dseries_epoch_of(timer: int, epochs: int, t0: int = 0, shift: int = 0) -> int:
    """The epoch of a record's timer in a series of `epochs` epochs of 2^shift cycles from t0
    (pu_dseries_epoch_of; the rule is in include/primeuncore.h)."""
    return counted("pu_dseries_epoch_of", int(timer), int(epochs), int(t0), int(shift))


def delay_series(reqs: np.ndarray, delays: np.ndarray, epochs: int, t0: int = 0, shift: int = 0,
                 fmt: int = A.PU_REQ_FMT_32, acc=None) -> np.ndarray:
    """The host fold of (request, delay) pairs into one replica's epoch series
    (pu_dseries_host_add; the rule is in include/primeuncore.h): A.DSERIES_DTYPE [2, epochs],
    reads and writes apart, per epoch of the records' own timers count, sum, nonpos (delays
    <= 0) and max (the largest of max(delay, 0)).  acc, an array an earlier call returned for
    the same epochs, is continued (and left unchanged).  reqs as for summarize_delays.
    Needs no device."""
    reqs, delays = _records(reqs, delays, fmt)
    epochs = int(epochs)
    if acc is None:
        cells = np.zeros((2, max(epochs, 1)), dtype=A.DSERIES_DTYPE)
    else:
        cells = acc.copy()
        if cells.shape != (2, epochs) or cells.dtype != A.DSERIES_DTYPE:
            raise UncoreError(f"delay_series: acc is not the result of a call with epochs = {epochs}")
    call("pu_dseries_host_add", _as(cells, A.DseriesCell), epochs, int(t0), int(shift), reqs.ctypes.data, fmt,
         _as(delays, C.c_int32), len(delays))
    return cells


class DeviceDelaySeries(_DelayStage):
    """Per-replica delays over simulated time kept on the device (pu_dseries_*): `add` folds
    every replica's records [begin[r], end[r]) of device request and delay arrays into its
    [2, epochs] cells by the epoch of each record's own timer (2^shift cycles from t0; the
    first and the last epoch are catch-alls), bit for bit what delay_series gives; `total`
    is merged on the device.  Pointers are plain integers (tensor.data_ptr()).
    Needs a GPU: there is no host fallback."""
    _prefix = "pu_dseries"

    def __init__(self, count: int, epochs: int, t0: int = 0, shift: int = 0, device: int = 0):
        self._n, self._e = count, epochs
        self._open(count, epochs, t0, shift, device)

    @property
    def epochs(self) -> int:
        """Epochs of a replica's series."""
        return int(lib().pu_dseries_epochs(self._handle()))

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Cells of replicas [first, first + n): A.DSERIES_DTYPE [n, 2, epochs] (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros((max(n, 0), 2, self._e), dtype=A.DSERIES_DTYPE)
        self._call("read", first, n, _as(out, A.DseriesCell))
        return out

    def total(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The cells merged over replicas [first, first + n): A.DSERIES_DTYPE [2, epochs]; count,
        sum and nonpos add, max is the largest, so ranks merge what this returns the same way."""
        out = np.zeros((2, self._e), dtype=A.DSERIES_DTYPE)
        self._call("read_total", first, self._count(first, n), _as(out, A.DseriesCell))
        return out
