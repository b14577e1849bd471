"""The log-linear delay histograms' C ABI on the host (pu_dhist_*; include/primeuncore.h):
arguments are validated before a device is touched, creation fails loudly where there
is no GPU, a NULL set is answered like a NULL pu_dsum, the ctypes mirror types every
entry, and the rule (primesim_amd/csrc/delay_hist_step.h) agrees with plain statements
of it (tests/cpp/delay_hist_check.cpp, a stand-alone program built with the host's
address and undefined-behaviour sanitizers)."""
import ctypes as C
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

P64, P32, PI32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.mark.parametrize("count", [0, -1])
def test_open_refuses_no_replicas(count):
    assert not lib().pu_dhist_open(count, 0)
    assert "no replicas" in U.last_error()
    with pytest.raises(P.UncoreError, match="no replicas"):
        P.DeviceDelayHistogram(count)


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    assert not lib().pu_dhist_open(2, 0)
    assert "no HIP device" in U.last_error() and "no CPU fallback" in U.last_error()
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceDelayHistogram(1)


def test_null_set_is_refused():
    L = lib()
    buf = np.zeros(2 * A.PU_DHIST_BUCKETS, dtype=np.uint64)
    p = buf.ctypes.data
    ppm = (C.c_uint32 * 1)(500000)
    q = (A.DhistQuantile * 2)()
    assert L.pu_dhist_add(None, p, A.PU_REQ_FMT_32, p, p, p, None) == -22
    assert L.pu_dhist_add(None, None, A.PU_REQ_FMT_32, None, None, None, None) == -22
    assert L.pu_dhist_read(None, 0, 0, None) == -22
    assert L.pu_dhist_read(None, 0, 1, buf.ctypes.data_as(P64)) == -22
    assert L.pu_dhist_quantiles(None, 0, 1, ppm, 1, q) == -22
    assert L.pu_dhist_read_total(None, 0, 1, buf.ctypes.data_as(P64)) == -22
    assert L.pu_dhist_reset(None) == -22
    assert L.pu_dhist_state_bytes(None) == 0
    L.pu_dhist_close(None)
    assert not buf.any()


def _host_add(hist, reqs, fmt, delays, n):
    return lib().pu_dhist_host_add(None if hist is None else hist.ctypes.data_as(P64),
                                   None if reqs is None else reqs.ctypes.data, fmt,
                                   None if delays is None else delays.ctypes.data_as(PI32), n)


def test_host_add_validates_its_arguments():
    hist = np.zeros((2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
    reqs = np.zeros(4, dtype=A.REQ_DTYPE)
    delays = np.full(4, 70, dtype=np.int32)
    assert _host_add(None, reqs, A.PU_REQ_FMT_32, delays, 4) == -22
    assert "pu_dhist_host_add" in U.last_error()
    assert _host_add(hist, reqs, 2, delays, 4) == -22              # no such format
    assert _host_add(hist, reqs, -1, delays, 4) == -22
    assert _host_add(hist, None, A.PU_REQ_FMT_32, delays, 4) == -22
    assert _host_add(hist, reqs, A.PU_REQ_FMT_32, None, 4) == -22
    assert not hist.any()                                          # nothing was counted
    assert _host_add(hist, None, A.PU_REQ_FMT_32, None, 0) == 0      # nothing to add is fine
    assert _host_add(hist, reqs, A.PU_REQ_FMT_32, delays, 4) == 0
    assert hist[0, 67] == 4 and hist.sum() == 4                    # 70 is in [70, 71]


def _host_q(hist, ppm, nq, want_count=True):
    count = C.c_uint64(77)
    out = (C.c_int32 * A.PU_DHIST_MAX_Q)(*([-9] * A.PU_DHIST_MAX_Q))
    arr = None if ppm is None else (C.c_uint32 * max(len(ppm), 1))(*ppm)
    rc = lib().pu_dhist_host_quantiles(None if hist is None else hist.ctypes.data_as(P64), arr, nq,
                                       C.byref(count) if want_count else None, out)
    return rc, count.value, list(out)


def test_host_quantiles_validate_their_arguments():
    hist = np.zeros(A.PU_DHIST_BUCKETS, dtype=np.uint64)
    hist[5] = 2
    for bad in ((None, [1], 1), (hist, None, 1), (hist, [1], 0), (hist, [1], -1), (hist, [1] * 9, 9),
                (hist, [1000001], 1), (hist, [0, 1 << 31], 2)):
        rc, count, out = _host_q(*bad)
        assert rc == -22 and count == 77 and out == [-9] * 8, bad    # nothing was written
        assert "pu_dhist_host_quantiles" in U.last_error()
    assert lib().pu_dhist_host_quantiles(hist.ctypes.data_as(P64), (C.c_uint32 * 1)(1), 1, None, None) == -22
    rc, count, out = _host_q(hist, [0, 1000000], 2)
    assert rc == 0 and count == 2 and out == [5, 5] + [-9] * 6      # only nq entries are written
    rc, _, out = _host_q(hist, [500000] * 8, 8, want_count=False)    # the count is optional
    assert rc == 0 and out == [5] * 8
    with pytest.raises(P.UncoreError, match=r"pu_dhist_host_quantiles.*\(-22\)"):
        P.histogram_quantiles(hist, [1000001])
    with pytest.raises(P.UncoreError, match=r"pu_dhist_host_quantiles.*\(-22\)"):
        P.histogram_quantiles(hist, list(range(9)))
    with pytest.raises(P.UncoreError, match="864 buckets"):
        P.histogram_quantiles(np.zeros(32, dtype=np.uint64), [1])
    with pytest.raises(P.UncoreError, match="ppm"):
        P.histogram_quantiles(hist, [-1])


def test_bucket_entries():
    L = lib()
    assert [L.pu_dhist_bucket_of(d) for d in (-(1 << 31), -1, 0, 1, 63, 64, 65, 66, (1 << 31) - 1)] == \
        [0, 0, 0, 1, 63, 64, 64, 65, 863]
    lo, hi = C.c_int32(5), C.c_int32(5)
    for k in (-1, 864, 1 << 20):
        assert L.pu_dhist_bucket_bounds(k, C.byref(lo), C.byref(hi)) == -34
        assert "no such bucket" in U.last_error() and lo.value == hi.value == 5
    assert L.pu_dhist_bucket_bounds(3, None, C.byref(hi)) == -22
    assert L.pu_dhist_bucket_bounds(3, C.byref(lo), None) == -22
    assert P.dhist_bucket_bounds(0) == (-(1 << 31), 0) and P.dhist_bucket_bounds(64) == (64, 65)
    assert P.dhist_bucket_bounds(863) == ((1 << 31) - (1 << 25), (1 << 31) - 1)
    assert P.dhist_bucket_of(131) == 96 and P.dhist_bucket_of(132) == 97
    with pytest.raises(P.UncoreError, match=r"\(-34\)"):
        P.dhist_bucket_bounds(864)


def test_mirror_declares_every_dhist_entry():
    L = lib()
    V, PQ = C.c_void_p, C.POINTER(A.DhistQuantile)
    want = {
        "pu_dhist_open": (V, [C.c_int, C.c_int]),
        "pu_dhist_close": (None, [V]),
        "pu_dhist_add": (C.c_int, [V, V, C.c_int, V, V, V, V]),
        "pu_dhist_read": (C.c_int, [V, C.c_int, C.c_int, P64]),
        "pu_dhist_quantiles": (C.c_int, [V, C.c_int, C.c_int, P32, C.c_int, PQ]),
        "pu_dhist_read_total": (C.c_int, [V, C.c_int, C.c_int, P64]),
        "pu_dhist_reset": (C.c_int, [V]),
        "pu_dhist_state_bytes": (C.c_uint64, [V]),
        "pu_dhist_host_add": (C.c_int, [P64, V, C.c_int, PI32, C.c_size_t]),
        "pu_dhist_host_quantiles": (C.c_int, [P64, P32, C.c_int, P64, PI32]),
        "pu_dhist_bucket_of": (C.c_int, [C.c_int32]),
        "pu_dhist_bucket_bounds": (C.c_int, [C.c_int, PI32, PI32]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    for define, value in (("PU_DHIST_SUB_BITS 5", A.PU_DHIST_SUB_BITS == 5), ("PU_DHIST_BUCKETS  864", A.PU_DHIST_BUCKETS == 864),
                          ("PU_DHIST_MAX_Q    8", A.PU_DHIST_MAX_Q == 8)):
        assert f"#define {define}" in header and value, define
    assert C.sizeof(A.DhistQuantile) == 8 + 8 * 4 == A.DHIST_Q_DTYPE.itemsize
    assert A.DhistQuantile.bucket.offset == A.DHIST_Q_DTYPE.fields["bucket"][1] == 8
    for name in ("DeviceDelayHistogram", "delay_histogram", "histogram_quantiles", "dhist_bucket_of", "dhist_bucket_bounds"):
        assert getattr(P, name) is getattr(U, name) and name in P.__all__, name
    assert b" src " in L.pu_version()


def test_rule_equals_plain_statements_of_it(tmp_path):
    assert run_cpp_check(tmp_path, "delay_hist_check.cpp").startswith("OK 1003458 delays")
