"""The delay summaries' C ABI on the host (pu_dsum_*; include/primeuncore.h):
arguments are validated before a device is touched, creation fails loudly where
there is no GPU, a NULL set is answered like a NULL pu_dstream, the ctypes mirror
types every entry, and the bucket rule (primesim_amd/csrc/delay_sum_step.h) agrees
with a loop of comparisons (tests/cpp/delay_bucket_check.cpp, a stand-alone program
built with the host's address and undefined-behaviour sanitizers)."""
import ctypes as C
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


@pytest.mark.parametrize("count", [0, -1])
def test_open_refuses_no_replicas(count):
    assert not lib().pu_dsum_open(count, None, 0)
    assert "no replicas" in U.last_error()
    assert not lib().pu_dsum_open(count, _i32(4), 0)
    assert "no replicas" in U.last_error()
    with pytest.raises(P.UncoreError, match="no replicas"):
        P.DeviceDelaySummary(count)


@pytest.mark.parametrize("bad", [0, -1, -(1 << 31)])
@pytest.mark.parametrize("where", [0, 1, 2])
def test_open_validates_every_num_cores_before_a_device(bad, where):
    """One invalid entry among valid ones: NULL and an error text, GPU or not."""
    nc = [16, 1, 1024]
    nc[where] = bad
    assert not lib().pu_dsum_open(3, _i32(*nc), 0)
    err = U.last_error()
    assert "invalid num_cores" in err and f"replica {where}" in err
    with pytest.raises(P.UncoreError, match="invalid num_cores"):
        P.DeviceDelaySummary(3, num_cores=nc)


def test_python_open_wants_one_num_cores_per_replica():
    with pytest.raises(P.UncoreError, match="2 num_cores entries for 3 replicas"):
        P.DeviceDelaySummary(3, num_cores=[4, 4])


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    assert not lib().pu_dsum_open(2, None, 0)
    assert "no HIP device" in U.last_error()
    assert not lib().pu_dsum_open(2, _i32(16, 1024), 0)
    assert "no HIP device" in U.last_error()
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceDelaySummary(1)
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceDelaySummary(2, num_cores=[3, 70000])


def test_null_set_is_refused():
    L = lib()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    assert L.pu_dsum_add(None, p, A.PU_REQ_FMT_32, p, p, p, None) == -22
    assert L.pu_dsum_add(None, None, A.PU_REQ_FMT_32, None, None, None, None) == -22
    assert L.pu_dsum_read(None, 0, 0, None) == -22
    assert L.pu_dsum_read_cores(None, 0, None, None, 0) == -22
    assert L.pu_dsum_reset(None) == -22
    assert L.pu_dsum_state_bytes(None) == 0
    L.pu_dsum_close(None)
    L.pu_dsum_host_init(None)


def _host_add(acc, cnt, sm, nc, reqs, fmt, delays, n):
    P64, PI64, PI32 = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    return lib().pu_dsum_host_add(
        None if acc is None else acc.ctypes.data_as(C.POINTER(A.DsumReplica)),
        None if cnt is None else cnt.ctypes.data_as(P64), None if sm is None else sm.ctypes.data_as(PI64), nc,
        None if reqs is None else reqs.ctypes.data, fmt, None if delays is None else delays.ctypes.data_as(PI32), n)


def test_host_add_validates_its_arguments():
    acc = np.zeros(1, dtype=A.DSUM_DTYPE)
    reqs = np.zeros(4, dtype=A.REQ_DTYPE)
    delays = np.ones(4, dtype=np.int32)
    cnt, sm = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int64)
    assert _host_add(None, None, None, 0, reqs, A.PU_REQ_FMT_32, delays, 4) == -22
    assert "pu_dsum_host_add" in U.last_error()
    assert _host_add(acc, None, None, 0, reqs, 2, delays, 4) == -22            # no such format
    assert _host_add(acc, None, None, 0, reqs, -1, delays, 4) == -22
    assert _host_add(acc, None, None, 0, None, A.PU_REQ_FMT_32, delays, 4) == -22
    assert _host_add(acc, None, None, 0, reqs, A.PU_REQ_FMT_32, None, 4) == -22
    assert _host_add(acc, cnt, None, 2, reqs, A.PU_REQ_FMT_32, delays, 4) == -22   # one table without the other
    assert _host_add(acc, None, sm, 2, reqs, A.PU_REQ_FMT_32, delays, 4) == -22
    assert _host_add(acc, cnt, sm, 0, reqs, A.PU_REQ_FMT_32, delays, 4) == -22     # tables need num_cores >= 1
    assert not acc.view(np.uint8).any()                                          # nothing was folded
    lib().pu_dsum_host_init(acc.ctypes.data_as(C.POINTER(A.DsumReplica)))
    assert _host_add(acc, None, None, 0, None, A.PU_REQ_FMT_32, None, 0) == 0      # nothing to add is fine
    assert _host_add(acc, cnt, sm, 2, reqs, A.PU_REQ_FMT_32, delays, 4) == 0
    assert acc[0]["cls"][0]["count"] == 4 and cnt[0] == 4 and sm[0] == 4


def test_mirror_declares_every_dsum_entry():
    L = lib()
    V, PR = C.c_void_p, C.POINTER(A.DsumReplica)
    P64, PI64, PI32 = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    want = {
        "pu_dsum_open": (V, [C.c_int, PI32, C.c_int]),
        "pu_dsum_close": (None, [V]),
        "pu_dsum_add": (C.c_int, [V, V, C.c_int, V, V, V, V]),
        "pu_dsum_read": (C.c_int, [V, C.c_int, C.c_int, PR]),
        "pu_dsum_read_cores": (C.c_int, [V, C.c_int, P64, PI64, C.c_size_t]),
        "pu_dsum_reset": (C.c_int, [V]),
        "pu_dsum_state_bytes": (C.c_uint64, [V]),
        "pu_dsum_host_init": (None, [PR]),
        "pu_dsum_host_add": (C.c_int, [PR, P64, PI64, C.c_int, V, C.c_int, PI32, C.c_size_t]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert "#define PU_DSUM_BUCKETS 32" in header and A.PU_DSUM_BUCKETS == 32
    # the structures: sizes and field offsets of the C layout (8-byte members, no hidden padding)
    assert C.sizeof(A.DsumClass) == 8 + 8 + 4 + 4 + 32 * 8 == A.DSUM_CLASS_DTYPE.itemsize
    assert C.sizeof(A.DsumReplica) == 2 * 280 + 8 == A.DSUM_DTYPE.itemsize
    for f in ("count", "sum", "min", "max", "hist"):
        assert getattr(A.DsumClass, f).offset == A.DSUM_CLASS_DTYPE.fields[f][1], f
    assert A.DsumReplica.core_out_of_range.offset == A.DSUM_DTYPE.fields["core_out_of_range"][1] == 560
    assert P.DeviceDelaySummary is U.DeviceDelaySummary and P.summarize_delays is U.summarize_delays
    assert "DeviceDelaySummary" in P.__all__ and "summarize_delays" in P.__all__


def test_bucket_rule_equals_a_loop_of_comparisons(tmp_path):
    assert run_cpp_check(tmp_path, "delay_bucket_check.cpp").startswith("OK 1000068 delays")
