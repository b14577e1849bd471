"""The C ABI of the slowest-request lists on the host (pu_dtail_*; include/primeuncore.h):
arguments are validated before a device is touched, creation fails loudly where there is no
GPU, a NULL set is answered like a NULL pu_dhist, the ctypes mirror types every entry, and
the rule (primesim_amd/csrc/delay_tail_step.h) agrees with plain statements of it
(tests/cpp/delay_tail_check.cpp, a stand-alone program built with the host's address and
undefined-behaviour sanitizers)."""
import ctypes as C
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

PE, P64, P32, PI32 = C.POINTER(A.DtailEntry), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.mark.parametrize("count", [0, -1])
def test_open_refuses_no_replicas(count):
    assert not lib().pu_dtail_open(count, 16, 0)
    assert "no replicas" in U.last_error()
    with pytest.raises(P.UncoreError, match="no replicas"):
        P.DeviceDelayTail(count)


@pytest.mark.parametrize("k", [0, -1, 65, 1 << 20])
def test_open_refuses_a_list_length_outside_1_to_64(k):
    assert not lib().pu_dtail_open(2, k, 0)
    assert "between 1 and 64 entries" in U.last_error()
    with pytest.raises(P.UncoreError, match="between 1 and 64 entries"):
        P.DeviceDelayTail(2, k=k)


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    assert not lib().pu_dtail_open(2, 16, 0)
    assert "no HIP device" in U.last_error() and "no CPU fallback" in U.last_error()
    assert "pu_dtail_host_add" in U.last_error()                   # the host twin is named
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceDelayTail(1)


def test_null_set_is_refused():
    L = lib()
    ent = np.zeros((2, 4), dtype=A.DTAIL_DTYPE)
    rep = np.zeros((2, 4), dtype=np.int32)
    cnt = np.zeros(2, dtype=np.uint32)
    p = ent.ctypes.data
    assert L.pu_dtail_add(None, p, A.PU_REQ_FMT_32, p, p, p, None) == -22
    assert "pu_dtail_add: bad arguments" in U.last_error()
    assert L.pu_dtail_add(None, None, A.PU_REQ_FMT_32, None, None, None, None) == -22
    assert L.pu_dtail_read(None, 0, 0, None, None) == -22
    assert L.pu_dtail_read(None, 0, 1, ent.ctypes.data_as(PE), cnt.ctypes.data_as(P32)) == -22
    assert L.pu_dtail_read_total(None, 0, 1, ent.ctypes.data_as(PE), rep.ctypes.data_as(PI32), cnt.ctypes.data_as(P32)) == -22
    assert L.pu_dtail_reset(None) == -22
    assert L.pu_dtail_state_bytes(None) == 0
    assert L.pu_dtail_k(None) == 0
    L.pu_dtail_close(None)
    assert not ent.view(np.uint8).any() and not rep.any() and not cnt.any()


def _host_add(entries, counts, seen, k, reqs, fmt, delays, n):
    return lib().pu_dtail_host_add(None if entries is None else entries.ctypes.data_as(PE),
                                   None if counts is None else counts.ctypes.data_as(P32),
                                   None if seen is None else seen.ctypes.data_as(P64), k,
                                   None if reqs is None else reqs.ctypes.data, fmt,
                                   None if delays is None else delays.ctypes.data_as(PI32), n)


def test_host_add_validates_its_arguments():
    k = 3
    ent = np.zeros((2, k), dtype=A.DTAIL_DTYPE)
    cnt = np.zeros(2, dtype=np.uint32)
    seen = np.zeros(1, dtype=np.uint64)
    reqs = np.zeros(4, dtype=A.REQ_DTYPE)
    reqs["addr"], reqs["timer"], reqs["core"] = [10, 20, 30, 40], [1, 2, 3, 4], [5, 6, 7, 8]
    delays = np.array([70, 90, 70, 80], dtype=np.int32)
    ok = (ent, cnt, seen, k, reqs, A.PU_REQ_FMT_32, delays, 4)
    for at, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -1), (3, 65), (4, None), (5, 2), (5, -1), (6, None)):
        args = list(ok)
        args[at] = bad
        assert _host_add(*args) == -22, (at, bad)
        assert "pu_dtail_host_add" in U.last_error()
    assert not ent.view(np.uint8).any() and not cnt.any() and not seen.any()      # nothing was written
    assert _host_add(ent, cnt, seen, k, None, A.PU_REQ_FMT_32, None, 0) == 0       # nothing to add is fine
    assert not cnt.any() and seen[0] == 0
    assert _host_add(*ok) == 0
    assert list(cnt) == [3, 0] and seen[0] == 4
    assert list(ent[0]["delay"]) == [90, 80, 70] and list(ent[0]["position"]) == [1, 3, 0]
    assert list(ent[0]["addr"]) == [20, 40, 10] and list(ent[0]["timer"]) == [2, 4, 1] and list(ent[0]["core"]) == [6, 8, 5]


def test_mirror_declares_every_dtail_entry():
    L = lib()
    V = C.c_void_p
    want = {
        "pu_dtail_open": (V, [C.c_int, C.c_int, C.c_int]),
        "pu_dtail_close": (None, [V]),
        "pu_dtail_add": (C.c_int, [V, V, C.c_int, V, V, V, V]),
        "pu_dtail_read": (C.c_int, [V, C.c_int, C.c_int, PE, P32]),
        "pu_dtail_read_total": (C.c_int, [V, C.c_int, C.c_int, PE, PI32, P32]),
        "pu_dtail_reset": (C.c_int, [V]),
        "pu_dtail_state_bytes": (C.c_uint64, [V]),
        "pu_dtail_k": (C.c_int, [V]),
        "pu_dtail_host_add": (C.c_int, [PE, P32, P64, C.c_int, V, C.c_int, PI32, C.c_size_t]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert "#define PU_DTAIL_MAX_K 64" in header and A.PU_DTAIL_MAX_K == 64
    assert C.sizeof(A.DtailEntry) == 32 == A.DTAIL_DTYPE.itemsize
    for name, offset in (("addr", 0), ("timer", 8), ("position", 16), ("delay", 24), ("core", 28)):
        assert getattr(A.DtailEntry, name).offset == A.DTAIL_DTYPE.fields[name][1] == offset, name
    for name in ("DeviceDelayTail", "delay_tail"):
        assert getattr(P, name) is getattr(U, name) and name in P.__all__, name
    assert b" src " in L.pu_version()


def test_rule_equals_plain_statements_of_it(tmp_path):
    assert run_cpp_check(tmp_path, "delay_tail_check.cpp").startswith("OK 104296 checks")
