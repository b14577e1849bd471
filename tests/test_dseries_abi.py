"""The C ABI of the epoch series on the host (pu_dseries_*; include/primeuncore.h): arguments
are validated before a device is touched, creation fails loudly where there is no GPU, a
NULL set is answered like a NULL pu_dhist, the ctypes mirror types every entry, and the rule
(primesim_amd/csrc/delay_series_step.h) agrees with plain statements of it
(tests/cpp/delay_series_check.cpp, a stand-alone program built with the host's address and
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

PC, PI32 = C.POINTER(A.DseriesCell), C.POINTER(C.c_int32)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.mark.parametrize("count", [0, -1])
def test_open_refuses_no_replicas(count):
    assert not lib().pu_dseries_open(count, 8, 0, 0, 0)
    assert "pu_dseries_open" in U.last_error() and "no replicas" in U.last_error()
    with pytest.raises(P.UncoreError, match="no replicas"):
        P.DeviceDelaySeries(count, 8)


@pytest.mark.parametrize("epochs", [0, -1, 513])
def test_open_refuses_epochs_outside_1_to_512(epochs):
    assert not lib().pu_dseries_open(2, epochs, 0, 0, 0)
    assert "between 1 and 512 epochs" in U.last_error()
    with pytest.raises(P.UncoreError, match="between 1 and 512 epochs"):
        P.DeviceDelaySeries(2, epochs)


@pytest.mark.parametrize("shift", [-1, 63])
def test_open_refuses_a_shift_outside_0_to_62(shift):
    assert not lib().pu_dseries_open(2, 8, 0, shift, 0)
    assert "shift between 0 and 62" in U.last_error()
    with pytest.raises(P.UncoreError, match="shift between 0 and 62"):
        P.DeviceDelaySeries(2, 8, shift=shift)


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    assert not lib().pu_dseries_open(2, 8, 0, 0, 0)
    assert "no HIP device" in U.last_error() and "no CPU fallback" in U.last_error()
    assert "pu_dseries_host_add" in U.last_error()                 # the host twin is named
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceDelaySeries(1, 8)


def test_null_set_is_refused():
    L = lib()
    cells = np.zeros((2, 4), dtype=A.DSERIES_DTYPE)
    p = cells.ctypes.data
    assert L.pu_dseries_add(None, p, A.PU_REQ_FMT_32, p, p, p, None) == -22
    assert "pu_dseries_add: bad arguments" in U.last_error()
    assert L.pu_dseries_add(None, None, A.PU_REQ_FMT_32, None, None, None, None) == -22
    assert L.pu_dseries_read(None, 0, 0, None) == -22
    assert L.pu_dseries_read(None, 0, 1, cells.ctypes.data_as(PC)) == -22
    assert L.pu_dseries_read_total(None, 0, 1, cells.ctypes.data_as(PC)) == -22
    assert L.pu_dseries_read_total(None, 0, 0, cells.ctypes.data_as(PC)) == -22
    assert L.pu_dseries_reset(None) == -22
    assert L.pu_dseries_state_bytes(None) == 0
    assert L.pu_dseries_epochs(None) == 0
    L.pu_dseries_close(None)
    assert not cells.view(np.uint8).any()


def test_epoch_of_checks_its_parameters_and_keeps_the_rule():
    L = lib()
    for epochs, shift in ((0, 0), (-1, 0), (513, 0), (8, -1), (8, 63)):
        assert L.pu_dseries_epoch_of(5, epochs, 0, shift) == -22, (epochs, shift)
        assert "pu_dseries_epoch_of" in U.last_error()
        with pytest.raises(P.UncoreError, match=r"pu_dseries_epoch_of.*\(-22\)"):
            P.dseries_epoch_of(5, epochs, 0, shift)
    assert [P.dseries_epoch_of(t, 8, 100, 4) for t in (I64_MIN, 99, 100, 115, 116, 211, 212, I64_MAX)] == [0, 0, 0, 0, 1, 6, 7, 7]
    assert P.dseries_epoch_of(I64_MAX, 512, I64_MIN, 62) == 3 and P.dseries_epoch_of(I64_MAX, 512, I64_MIN, 0) == 511
    assert P.dseries_epoch_of(I64_MIN, 512, I64_MAX, 0) == 0 and P.dseries_epoch_of(I64_MAX, 1, 0, 0) == 0


def _host_add(cells, epochs, t0, shift, reqs, fmt, delays, n):
    return lib().pu_dseries_host_add(None if cells is None else cells.ctypes.data_as(PC), epochs, t0, shift,
                                     None if reqs is None else reqs.ctypes.data, fmt,
                                     None if delays is None else delays.ctypes.data_as(PI32), n)


def test_host_add_validates_its_arguments():
    E = 3
    cells = np.zeros((2, E), dtype=A.DSERIES_DTYPE)
    reqs = np.zeros(5, dtype=A.REQ_DTYPE)
    reqs["timer"], reqs["mem_type"] = [0, 1, 2, 3, 100], [0, 1, 0, 1, 0]
    delays = np.array([5, -1, 0, 7, 2147483647], dtype=np.int32)
    ok = (cells, E, 0, 0, reqs, A.PU_REQ_FMT_32, delays, 5)
    for at, bad in ((0, None), (1, 0), (1, -1), (1, 513), (3, -1), (3, 63), (4, None), (5, 2), (5, -1), (6, None)):
        args = list(ok)
        args[at] = bad
        assert _host_add(*args) == -22, (at, bad)
        assert "pu_dseries_host_add" in U.last_error()
    assert not cells.view(np.uint8).any()                                          # nothing was written
    assert _host_add(cells, E, 0, 0, None, A.PU_REQ_FMT_32, None, 0) == 0          # nothing to add is fine
    assert not cells.view(np.uint8).any()
    assert _host_add(*ok) == 0
    assert cells["count"].tolist() == [[1, 0, 2], [0, 1, 1]] and cells["sum"].tolist() == [[5, 0, 2147483647], [0, -1, 7]]
    assert cells["nonpos"].tolist() == [[0, 0, 1], [0, 1, 0]] and cells["max"].tolist() == [[5, 0, 2147483647], [0, 0, 7]]
    assert not cells["_pad"].any()


def test_mirror_declares_every_dseries_entry():
    L = lib()
    V = C.c_void_p
    want = {
        "pu_dseries_open": (V, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]),
        "pu_dseries_close": (None, [V]),
        "pu_dseries_add": (C.c_int, [V, V, C.c_int, V, V, V, V]),
        "pu_dseries_read": (C.c_int, [V, C.c_int, C.c_int, PC]),
        "pu_dseries_read_total": (C.c_int, [V, C.c_int, C.c_int, PC]),
        "pu_dseries_reset": (C.c_int, [V]),
        "pu_dseries_state_bytes": (C.c_uint64, [V]),
        "pu_dseries_epochs": (C.c_int, [V]),
        "pu_dseries_host_add": (C.c_int, [PC, C.c_int, C.c_int64, C.c_int, V, C.c_int, PI32, C.c_size_t]),
        "pu_dseries_epoch_of": (C.c_int, [C.c_int64, C.c_int, C.c_int64, C.c_int]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert "#define PU_DSERIES_MAX_EPOCHS 512" in header and A.PU_DSERIES_MAX_EPOCHS == 512
    assert C.sizeof(A.DseriesCell) == 32 == A.DSERIES_DTYPE.itemsize
    for name, offset in (("count", 0), ("sum", 8), ("nonpos", 16), ("max", 24), ("_pad", 28)):
        assert getattr(A.DseriesCell, name).offset == A.DSERIES_DTYPE.fields[name][1] == offset, name
    for name in ("DeviceDelaySeries", "delay_series", "dseries_epoch_of"):
        assert getattr(P, name) is getattr(U, name), name
    assert P.DeviceDelaySeries._prefix == "pu_dseries"
    assert P.DeviceDelaySeries.add is P.DeviceDelayHistogram.add and P.DeviceDelaySeries.reset is P.DeviceDelayHistogram.reset


def test_rule_equals_plain_statements_of_it(tmp_path):
    assert run_cpp_check(tmp_path, "delay_series_check.cpp").startswith("OK 203531 checks")
