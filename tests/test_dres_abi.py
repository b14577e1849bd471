"""The end-of-run results' C ABI on the host (pu_dres_*; include/primeuncore.h):
arguments are validated before a device is touched, a set cannot be opened
without a handle (and so not without a GPU), a NULL set is refused, the ctypes
mirror types every entry, the record's C layout equals the numpy dtype, and the
rules of primesim_amd/csrc/run_results_step.h agree with literal arithmetic
(tests/cpp/queue_header_check.cpp, a stand-alone program built with the host's
address and undefined-behaviour sanitizers)."""
import ctypes as C
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

PREC = C.POINTER(A.DresReplica)
P64 = C.POINTER(C.c_uint64)


def test_open_refuses_unknown_flags_and_a_null_handle():
    for flags in (2, 3, -1, 1 << 20):
        assert not lib().pu_dres_open(None, flags)
        assert "unknown flags" in U.last_error()
    for flags in (0, A.PU_DRES_QUEUES):
        assert not lib().pu_dres_open(None, flags)
        assert "no handle" in U.last_error()


def test_python_open_needs_an_initialised_manager():
    """Without a GPU no UncoreManager can be initialised, so no set can be opened: both fail loudly."""
    um = P.UncoreManager()
    with pytest.raises(P.UncoreError):
        P.DeviceRunResults(um)
    with pytest.raises(P.UncoreError):
        P.host_run_results(um)
    if not gpu_present():
        with pytest.raises(P.UncoreError, match="no HIP device"):
            um.init(P.config_from_dict(CF.preset("C1")))
        with pytest.raises(P.UncoreError):
            P.DeviceRunResults(um, queues=True)


def test_null_set_and_null_handle_are_refused():
    L = lib()
    rec = np.zeros(2, dtype=A.DRES_DTYPE)
    q = np.zeros(64, dtype=np.uint64)
    pr, pq = rec.ctypes.data_as(PREC), q.ctypes.data_as(P64)
    assert L.pu_dres_gather(None, 0, 1, None) == -22
    assert L.pu_dres_read(None, 0, 1, pr) == -22
    assert L.pu_dres_read(None, 0, 0, None) == -22
    assert L.pu_dres_read_queues(None, 0, pq, pq, 64) == -22
    assert L.pu_dres_read_queue_totals(None, pq, pq, 64) == -22
    assert L.pu_dres_nqueues(None) == 0 and L.pu_dres_state_bytes(None) == 0
    assert L.pu_num_queues(None) == 0 and L.pu_num_links(None) == 0
    L.pu_dres_close(None)
    assert L.pu_dres_host_gather(None, 0, pr, None, None, 0) == -22
    assert "pu_dres_host_gather" in U.last_error()
    assert not rec.view(np.uint8).any() and not q.any()


def test_queue_ends_validates_its_arguments():
    L = lib()
    cfg = P.config_from_dict(CF.preset("C1"))
    k, a, b = C.c_int(7), C.c_int(7), C.c_int(7)
    assert L.pu_config_queue_ends(None, 0, C.byref(k), C.byref(a), C.byref(b)) == -22
    assert L.pu_config_queue_ends(C.byref(cfg), 0, None, C.byref(a), C.byref(b)) == -22
    assert L.pu_config_queue_ends(C.byref(cfg), 0, C.byref(k), None, C.byref(b)) == -22
    assert L.pu_config_queue_ends(C.byref(cfg), 0, C.byref(k), C.byref(a), None) == -22
    assert (k.value, a.value, b.value) == (7, 7, 7)
    bad = P.config_from_dict(CF.preset("C1"))
    bad.sys.num_levels = 0                              # what pu_create refuses, this refuses too
    assert L.pu_config_queue_ends(C.byref(bad), 0, C.byref(k), C.byref(a), C.byref(b)) == -22
    assert "num_levels" in U.last_error()
    assert L.pu_config_queue_ends(C.byref(cfg), 0, C.byref(k), C.byref(a), C.byref(b)) == 0
    assert (k.value, a.value, b.value) == (0, 0, 1)


def test_mirror_declares_every_dres_entry():
    L = lib()
    V, PI = C.c_void_p, C.POINTER(C.c_int)
    want = {
        "pu_dres_open": (V, [V, C.c_int]),
        "pu_dres_close": (None, [V]),
        "pu_dres_gather": (C.c_int, [V, C.c_int, C.c_int, V]),
        "pu_dres_read": (C.c_int, [V, C.c_int, C.c_int, PREC]),
        "pu_dres_read_queues": (C.c_int, [V, C.c_int, P64, P64, C.c_size_t]),
        "pu_dres_read_queue_totals": (C.c_int, [V, P64, P64, C.c_size_t]),
        "pu_dres_nqueues": (C.c_int, [V]),
        "pu_dres_state_bytes": (C.c_uint64, [V]),
        "pu_num_links": (C.c_int, [V]),
        "pu_num_queues": (C.c_int, [V]),
        "pu_dres_host_gather": (C.c_int, [V, C.c_int, PREC, P64, P64, C.c_size_t]),
        "pu_config_queue_ends": (C.c_int, [C.POINTER(A.SimCfg), C.c_int, PI, PI, PI]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert "#define PU_DRES_QUEUES 1" in header and A.PU_DRES_QUEUES == 1
    assert P.DeviceRunResults is U.DeviceRunResults and "DeviceRunResults" in P.__all__
    assert "host_run_results" in P.__all__ and "queue_ends" in P.__all__


def _flat(dtype, prefix=""):
    """(dotted name, offset, size) of every scalar of a structured dtype."""
    out = []
    for name in dtype.names:
        sub, off = dtype.fields[name][:2]
        base, shape = (sub.subdtype if sub.subdtype else (sub, ()))
        n = int(np.prod(shape)) if shape else 1
        for k in range(n):
            tag = f"{prefix}{name}" + (f"[{k}]" if shape else "")
            at = off + k * base.itemsize
            if base.names:
                out += [(t, at + o, s) for t, o, s in _flat(base, tag + ".")]
            else:
                out.append((tag, at, base.itemsize))
    return out


def _flat_c(struct, prefix="", base_off=0):
    out = []
    for name, typ in struct._fields_:
        off = base_off + getattr(struct, name).offset
        if issubclass(typ, C.Array):
            el = typ._type_
            for k in range(typ._length_):
                tag, at = f"{prefix}{name}[{k}]", off + k * C.sizeof(el)
                out += _flat_c(el, tag + ".", at) if issubclass(el, C.Structure) else [(tag, at, C.sizeof(el))]
        elif issubclass(typ, C.Structure):
            out += _flat_c(typ, f"{prefix}{name}.", off)
        else:
            out.append((f"{prefix}{name}", off, C.sizeof(typ)))
    return out


def test_record_layout_equals_the_numpy_dtype():
    """sizeof(pu_dres_replica) = 448 with no hidden padding: the scalars tile the record, and the
    ctypes structure, the numpy dtype and the header's comment agree."""
    assert C.sizeof(A.DresReplica) == A.DRES_DTYPE.itemsize == 448
    assert C.sizeof(A.Stats) == A.STATS_DTYPE.itemsize == 352
    c, n = _flat_c(A.DresReplica), _flat(A.DRES_DTYPE)
    assert c == n
    at = 0
    for _, off, size in c:                              # contiguous: a snapshot has no undefined byte
        assert off == at
        at += size
    assert at == 448
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        assert "} pu_dres_replica;                  /* 448 bytes */" in f.read()


def test_header_decode_fold_and_tie_rule_equal_literal_arithmetic(tmp_path):
    """7 edge counts x 128 cursor values + 100,000 random pairs; the completion fold and the
    busiest-queue rule against sequential loops."""
    assert run_cpp_check(tmp_path, "queue_header_check.cpp").startswith("OK 100896 headers")


def test_the_stats_rule_writes_every_field_from_its_source(tmp_path):
    """pu::stats_fill (stats_rule.h), the one rule pu_stats_get and the device gather share: 45 fields
    against their literals for 1 and for 4 levels, on a record pre-filled with 0xA5."""
    assert run_cpp_check(tmp_path, "stats_rule_check.cpp").startswith("OK 90 fields")
