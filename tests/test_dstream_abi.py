"""The device stream generator's C ABI on the host (pu_dstream_*,
pu_stream_fits_req16; include/primeuncore.h): parameters are validated before a
device is touched, creation fails loudly where there is no GPU, the format-16
verdict is one-sided against pu_pack_req16, the ctypes mirror types every entry,
and the scan-and-cut rule of the kernel (primesim_amd/csrc/stream_step.h) agrees
with the host generator's sequential loop (tests/cpp/stream_cut_check.cpp, a
stand-alone program built with the host's address and undefined-behaviour
sanitizers)."""
import ctypes as C
import os

import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

KINDS = [A.PU_STREAM_PRIVATE_STREAMING, A.PU_STREAM_SHARED_UNIFORM, A.PU_STREAM_MULTIPROGRAM,
         A.PU_STREAM_UNIFORM_HOTSPOT, A.PU_STREAM_PRODUCER_CONSUMER, A.PU_STREAM_UNIFORM]


def _params(specs):
    return (A.StreamParams * len(specs))(*[s.params() for s in specs])


GOOD = P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 16, seed=3)


def test_open_refuses_no_streams():
    arr = _params([GOOD])
    assert not lib().pu_dstream_open(arr, 0, 0)
    assert U.last_error()
    assert not lib().pu_dstream_open(None, 1, 0)
    assert U.last_error()


@pytest.mark.parametrize("bad", [dict(kind=99), dict(num_cores=0), dict(quantum=0), dict(max_msg=0)])
@pytest.mark.parametrize("where", [0, 1, 2])
def test_open_validates_every_entry_before_a_device(bad, where):
    """One invalid entry among valid ones: NULL and an error text, GPU or not."""
    fields = dict(kind=A.PU_STREAM_UNIFORM, num_cores=8, seed=5)
    fields.update(bad)
    specs = [GOOD, GOOD, GOOD]
    specs[where] = P.StreamSpec(**fields)
    assert not lib().pu_dstream_open(_params(specs), 3, 0)
    err = U.last_error()
    assert "invalid stream parameters" in err and f"stream {where}" in err
    with pytest.raises(P.UncoreError, match="invalid stream parameters"):
        P.DeviceStreamSet(specs)


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    assert not lib().pu_dstream_open(_params([GOOD, GOOD]), 2, 0)
    assert "no HIP device" in U.last_error()
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceStreamSet([GOOD])


def test_null_set_is_refused():
    assert lib().pu_dstream_next(None, None, 0, 0, A.PU_REQ_FMT_32, None, None) == -22
    assert lib().pu_dstream_positions(None, None, 0) == -22
    assert lib().pu_dstream_state_bytes(None) == 0
    lib().pu_dstream_close(None)


@pytest.mark.parametrize("fields,fits", [
    (dict(num_cores=65536), True),
    (dict(num_cores=65537), False),
    (dict(num_progs=63), True),
    (dict(num_progs=64), False),
    (dict(quantum=1 << 20, num_quanta=1 << 20), True),          # quantum * num_quanta = 2^40
    (dict(quantum=1 << 20, num_quanta=(1 << 20) + 1), False),
])
def test_fits_req16_at_the_boundaries(fields, fits):
    base = dict(kind=A.PU_STREAM_UNIFORM_HOTSPOT, num_cores=16)
    base.update(fields)
    spec = P.StreamSpec(**base)
    p = spec.params()
    assert lib().pu_stream_fits_req16(C.byref(p)) == (0 if fits else -34)
    assert P.stream_fits_req16(spec) is fits
    if not fits:
        assert "pu_req16" in U.last_error()


def test_fits_req16_refuses_invalid_parameters():
    p = P.StreamSpec(99, 16).params()
    assert lib().pu_stream_fits_req16(C.byref(p)) == -22
    assert lib().pu_stream_fits_req16(None) == -22


@pytest.mark.parametrize("kind", KINDS)
def test_fits_req16_agrees_with_the_packer(kind):
    spec = P.StreamSpec(kind, 48, seed=kind, quantum=200, num_quanta=3, max_msg=9, num_progs=2)
    assert P.stream_fits_req16(spec)
    reqs = P.generate_stream(spec)
    assert len(reqs) > 10000
    assert U.pack_req16(reqs).shape == (len(reqs), 2)


@pytest.mark.parametrize("kind", KINDS)
def test_fits_req16_is_one_sided(kind):
    """Program 64 really occurs (core 63 of 64 cores, 64 programs): refused by both."""
    spec = P.StreamSpec(kind, 64, seed=2, quantum=100, num_quanta=1, max_msg=9, num_progs=64)
    reqs = P.generate_stream(spec)
    assert reqs["prog_id"].max() == 64
    assert not P.stream_fits_req16(spec)
    with pytest.raises(P.UncoreError, match="does not fit"):
        U.pack_req16(reqs)


def test_mirror_declares_every_dstream_entry():
    L = lib()
    PP = C.POINTER(A.StreamParams)
    want = {
        "pu_stream_fits_req16": (C.c_int, [PP]),
        "pu_dstream_open": (C.c_void_p, [PP, C.c_int, C.c_int]),
        "pu_dstream_close": (None, [C.c_void_p]),
        "pu_dstream_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
        "pu_dstream_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_dstream_state_bytes": (C.c_uint64, [C.c_void_p]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert A.PU_REQ_FMT_32 == 0 and A.PU_REQ_FMT_16 == 1
    assert P.DeviceStreamSet is U.DeviceStreamSet and P.stream_fits_req16 is U.stream_fits_req16


def test_scan_and_cut_rule_equals_the_sequential_loop(tmp_path):
    assert run_cpp_check(tmp_path, "stream_cut_check.cpp").startswith("OK 3000 rounds")
