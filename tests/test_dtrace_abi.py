"""The recorded-trace replay's C ABI on the host (pu_dtrace_*, pu_trace_place,
pu_placement_shuffle; include/primeuncore.h): the host twin against a NumPy
restatement of the rule in both formats, every refusal of pu_dtrace_open with its
code and the index it names, raised before a device is touched, the format-16
verdict at its boundaries, the seeded placements, the ctypes mirror, and the step
header (primesim_amd/csrc/trace_place_step.h) in tests/cpp/trace_place_check.cpp, a
stand-alone program built with the host's address and undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, gpu_present, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

PI32 = C.POINTER(C.c_int32)
NC = 70


def _trace(n=500, nc=NC, seed=3, tmax=1 << 30):
    """A trace whose cores include 0 and the last one, with tags and both types."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=A.REQ_DTYPE)
    r["addr"] = rng.integers(0, 1 << 48, n, dtype=np.uint64)
    r["timer"] = np.sort(rng.integers(0, tmax, n))
    r["core"] = rng.integers(0, nc, n)
    r["core"][0], r["core"][-1] = 0, nc - 1
    r["prog_id"] = rng.integers(1, 64, n)
    r["mem_type"] = rng.integers(0, 2, n)
    r["batch_start"] = rng.integers(0, 2, n)
    return r


def _restate(reqs, place, skew):
    """The rule, written out in NumPy."""
    out = reqs.copy()
    if place is not None:
        out["core"] = np.asarray(place)[reqs["core"]]
    if skew is not None:
        out["timer"] = reqs["timer"] + np.asarray(skew, dtype=np.int64)[reqs["core"]]
    out["_pad1"] = 0
    return out


def _restate16(r):
    b = (r["timer"].astype(np.uint64) | r["core"].astype(np.uint64) << np.uint64(40)
         | r["prog_id"].astype(np.uint64) << np.uint64(56) | r["mem_type"].astype(np.uint64) << np.uint64(62)
         | r["batch_start"].astype(np.uint64) << np.uint64(63))
    return np.stack([r["addr"], b], axis=1)


def _open(reqs, nc, count, place=None, skew=None):
    """pu_dtrace_open on raw arrays: (handle, error text)."""
    place = None if place is None else np.ascontiguousarray(place, dtype=np.int32)
    skew = None if skew is None else np.ascontiguousarray(skew, dtype=np.int32)
    h = lib().pu_dtrace_open(reqs.ctypes.data if reqs is not None else None, 0 if reqs is None else len(reqs), nc, count,
                             None if place is None else place.ctypes.data_as(PI32),
                             None if skew is None else skew.ctypes.data_as(PI32), 0)
    return h, U.last_error()


ROWS = [("neither", False, False), ("placement", True, False), ("skew", False, True), ("both", True, True)]


@pytest.mark.parametrize("name,with_place,with_skew", ROWS)
def test_host_twin_equals_the_numpy_restatement(name, with_place, with_skew):
    reqs = _trace()
    reqs["tag"] = np.arange(len(reqs)) % 7
    reqs["_pad1"] = -1                                    # rubbish in the padding: the rule clears it
    place = np.random.default_rng(1).permutation(NC).astype(np.int32) if with_place else None
    skew = (np.arange(NC) * 37 % 1000).astype(np.int32) if with_skew else None
    got = P.place_trace(reqs, place, skew, num_cores=NC)
    want = _restate(reqs, place, skew)
    assert got.dtype == A.REQ_DTYPE and got.tobytes() == want.tobytes()
    untagged = reqs.copy()
    untagged["tag"] = 0
    got16 = P.place_trace(untagged, place, skew, num_cores=NC, fmt=A.PU_REQ_FMT_16)
    want32 = _restate(untagged, place, skew)
    np.testing.assert_array_equal(got16, _restate16(want32))
    np.testing.assert_array_equal(got16, U.pack_req16(P.place_trace(untagged, place, skew, num_cores=NC)))
    with pytest.raises(P.UncoreError, match=r"request 1 does not fit pu_req16.*\(-34\)"):   # tag 1: as pu_pack_req16
        P.place_trace(reqs, place, skew, num_cores=NC, fmt=A.PU_REQ_FMT_16)


def test_identity_returns_the_input_bytes_with_tag_kept_and_padding_zero():
    reqs = _trace()
    reqs["tag"] = 0x1234
    for place, skew in ((None, None), (np.arange(NC), None), (None, np.zeros(NC, int)), (np.arange(NC), np.zeros(NC, int))):
        out = P.place_trace(reqs, place, skew, num_cores=NC)
        assert out.tobytes() == reqs.tobytes() and (out["tag"] == 0x1234).all() and (out["_pad1"] == 0).all()
    assert len(P.place_trace(reqs[:0])) == 0
    assert P.place_trace(reqs).tobytes() == reqs.tobytes()          # num_cores from the trace itself


def test_inverse_permutation_restores_the_cores():
    reqs = _trace()
    place = P.random_placements(2, NC, 11)[1]
    inv = np.empty_like(place)
    inv[place] = np.arange(NC, dtype=np.int32)
    there = P.place_trace(reqs, place)                                # num_cores from the row
    assert (there["core"] != reqs["core"]).any()
    assert P.place_trace(there, inv).tobytes() == reqs.tobytes()
    # the skew is indexed by the trace's core, not the placed one
    skew = np.arange(NC, dtype=np.int32)
    both = P.place_trace(reqs, place, skew)
    np.testing.assert_array_equal(both["timer"] - reqs["timer"], reqs["core"])


def test_host_twin_refusals():
    reqs = _trace()
    bad = reqs.copy()
    bad["core"][17] = NC
    with pytest.raises(P.UncoreError, match=r"record 17 has core 70.*\(-34\)"):
        P.place_trace(bad, num_cores=NC)
    with pytest.raises(P.UncoreError, match=r"entry 5 repeats core 4.*\(-22\)"):
        P.place_trace(reqs, [0, 1, 2, 3, 4, 4] + list(range(6, NC)))
    with pytest.raises(P.UncoreError, match=r"skew of core 3 is negative.*\(-22\)"):
        P.place_trace(reqs, None, [0, 0, 0, -1] + [0] * (NC - 4))
    far = reqs[:2].copy()
    far["timer"][1] = (1 << 63) - 1
    with pytest.raises(P.UncoreError, match=r"record 1: timer plus skew overflows int64.*\(-34\)"):
        P.place_trace(far, None, np.ones(NC, dtype=np.int32))
    assert lib().pu_trace_place(reqs.ctypes.data, 1, None, None, NC, 7, reqs.ctypes.data) == -22
    assert lib().pu_trace_place(reqs.ctypes.data, 1, None, None, 0, A.PU_REQ_FMT_32, reqs.ctypes.data) == -22
    assert lib().pu_trace_place(None, 1, None, None, NC, A.PU_REQ_FMT_32, None) == -22


# ------------------------------------------------------------------ pu_dtrace_open
def _refused(h, err, text):
    assert not h and text in err, err


def test_open_refuses_sizes_before_a_device():
    reqs = _trace()
    _refused(*_open(None, NC, 1), "no trace")
    _refused(*_open(reqs[:0], NC, 1), "no trace")
    _refused(*_open(reqs, NC, 0), "no replicas")
    _refused(*_open(reqs, NC, -3), "no replicas")
    for nc in (0, -1, 65537):
        _refused(*_open(reqs, nc, 1), f"num_cores {nc} is outside 1 .. 65536")
    with pytest.raises(P.UncoreError, match="num_cores 0 is outside"):
        P.DeviceTraceSet(reqs, 0, 1)


@pytest.mark.parametrize("where", [0, 250, 499])
def test_open_names_the_record_whose_core_is_out_of_range(where):
    for core in (NC, -1):
        reqs = _trace()
        reqs["core"][where] = core
        h, err = _open(reqs, NC, 3)
        _refused(h, err, f"record {where} has core {core}")
        with pytest.raises(P.UncoreError, match=f"record {where} has core"):
            P.DeviceTraceSet(reqs, NC, 3)


@pytest.mark.parametrize("replica", [0, 2])
def test_open_names_the_replica_and_entry_of_a_bad_placement(replica):
    reqs = _trace()
    place = P.random_placements(3, NC, 5)
    rep = place.copy()
    rep[replica, 40] = rep[replica, 9]                    # the first repeated entry is 40
    _refused(*_open(reqs, NC, 3, rep), f"placement of replica {replica} is no permutation: entry 40 repeats core {rep[replica, 9]}")
    for v in (NC, -1):
        out = place.copy()
        out[replica, 13] = v
        _refused(*_open(reqs, NC, 3, out), f"placement of replica {replica} is no permutation: entry 13 ({v}) is out of range")
    with pytest.raises(P.UncoreError, match=f"replica {replica} is no permutation: entry 40"):
        P.DeviceTraceSet(reqs, NC, 3, placements=rep)


def test_open_refuses_a_negative_skew_and_an_overflowing_timer():
    reqs = _trace()
    skew = np.zeros((2, NC), dtype=np.int32)
    skew[1, 69] = -5
    h, err = _open(reqs, NC, 2, None, skew)
    _refused(h, err, "skew of replica 1 of core 69 is negative (-5)")
    far = reqs.copy()
    far["timer"][-1] = (1 << 63) - 10
    skew[1, 69] = 10
    h, err = _open(far, NC, 2, None, skew)
    _refused(h, err, "plus skew 10 overflows int64")


def test_refusal_codes():
    """The code of each refusal, where the text does not carry it: through pu_trace_place, which shares the checks."""
    reqs = _trace()
    L = lib()
    one = np.zeros(NC, dtype=np.int32)
    out = np.zeros(len(reqs), dtype=A.REQ_DTYPE)
    assert L.pu_trace_place(reqs.ctypes.data, len(reqs), one.ctypes.data_as(PI32), None, NC, 0, out.ctypes.data) == -22
    one[:] = -1
    assert L.pu_trace_place(reqs.ctypes.data, len(reqs), None, one.ctypes.data_as(PI32), NC, 0, out.ctypes.data) == -22
    assert L.pu_trace_place(reqs.ctypes.data, len(reqs), None, None, NC - 1, 0, out.ctypes.data) == -34


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU path")
def test_open_without_a_gpu_fails_loudly():
    reqs = _trace()
    place = P.random_placements(2, NC, 5)
    h, err = _open(reqs, NC, 2, place, np.ones((2, NC), dtype=np.int32))
    _refused(h, err, "no HIP device")
    with pytest.raises(P.UncoreError, match="no HIP device"):
        P.DeviceTraceSet(reqs, NC, 2, placements=place)


def test_null_set_is_refused():
    L = lib()
    assert L.pu_dtrace_next(None, None, 0, 0, A.PU_REQ_FMT_32, None, None) == -22
    assert L.pu_dtrace_seek(None, 0) == -22
    assert L.pu_dtrace_position(None) == -22
    assert L.pu_dtrace_fits_req16(None) == -22
    assert L.pu_dtrace_state_bytes(None) == 0
    L.pu_dtrace_close(None)


# ------------------------------------------------------------------ the format-16 verdict
def _verdict16(reqs, nc, skew=None):
    """What the set would answer, read where no device is needed: the host twin refuses exactly the placed
    records pu_pack_req16 refuses; on a GPU the set's own verdict is asked too (test_gpu_dtrace.py)."""
    try:
        P.place_trace(reqs, None, skew, num_cores=nc, fmt=A.PU_REQ_FMT_16)
        return True
    except P.UncoreError as e:
        assert "does not fit pu_req16" in str(e) and "(-34)" in str(e)
        return False


@pytest.mark.parametrize("timer,skew,fits", [((1 << 40) - 1, 0, True), (1 << 40, 0, False),
                                             ((1 << 40) - 8, 7, True), ((1 << 40) - 8, 8, False)])
def test_req16_verdict_at_the_timer_boundary(timer, skew, fits):
    reqs = _trace(n=4, nc=4)
    reqs["timer"][3] = timer
    sk = np.zeros(4, dtype=np.int32)
    sk[reqs["core"][3]] = skew
    assert _verdict16(reqs, 4, sk) is fits
    if gpu_present():
        s = P.DeviceTraceSet(reqs, 4, 2, skews=np.stack([np.zeros(4, np.int32), sk]))
        try:
            assert s.fits_req16() is fits
        finally:
            s.close()


@pytest.mark.parametrize("prog,fits", [(63, True), (64, False)])
def test_req16_verdict_at_the_program_boundary(prog, fits):
    reqs = _trace(n=4, nc=4)
    reqs["prog_id"][2] = prog
    assert _verdict16(reqs, 4) is fits
    if gpu_present():
        s = P.DeviceTraceSet(reqs, 4, 1)
        try:
            assert s.fits_req16() is fits
        finally:
            s.close()


def test_req16_holds_every_core_of_the_widest_configuration():
    reqs = _trace(n=4, nc=65536)
    place = np.arange(65536, dtype=np.int32)[::-1].copy()
    out = P.place_trace(reqs, place, fmt=A.PU_REQ_FMT_16)
    assert int(out[0, 1] >> np.uint64(40)) & 0xFFFF == 65535          # core 0 placed on the last core
    assert int(out[3, 1] >> np.uint64(40)) & 0xFFFF == 0
    with pytest.raises(P.UncoreError, match="num_cores 65537 is outside"):
        P.place_trace(reqs, num_cores=65537, fmt=A.PU_REQ_FMT_16)


# ------------------------------------------------------------------ placements
def test_random_placements_are_deterministic_permutations_with_row_0_the_identity():
    a, b = P.random_placements(6, 1030, 9), P.random_placements(6, 1030, 9)
    assert a.dtype == np.int32 and a.shape == (6, 1030)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a[0], np.arange(1030))
    for r in range(6):
        np.testing.assert_array_equal(np.sort(a[r]), np.arange(1030))
    assert len({a[r].tobytes() for r in range(6)}) == 6
    assert (P.random_placements(6, 1030, 10)[1:] != a[1:]).any()
    assert P.placement_seed(9, 0) == 0 and P.placement_seed(9, 1) != 0
    # a row is pu_placement_shuffle of its stated seed
    row = np.zeros(1030, dtype=np.int32)
    assert lib().pu_placement_shuffle(row.ctypes.data_as(PI32), 1030, P.placement_seed(9, 4)) == 0
    np.testing.assert_array_equal(row, a[4])
    assert lib().pu_placement_shuffle(row.ctypes.data_as(PI32), 1030, 0) == 0
    np.testing.assert_array_equal(row, np.arange(1030))
    assert lib().pu_placement_shuffle(None, 4, 1) == -22
    assert lib().pu_placement_shuffle(row.ctypes.data_as(PI32), 0, 1) == -22


def test_placement_shuffle_is_the_stated_fisher_yates():
    def mix(z):
        m = (1 << 64) - 1
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    n, seed = 48, 0xC0FFEE
    want, s = list(range(n)), seed
    for i in range(n - 1, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        j = mix(s) % (i + 1)
        want[i], want[j] = want[j], want[i]
    row = np.zeros(n, dtype=np.int32)
    assert lib().pu_placement_shuffle(row.ctypes.data_as(PI32), n, seed) == 0
    assert row.tolist() == want


# ------------------------------------------------------------------ mirror, header, step
def test_mirror_declares_every_dtrace_entry():
    L = lib()
    want = {
        "pu_dtrace_open": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, PI32, PI32, C.c_int]),
        "pu_dtrace_close": (None, [C.c_void_p]),
        "pu_dtrace_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
        "pu_dtrace_seek": (C.c_int, [C.c_void_p, C.c_int64]),
        "pu_dtrace_position": (C.c_int64, [C.c_void_p]),
        "pu_dtrace_fits_req16": (C.c_int, [C.c_void_p]),
        "pu_dtrace_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_trace_place": (C.c_int, [C.c_void_p, C.c_size_t, PI32, PI32, C.c_int, C.c_int, C.c_void_p]),
        "pu_placement_shuffle": (C.c_int, [PI32, C.c_int, C.c_uint64]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    for name in ("DeviceTraceSet", "place_trace", "random_placements", "placement_seed"):
        assert getattr(P, name) is getattr(U, name) and name in P.__all__, name
    import inspect
    assert (list(inspect.signature(P.DeviceTraceSet.next_into).parameters)
            == list(inspect.signature(P.DeviceStreamSet.next_into).parameters))


def test_engine_source_set_is_untouched():
    """The replay is no engine source: the Makefile's JIT_SRCS names what it named."""
    with open(os.path.join(ROOT, "primesim_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "JIT_SRCS := engine.hip geometry.h ../../include/primeuncore_records.h\n" in mk
    assert "trace_place_step.h" in mk.split("HDRS")[1].split("\n\n")[0]
    assert len(lib().pu_jit_source_tag()) == 8


def test_step_header_equals_plain_statements_of_it(tmp_path):
    out = run_cpp_check(tmp_path, "trace_place_check.cpp")
    assert out.startswith("OK 388 edge records, 100000 random records, 20 counts 154727 tile records, 4000 placements")
