"""summarize_delays (the host fold, pu_dsum_host_add) against an independent numpy
fold (tests/dsum_fold.py): every bucket edge, both classes and an empty one, cores
out of range on both sides, both record formats, and three goldens."""
import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from dsum_fold import EDGE_DELAYS, I32_MAX, I32_MIN, assert_same, buckets, fold, synth
from golden_util import Case


def _check(reqs, delays, num_cores=None, fmt=A.PU_REQ_FMT_32, what=""):
    got = P.summarize_delays(reqs, delays, num_cores=num_cores, fmt=fmt)
    want = fold(reqs, delays, num_cores=num_cores, fmt=fmt)
    assert_same(got[0], want[0], what)
    if num_cores is None:
        assert got[1] is None and got[2] is None
    else:
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: per-core count")
        np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: per-core sum")
    return got


def test_the_numpy_bucket_is_the_rule_of_the_header():
    """The reference fold itself, on the values the header names."""
    d = np.array([I32_MIN, -1, 0, 1, 2, 3, 4, 7, 8, (1 << 30) - 1, 1 << 30, I32_MAX], dtype=np.int32)
    np.testing.assert_array_equal(buckets(d), [0, 0, 0, 1, 2, 2, 3, 3, 4, 30, 31, 31])
    # 3 non-positive values, then both ends of every bucket 1..31 (bucket 1 is the single value 1)
    assert len(EDGE_DELAYS) == 64 and buckets(EDGE_DELAYS).max() == 31


@pytest.mark.parametrize("mem_type", [A.PU_RD, A.PU_WR])
def test_every_bucket_edge_in_one_class_and_the_other_left_empty(mem_type):
    n = len(EDGE_DELAYS)
    reqs, _ = synth(n, 4, seed=1)
    reqs["mem_type"] = mem_type
    s, _, _ = _check(reqs, EDGE_DELAYS, what=f"edges, mem_type {mem_type}")
    full, empty = s["cls"][mem_type], s["cls"][1 - mem_type]
    assert full["count"] == n and full["min"] == I32_MIN and full["max"] == I32_MAX
    assert full["sum"] == int(EDGE_DELAYS.astype(np.int64).sum())
    assert full["hist"][0] == 3 and full["hist"][1] == 1 and full["hist"][31] == 2 and all(full["hist"][2:31] == 2)
    assert empty["count"] == 0 and empty["sum"] == 0 and empty["min"] == I32_MAX and empty["max"] == I32_MIN
    assert not empty["hist"].any()


def test_both_classes_share_the_edges():
    reqs, _ = synth(2 * len(EDGE_DELAYS), 4, seed=2)
    reqs["mem_type"] = np.arange(len(reqs)) & 1
    s, _, _ = _check(reqs, np.repeat(EDGE_DELAYS, 2), num_cores=4, what="edges in both classes")
    assert s["cls"][0]["count"] == s["cls"][1]["count"] == len(EDGE_DELAYS)
    np.testing.assert_array_equal(s["cls"][0]["hist"], s["cls"][1]["hist"])


def test_only_pu_wr_is_a_write():
    """The engine's rule: mem_type is handed on unchanged and only PU_WR takes the write path."""
    reqs, delays = synth(6, 2, seed=3)
    reqs["mem_type"] = [A.PU_RD, A.PU_WR, A.PU_WB, 3, 255, A.PU_WR]
    s, _, _ = _check(reqs, delays, what="mem_type values")
    assert s["cls"][1]["count"] == 2 and s["cls"][0]["count"] == 4


def test_cores_out_of_range_on_both_sides():
    nc = 5
    cores = np.array([0, 4, 5, -1, I32_MAX, I32_MIN, 2, 2, 6, 4], dtype=np.int64)
    reqs, delays = synth(len(cores), nc, seed=4, cores=cores)
    s, cnt, sm = _check(reqs, delays, num_cores=nc, what="cores out of range")
    assert s["core_out_of_range"] == 5
    assert s["cls"][0]["count"] + s["cls"][1]["count"] == len(cores)        # they still count in their class
    assert cnt.sum() == 5 and list(cnt) == [1, 0, 2, 0, 2]
    assert sm[2] == int(delays[6]) + int(delays[7])
    # without num_cores only the negative ids are out of range
    s, _, _ = _check(reqs, delays, what="no num_cores")
    assert s["core_out_of_range"] == 2


@pytest.mark.parametrize("nc", [1, 70, 1030, 65536])
def test_both_formats_give_the_same_answer(nc):
    reqs, delays = synth(5000, nc, seed=10 + nc)
    reqs["core"][-3:] = nc - 1
    packed = U.pack_req16(reqs)
    a = _check(reqs, delays, num_cores=nc, what=f"pu_req, {nc} cores")
    b = _check(packed, delays, num_cores=nc, fmt=A.PU_REQ_FMT_16, what=f"pu_req16, {nc} cores")
    assert_same(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    if nc < 65536:        # one past the last core: a pu_req16 can still name it
        reqs["core"][:7] = nc
        a = _check(reqs, delays, num_cores=nc)
        b = _check(U.pack_req16(reqs), delays, num_cores=nc, fmt=A.PU_REQ_FMT_16)
        assert a[0]["core_out_of_range"] == b[0]["core_out_of_range"] == 7


def test_nothing_to_add():
    s, cnt, sm = _check(np.zeros(0, dtype=A.REQ_DTYPE), np.zeros(0, dtype=np.int32), num_cores=3, what="empty")
    assert s["cls"][0]["count"] == 0 and s["cls"][0]["min"] == I32_MAX and not cnt.any() and not sm.any()


def test_bad_arguments_raise():
    reqs, delays = synth(4, 2, seed=5)
    with pytest.raises(P.UncoreError, match=r"pu_dsum_host_add.*\(-22\)"):
        P.summarize_delays(reqs, delays, fmt=7)
    with pytest.raises(P.UncoreError, match=r"pu_dsum_host_add.*\(-22\)"):
        P.summarize_delays(reqs, delays, num_cores=0)


@pytest.mark.parametrize("name", ["c4_hotspot", "c3_multiprog", "c4_overflow_halt"])
def test_goldens(name):
    c = Case(name)
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    nc = len(c.completion)
    s, cnt, sm = _check(reqs, delays, num_cores=nc, what=name)
    assert s["cls"][0]["count"] + s["cls"][1]["count"] == len(reqs) == int(cnt.sum()) + int(s["core_out_of_range"])
    assert int(sm.sum()) + int(delays[(reqs["core"] < 0) | (reqs["core"] >= nc)].astype(np.int64).sum()) == \
        int(s["cls"][0]["sum"] + s["cls"][1]["sum"])
    if name == "c4_overflow_halt":     # a wrapped delay, and the zeros after the halt
        assert min(s["cls"][0]["min"], s["cls"][1]["min"]) < 0
        assert s["cls"][0]["hist"][0] + s["cls"][1]["hist"][0] == int((delays <= 0).sum()) > 1
    else:
        p = _check(U.pack_req16(reqs), delays, num_cores=nc, fmt=A.PU_REQ_FMT_16, what=f"{name} as pu_req16")
        assert_same(p[0], s)
