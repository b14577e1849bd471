"""delay_tail (the host twin pu_dtail_host_add) against an independent numpy statement of
the rule (tests/dtail_fold.py): lengths around the list length, the list lengths 1, 5 and
64, both record formats, every tie pattern (all delays equal, ascending, descending), the
extreme delays as ordinary values, an empty class, the class rule, and continuation through
`acc`."""
import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from dsum_fold import I32_MAX, I32_MIN, synth
from dtail_fold import assert_same, fold

KS = [1, 5, 64]


def _check(reqs, delays, k, fmt=A.PU_REQ_FMT_32, what=""):
    got = P.delay_tail(reqs, delays, k, fmt=fmt)
    assert got[0].shape == (2, k) and got[0].dtype == A.DTAIL_DTYPE and got[1].dtype == np.uint32
    assert_same(got, fold(reqs, delays, k, fmt=fmt), what)
    for c in (0, 1):   # past the count: all-zero bytes
        assert not got[0][c][int(got[1][c]):].view(np.uint8).any(), what
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", [A.PU_REQ_FMT_32, A.PU_REQ_FMT_16])
def test_lengths_around_the_list_length(fmt, k):
    reqs, delays = synth(3000, 70, seed=31)
    packed = U.pack_req16(reqs) if fmt == A.PU_REQ_FMT_16 else reqs
    for n in sorted({0, 1, max(k - 1, 0), k, k + 1, 3000}):
        e, counts, seen = _check(packed[:n], delays[:n], k, fmt=fmt, what=f"k {k}, {n} records")
        assert seen == n and (counts <= k).all()
        if n <= k:
            assert counts.sum() == n            # every record is in a list


def test_both_formats_give_the_same_entries():
    reqs, delays = synth(3000, 70, seed=32)
    a = _check(reqs, delays, 5, what="pu_req")
    b = _check(U.pack_req16(reqs), delays, 5, fmt=A.PU_REQ_FMT_16, what="pu_req16")
    assert_same(a, b, "pu_req vs pu_req16")
    assert (a[0]["delay"][:, 0] >= a[0]["delay"][:, -1]).all()


@pytest.mark.parametrize("k", KS)
def test_all_equal_delays_keep_the_first_positions_of_each_class(k):
    reqs, _ = synth(300, 8, seed=33)
    reqs["mem_type"] = np.arange(300) & 1
    e, counts, _ = _check(reqs, np.full(300, 77, dtype=np.int32), k, what="all equal")
    assert list(counts) == [k, k]
    np.testing.assert_array_equal(e["position"][0], 2 * np.arange(k))
    np.testing.assert_array_equal(e["position"][1], 2 * np.arange(k) + 1)


@pytest.mark.parametrize("k", KS)
def test_ascending_and_descending_delays(k):
    reqs, _ = synth(500, 8, seed=34)
    reqs["mem_type"] = 0
    up = np.arange(-100, 400, dtype=np.int32)
    e, _, _ = _check(reqs, up, k, what="ascending")
    np.testing.assert_array_equal(e["position"][0], 499 - np.arange(k))      # the last k, the last first
    e, _, _ = _check(reqs, up[::-1].copy(), k, what="descending")
    np.testing.assert_array_equal(e["position"][0], np.arange(k))            # the first k


def test_extreme_delays_are_ordinary_values():
    d = np.resize(np.array([I32_MIN, -1, 0, I32_MAX, 0, I32_MIN, I32_MAX, -1], dtype=np.int32), 200)
    reqs, _ = synth(200, 8, seed=35)
    _check(reqs, d, 64, what="extremes, both classes")
    reqs["mem_type"] = A.PU_RD
    e, counts, _ = _check(reqs[:60], d[:60], 64, what="extremes, fewer than k")
    assert counts[0] == 60 and e["delay"][0][0] == I32_MAX and e["delay"][0][59] == I32_MIN
    e, _, _ = _check(reqs, d, 64, what="extremes, reads")
    assert (e["delay"][0][:50] == I32_MAX).all() and (e["delay"][0][50:] == 0).all()     # 50 maxima, then zeros
    _check(reqs[:7], np.full(7, I32_MIN, dtype=np.int32), 5, what="only INT32_MIN")
    _check(reqs[:7], np.zeros(7, dtype=np.int32), 5, what="only zeros")


@pytest.mark.parametrize("mem_type", [A.PU_RD, A.PU_WR])
def test_one_class_empty(mem_type):
    reqs, delays = synth(100, 8, seed=36)
    reqs["mem_type"] = mem_type
    e, counts, _ = _check(reqs, delays, 5, what=f"only mem_type {mem_type}")
    assert counts[mem_type] == 5 and counts[1 - mem_type] == 0 and not e[1 - mem_type].view(np.uint8).any()


def test_only_pu_wr_is_a_write():
    reqs, delays = synth(10, 2, seed=37)
    reqs["mem_type"] = [A.PU_RD, A.PU_WR, A.PU_WB, 3, 255, A.PU_WR, A.PU_RD, A.PU_WB, 3, 255]
    e, counts, _ = _check(reqs, delays, 64, what="mem_type values")
    assert list(counts) == [8, 2] and sorted(e["position"][1][:2]) == [1, 5]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", [A.PU_REQ_FMT_32, A.PU_REQ_FMT_16])
def test_three_thirds_through_acc_equal_one_call(fmt, k):
    reqs, delays = synth(3000, 70, seed=38)
    packed = U.pack_req16(reqs) if fmt == A.PU_REQ_FMT_16 else reqs
    whole = P.delay_tail(packed, delays, k, fmt=fmt)
    acc = want = None
    for lo, hi in ((0, 1000), (1000, 2000), (2000, 3000)):
        before = None if acc is None else (acc[0].copy(), acc[1].copy(), acc[2])
        nxt = P.delay_tail(packed[lo:hi], delays[lo:hi], k, fmt=fmt, acc=acc)
        if before is not None:                                  # acc is left unchanged
            assert_same(acc, before, "acc after the call")
        acc = nxt
        want = fold(packed[lo:hi], delays[lo:hi], k, fmt=fmt, acc=want)
        assert_same(acc, want, f"after [{lo}, {hi})")
    assert_same(acc, whole, "three thirds vs one call")
    assert acc[2] == 3000


def test_bad_arguments_raise():
    reqs, delays = synth(4, 2, seed=39)
    for k in (0, -1, 65):
        with pytest.raises(P.UncoreError, match=r"pu_dtail_host_add.*\(-22\)"):
            P.delay_tail(reqs, delays, k)
    with pytest.raises(P.UncoreError, match=r"pu_dtail_host_add.*\(-22\)"):
        P.delay_tail(reqs, delays, 5, fmt=7)
    acc = P.delay_tail(reqs, delays, 5)
    with pytest.raises(P.UncoreError, match="acc is not the result"):
        P.delay_tail(reqs, delays, 6, acc=acc)
