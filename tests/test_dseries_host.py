"""delay_series (the host twin pu_dseries_host_add) against an independent numpy statement of
the rule (tests/dseries_fold.py): both record formats, timers in order, shuffled, and for
pu_req negative and at or beyond 2^40, the epoch counts 1, 2, 7, 64 and 512, continuation
through `acc`, and a replica's cells summed over the epochs against summarize_delays."""
import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from dseries_fold import assert_same, epochs_of, fold, merged
from dsum_fold import I32_MAX, I32_MIN, synth

CASES = [(1, 0, 0), (2, 0, 0), (64, 0, 4), (512, -1000, 3), (7, 500, 10)]      # (E, t0, shift)
FMTS = [A.PU_REQ_FMT_32, A.PU_REQ_FMT_16]
N = 3000


def _timers(kind: str) -> np.ndarray:
    rng = np.random.default_rng(51)
    t = np.arange(N, dtype=np.int64)
    if kind == "shuffled":
        rng.shuffle(t)
    elif kind == "negative":
        t = t - 2000                                     # from -2000 on: below and above every t0 of CASES
    elif kind == "wide":
        t = np.where(t % 3 == 0, (1 << 40) + t, np.where(t % 3 == 1, (1 << 62) + t, t))
    return t


def _data(kind: str, fmt: int, seed: int = 50):
    reqs, delays = synth(N, 70, seed)
    reqs["timer"] = _timers(kind)
    return (U.pack_req16(reqs) if fmt == A.PU_REQ_FMT_16 else reqs), delays, reqs


@pytest.mark.parametrize("case", CASES, ids=lambda c: "E%d_t%d_s%d" % c)
@pytest.mark.parametrize("kind,fmt", [("arange", FMTS[0]), ("arange", FMTS[1]), ("shuffled", FMTS[0]), ("shuffled", FMTS[1]),
                                      ("negative", FMTS[0]), ("wide", FMTS[0])])
def test_host_fold_equals_numpy(kind, fmt, case):
    E, t0, shift = case
    packed, delays, reqs = _data(kind, fmt)
    got = P.delay_series(packed, delays, E, t0, shift, fmt=fmt)
    assert got.shape == (2, E) and got.dtype == A.DSERIES_DTYPE
    assert_same(got, fold(packed, delays, E, t0, shift, fmt=fmt), f"{kind}, fmt {fmt}, {case}")
    assert int(got["count"].sum()) == N
    # the epoch of single timers, entry by entry
    for t in (int(reqs["timer"][0]), int(reqs["timer"][N // 2]), int(reqs["timer"].max()), int(reqs["timer"].min())):
        assert P.dseries_epoch_of(t, E, t0, shift) == int(epochs_of(np.array([t]), E, t0, shift)[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_both_formats_give_the_same_cells_and_every_record_is_kept(fmt):
    packed, delays, reqs = _data("arange", fmt)
    a = P.delay_series(packed, delays, 64, 0, 4, fmt=fmt)
    b = P.delay_series(reqs, delays, 64, 0, 4)
    assert_same(a, b, "pu_req16 vs pu_req")
    # an epoch is 16 records here: the last one catches everything from 63 * 16 on
    assert (a["count"].sum(axis=0)[:63] == 16).all() and a["count"].sum(axis=0)[63] == N - 63 * 16


@pytest.mark.parametrize("case", CASES, ids=lambda c: "E%d_t%d_s%d" % c)
@pytest.mark.parametrize("fmt", FMTS)
def test_three_thirds_through_acc_equal_one_call(fmt, case):
    E, t0, shift = case
    packed, delays, _ = _data("shuffled", fmt, seed=52)
    whole = P.delay_series(packed, delays, E, t0, shift, fmt=fmt)
    acc = want = None
    for lo, hi in ((0, 1000), (1000, 2000), (2000, 3000)):
        before = None if acc is None else acc.copy()
        nxt = P.delay_series(packed[lo:hi], delays[lo:hi], E, t0, shift, fmt=fmt, acc=acc)
        if before is not None:                                  # acc is left unchanged
            assert_same(acc, before, "acc after the call")
        acc = nxt
        want = fold(packed[lo:hi], delays[lo:hi], E, t0, shift, fmt=fmt, acc=want)
        assert_same(acc, want, f"after [{lo}, {hi})")
    assert_same(acc, whole, "three thirds vs one call")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "E%d_t%d_s%d" % c)
@pytest.mark.parametrize("fmt", FMTS)
def test_cells_summed_over_epochs_equal_the_delay_summary(fmt, case):
    E, t0, shift = case
    packed, delays, _ = _data("shuffled", fmt, seed=53)
    cells = P.delay_series(packed, delays, E, t0, shift, fmt=fmt)
    s, _, _ = P.summarize_delays(packed, delays, fmt=fmt)
    for c in (0, 1):
        k = s["cls"][c]
        assert int(k["count"]) > 0
        assert int(cells["count"][c].sum()) == int(k["count"]) and int(cells["sum"][c].sum()) == int(k["sum"])
        assert int(cells["nonpos"][c].sum()) == int(k["hist"][0]) > 0
        assert int(cells["max"][c].max()) == max(int(k["max"]), 0)


def test_extreme_delays_and_an_empty_class():
    d = np.resize(np.array([I32_MIN, -1, 0, I32_MAX, 0, I32_MIN, I32_MAX, -1], dtype=np.int32), 200)
    reqs, _ = synth(200, 8, seed=54)
    reqs["mem_type"] = A.PU_RD
    got = P.delay_series(reqs, d, 4, 0, 6)
    assert_same(got, fold(reqs, d, 4, 0, 6), "extremes")
    assert not got[1].view(np.uint8).any()                                   # an empty class: all-zero bytes
    assert got["nonpos"][0].sum() == 150 and (got["max"][0] == I32_MAX).all()
    only_neg = P.delay_series(reqs[:7], np.full(7, I32_MIN, dtype=np.int32), 1)
    assert only_neg["max"][0][0] == 0 and only_neg["sum"][0][0] == 7 * I32_MIN and only_neg["nonpos"][0][0] == 7
    big = P.delay_series(reqs, np.full(200, I32_MAX, dtype=np.int32), 1)     # the sum leaves 32 bits
    assert big["sum"][0][0] == 200 * I32_MAX
    assert_same(merged(np.stack([got, got])), fold(reqs, d, 4, 0, 6, acc=got), "merge of two equals twice the records")


def test_only_pu_wr_is_a_write():
    reqs, delays = synth(10, 2, seed=55)
    reqs["mem_type"] = [A.PU_RD, A.PU_WR, A.PU_WB, 3, 255, A.PU_WR, A.PU_RD, A.PU_WB, 3, 255]
    got = P.delay_series(reqs, delays, 2, 5, 0)
    assert_same(got, fold(reqs, delays, 2, 5, 0), "mem_type values")
    assert got["count"].tolist() == [[4, 4], [2, 0]]            # timers 0 .. 5 are epoch 0; writes at 1 and 5


def test_bad_arguments_raise():
    reqs, delays = synth(4, 2, seed=56)
    for E in (0, -1, 513):
        with pytest.raises(P.UncoreError, match=r"pu_dseries_host_add.*\(-22\)"):
            P.delay_series(reqs, delays, E)
    for shift in (-1, 63):
        with pytest.raises(P.UncoreError, match=r"pu_dseries_host_add.*\(-22\)"):
            P.delay_series(reqs, delays, 4, shift=shift)
    with pytest.raises(P.UncoreError, match=r"pu_dseries_host_add.*\(-22\)"):
        P.delay_series(reqs, delays, 5, fmt=7)
    acc = P.delay_series(reqs, delays, 5)
    with pytest.raises(P.UncoreError, match="acc is not the result"):
        P.delay_series(reqs, delays, 6, acc=acc)
