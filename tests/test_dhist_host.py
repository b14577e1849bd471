"""delay_histogram and histogram_quantiles (the host twins pu_dhist_host_add and
pu_dhist_host_quantiles) against an independent numpy statement of the rule
(tests/dhist_fold.py): every bucket edge, both classes and an empty one, both record
formats, three goldens; the fine histogram folded down equals summarize_delays'; and
a quantile's bucket is the bucket of the value np.sort gives, never read from a
histogram."""
import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from dhist_fold import EDGE_DELAYS_FINE, HI, LO, NB, buckets, coarse, fold, quantile_buckets, rank, sorted_quantile
from dsum_fold import EDGE_DELAYS, I32_MAX, I32_MIN, synth
from golden_util import Case

PPMS = [0, 1, 500000, 900000, 990000, 999000, 999999, 1000000]


def _check(reqs, delays, fmt=A.PU_REQ_FMT_32, what=""):
    """The host fold equals the numpy fold; its quantiles are the sort-based ones; folded down it is
    summarize_delays' histogram."""
    got = P.delay_histogram(reqs, delays, fmt=fmt)
    assert got.shape == (2, NB) and got.dtype == np.uint64
    np.testing.assert_array_equal(got, fold(reqs, delays, fmt=fmt), err_msg=f"{what}: histogram (host vs numpy)")
    count, bucket = P.histogram_quantiles(got, PPMS)
    assert count.shape == (2,) and bucket.shape == (2, len(PPMS))
    np.testing.assert_array_equal(count, got.sum(axis=1), err_msg=f"{what}: count")
    np.testing.assert_array_equal(bucket, quantile_buckets(reqs, delays, PPMS, fmt=fmt),
                                  err_msg=f"{what}: quantile buckets (host vs np.sort)")
    s = P.summarize_delays(reqs, delays, fmt=fmt)[0]
    np.testing.assert_array_equal(coarse(got), s["cls"]["hist"], err_msg=f"{what}: folded down to pu_dsum's buckets")
    return got, bucket


def test_the_numpy_bucket_is_the_rule_of_the_header():
    """The reference fold itself, on the values the header names."""
    d = np.array([I32_MIN, -1, 0, 1, 63, 64, 65, 66, 127, 128, 131, 132, (1 << 30) - 1, 1 << 30, I32_MAX], dtype=np.int32)
    np.testing.assert_array_equal(buckets(d), [0, 0, 0, 1, 63, 64, 64, 65, 95, 96, 96, 97, 831, 832, 863])
    assert len(LO) == 864 and LO[64] == 64 and HI[64] == 65 and LO[863] == (1 << 31) - (1 << 25)
    # from bucket 64 on a bucket is at most lo / 32 wide: <= 3.2 % relative width
    assert ((HI[64:] - LO[64:] + 1) * 32 <= LO[64:]).all()
    assert [rank(c, p) for c, p in ((0, 0), (7, 0), (4, 750000), (4, 750001), (10 ** 6 + 1, 1), (1 << 63, 10 ** 6))] == \
        [1, 1, 3, 4, 2, 1 << 63]
    assert sorted_quantile(np.array([5, 1, 9, 3]), 500000) == 3 and sorted_quantile(np.array([]), 5) is None


def test_bucket_of_and_bounds_agree_with_the_numpy_bounds():
    for k in range(NB):
        assert P.dhist_bucket_bounds(k) == (int(LO[k]), int(HI[k])), k
    got = np.array([P.dhist_bucket_of(int(d)) for d in EDGE_DELAYS_FINE])
    np.testing.assert_array_equal(got, buckets(EDGE_DELAYS_FINE))


@pytest.mark.parametrize("mem_type", [A.PU_RD, A.PU_WR])
@pytest.mark.parametrize("edges", ["fine", "coarse"])
def test_every_bucket_edge_in_one_class_and_the_other_left_empty(mem_type, edges):
    d = EDGE_DELAYS_FINE if edges == "fine" else EDGE_DELAYS
    reqs, _ = synth(len(d), 4, seed=1)
    reqs["mem_type"] = mem_type
    h, q = _check(reqs, d, what=f"{edges} edges, mem_type {mem_type}")
    assert h[mem_type].sum() == len(d) and not h[1 - mem_type].any()
    assert (q[1 - mem_type] == -1).all() and q[mem_type][0] == 0 and q[mem_type][-1] == 863
    if edges == "fine":
        # three non-positive values; a bucket per value below 64; both ends of every wider bucket
        assert h[mem_type][0] == 3 and (h[mem_type][1:64] == 1).all() and (h[mem_type][64:] == 2).all()


def test_both_classes_share_the_edges():
    reqs, _ = synth(2 * len(EDGE_DELAYS_FINE), 4, seed=2)
    reqs["mem_type"] = np.arange(len(reqs)) & 1
    h, _ = _check(reqs, np.repeat(EDGE_DELAYS_FINE, 2), what="edges in both classes")
    np.testing.assert_array_equal(h[0], h[1])


def test_only_pu_wr_is_a_write():
    reqs, delays = synth(6, 2, seed=3)
    reqs["mem_type"] = [A.PU_RD, A.PU_WR, A.PU_WB, 3, 255, A.PU_WR]
    h, _ = _check(reqs, delays, what="mem_type values")
    assert h[1].sum() == 2 and h[0].sum() == 4


@pytest.mark.parametrize("seed", [11, 12])
def test_both_formats_give_the_same_answer(seed):
    reqs, delays = synth(5000, 70, seed=seed)
    a, qa = _check(reqs, delays, what="pu_req")
    b, qb = _check(U.pack_req16(reqs), delays, fmt=A.PU_REQ_FMT_16, what="pu_req16")
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(qa, qb)
    # the edges of the delay summaries, as pu_req16
    r2, _ = synth(len(EDGE_DELAYS), 4, seed=seed)
    _check(U.pack_req16(r2), EDGE_DELAYS, fmt=A.PU_REQ_FMT_16, what="pu_req16, EDGE_DELAYS")


def test_one_record_and_all_records_in_bucket_0():
    reqs, _ = synth(1, 2, seed=4)
    reqs["mem_type"] = 1
    h, q = _check(reqs, np.array([777], dtype=np.int32), what="one record")
    assert (q[1] == buckets(np.array([777]))[0]).all() and (q[0] == -1).all()
    reqs, _ = synth(50, 2, seed=5)
    h, q = _check(reqs, np.resize(np.array([0, -1, I32_MIN], dtype=np.int32), 50), what="all in bucket 0")
    assert h[:, 0].sum() == 50 and h[:, 1:].sum() == 0 and set(q.ravel()) <= {0, -1}


def test_nothing_to_add_and_accumulation_by_addition():
    h, q = _check(np.zeros(0, dtype=A.REQ_DTYPE), np.zeros(0, dtype=np.int32), what="empty")
    assert not h.any() and (q == -1).all()
    reqs, delays = synth(3000, 16, seed=6)
    parts = [P.delay_histogram(reqs[a:b], delays[a:b]) for a, b in ((0, 1000), (1000, 1001), (1001, 3000))]
    np.testing.assert_array_equal(parts[0] + parts[1] + parts[2], P.delay_histogram(reqs, delays))


def test_histogram_quantiles_takes_any_leading_shape():
    reqs, delays = synth(2000, 16, seed=7)
    h = np.stack([P.delay_histogram(reqs[:1000], delays[:1000]), P.delay_histogram(reqs[1000:], delays[1000:])])
    count, bucket = P.histogram_quantiles(h, [500000, 990000])
    assert count.shape == (2, 2) and bucket.shape == (2, 2, 2)
    for k, sl in enumerate((slice(0, 1000), slice(1000, 2000))):
        np.testing.assert_array_equal(bucket[k], quantile_buckets(reqs[sl], delays[sl], [500000, 990000]))
    c1, b1 = P.histogram_quantiles(h[0, 0], 500000)
    assert c1.shape == () and b1.shape == (1,) and b1[0] == bucket[0, 0, 0]


def test_bad_arguments_raise():
    reqs, delays = synth(4, 2, seed=5)
    with pytest.raises(P.UncoreError, match=r"pu_dhist_host_add.*\(-22\)"):
        P.delay_histogram(reqs, delays, fmt=7)


def test_the_abi_validates_before_touching_a_device():
    """Bad arguments are answered the same with or without a GPU (tests/test_dhist_abi.py has every entry)."""
    L = U.lib()
    assert not L.pu_dhist_open(0, 0) and "no replicas" in U.last_error()
    assert L.pu_dhist_add(None, None, A.PU_REQ_FMT_32, None, None, None, None) == -22
    assert "pu_dhist_add: bad arguments" in U.last_error()
    assert L.pu_dhist_quantiles(None, 0, 0, None, 0, None) == -22 and L.pu_dhist_read_total(None, 0, 0, None) == -22


def test_open_without_a_gpu_gives_the_device_check_message():
    from abi_helpers import gpu_present
    if gpu_present():
        pytest.skip("checks the no-GPU path")
    with pytest.raises(P.UncoreError, match=r"no HIP device available \(the device histograms have no CPU fallback"):
        P.DeviceDelayHistogram(3)


@pytest.mark.parametrize("name", ["c4_hotspot", "c3_multiprog", "c4_overflow_halt"])
def test_goldens(name):
    c = Case(name)
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    h, q = _check(reqs, delays, what=name)
    assert h.sum() == len(reqs)
    # the answering bucket contains the value np.sort gives
    for cls in (0, 1):
        d = delays[(reqs["mem_type"] == A.PU_WR) == bool(cls)]
        for i, ppm in enumerate(PPMS):
            v = sorted_quantile(d, ppm)
            if v is None:
                assert q[cls][i] == -1
            else:
                lo, hi = P.dhist_bucket_bounds(int(q[cls][i]))
                assert lo <= v <= hi, (name, cls, ppm)
    if name == "c4_overflow_halt":     # a wrapped delay, and the zeros after the halt
        assert h[:, 0].sum() == int((delays <= 0).sum()) > 1
    else:
        p, _ = _check(U.pack_req16(reqs), delays, fmt=A.PU_REQ_FMT_16, what=f"{name} as pu_req16")
        np.testing.assert_array_equal(p, h)
