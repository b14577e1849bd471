"""The log-linear delay histograms kept on the device (DeviceDelayHistogram, pu_dhist_*;
primesim_amd/csrc/delay_hist.hip) equal an independent numpy statement of the rule
(tests/dhist_fold.py) bit for bit: any range and alignment, any pattern of equal
buckets in a wave, both record formats, accumulation over calls, reset, per-set
state and stream ordering; the quantiles formed on the device equal pu_dhist_host_quantiles and the bucket of the
value np.sort gives; the fine histogram folded down equals DeviceDelaySummary's; the
ensemble total equals the sum of the histograms read; then on goldens run by the
engine, and through tools/ensemble_summary.py --quantiles.

The kernels need no engine: requests and delays are synthetic numpy arrays copied to
the device.  The kernels' marks: a wave is 64 records, a workgroup pass 256, a trip of
the loop 1,024; a lane of the quantile scan takes 14 buckets; the total's first pass
has at most 120 replica groups.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U
from delay_stage_util import FMTS, LENGTHS, REC, ROOT, data, opened, run_golden, summary_tool
from delay_stage_util import add as _add, idx as _idx, to_dev as _to_dev
from dhist_fold import EDGE_DELAYS_FINE, NB, buckets, coarse, fold, quantile_buckets, sorted_quantile
from dsum_fold import I32_MAX, I32_MIN, synth
from golden_util import Case

pytestmark = pytest.mark.gpu

PPMS = [0, 1, 500000, 900000, 990000, 999000, 999999, 1000000]


def _open(count):
    return opened(P.DeviceDelayHistogram, count)


def _data(n, seed):
    return data(n, 70, seed)


def _want(acc, reqs, delays, b, e):
    """acc (or zeros) plus records [b, e); b >= e adds nothing."""
    if b >= e:
        return acc if acc is not None else np.zeros((2, NB), dtype=np.uint64)
    return fold(reqs[b:e], delays[b:e], acc=acc)


def _verify(ds, wants, what):
    got = ds.read()
    assert got.shape == (len(wants), 2, NB) and got.dtype == np.uint64
    for r, w in enumerate(wants):
        np.testing.assert_array_equal(got[r], w, err_msg=f"{what}: replica {r} (device vs numpy)")
    return got


# ---------------------------------------------------------------- ranges
@pytest.mark.parametrize("begin", [0, 1, 3, 5])
@pytest.mark.parametrize("fmt", FMTS)
def test_one_replica_any_length_and_alignment(fmt, begin):
    """Unaligned heads and tails; wave, workgroup-pass and trip edges."""
    reqs, delays = _data(1100, 21)
    dev = _to_dev(reqs, delays, fmt)
    with _open(1) as ds:
        for n in LENGTHS:
            ds.reset()
            keep = _add(ds, dev, [begin], [begin + n], fmt)
            got = _verify(ds, [_want(None, reqs, delays, begin, begin + n)], f"begin {begin}, {n} records")
            assert got.sum() == n
            del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_five_replicas_with_gaps_an_empty_and_a_reversed_range(fmt):
    """Different lengths in one call; the records between the ranges carry a delay that must not count."""
    ranges = [(3, 260), (300, 1300), (1400, 1400), (2000, 1990), (2100, 5000)]
    reqs, delays = synth(5100, 70, 29)
    delays = delays.copy()
    between = 77777
    assert not (delays == between).any()
    keep_mask = np.zeros(len(delays), dtype=bool)
    for b, e in ranges:
        keep_mask[b:max(b, e)] = True
    delays[~keep_mask] = between
    dev = _to_dev(reqs, delays, fmt)
    with _open(5) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        got = _verify(ds, [_want(None, reqs, delays, b, e) for b, e in ranges], "five replicas")
        assert got[0].sum() == 257 and got[1].sum() == 1000 and got[4].sum() == 2900
        assert not got[2].any() and not got[3].any()
        assert not got[:, :, buckets(np.array([between]))[0]].any()
        np.testing.assert_array_equal(ds.read(3, 2), got[3:5])
        assert ds.read(1, 0).shape == (0, 2, NB)
        del keep


# ---------------------------------------------------------------- equal buckets in a wave
def _patterns():
    """(delays, classes, ranges): the patterns one after the other, a range per pattern.  All 64 records of a
    wave one value (64 LDS adds on one counter); two values alternating; five values cycling; 64
    distinct buckets; one bucket in both classes alternating; random values of few buckets."""
    rng = np.random.default_rng(41)
    parts = [
        (np.full(192, 100), np.zeros(192, dtype=np.int64)),
        (np.tile([100, 300], 96), np.ones(192, dtype=np.int64)),
        (np.tile([10, 70, 200, 900, 5000], 52), rng.integers(0, 2, 260)),
        (np.tile(np.arange(1, 65), 3), np.zeros(192, dtype=np.int64)),
        (np.full(200, 150), np.arange(200) & 1),
        (rng.choice([1, 1, 1, 64, 7000, I32_MAX, 0, -1], 1500), rng.integers(0, 2, 1500)),
    ]
    d = np.concatenate([p[0] for p in parts]).astype(np.int32)
    c = np.concatenate([p[1] for p in parts])
    at = np.cumsum([0] + [len(p[0]) for p in parts])
    return d, c, list(zip(at[:-1], at[1:]))


@pytest.mark.parametrize("begin", [0, 5])
@pytest.mark.parametrize("fmt", FMTS)
def test_equal_bucket_patterns_in_a_wave(fmt, begin):
    """A replica per pattern (each range starts `begin` records in, so with 5 the patterns straddle the wave
    edges, and ends 27 records early, in the middle of a wave: dead lanes among live ones), and one
    replica over all of them."""
    delays, cls, ranges = _patterns()
    reqs, _ = synth(len(delays), 70, 40)
    reqs["mem_type"] = cls
    ranges = [(b + begin, e - 27) for b, e in ranges] + [(begin, len(delays) - 27)]
    assert all((e - b) % 64 for b, e in ranges)
    dev = _to_dev(reqs, delays, fmt)
    with _open(len(ranges)) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        got = _verify(ds, [_want(None, reqs, delays, b, e) for b, e in ranges], "patterns")
        assert got[0][0][buckets(np.array([100]))[0]] == 192 - begin - 27 and got[0].sum() == 192 - begin - 27
        assert (got[3][0][1:65] >= 2).all() and got[4][0].sum() + got[4][1].sum() == 200 - begin - 27
        del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_bucket_edges_in_both_classes_fold_down_to_the_delay_summary(fmt):
    """lo and hi of every bucket, INT32_MIN, -1 and 0, in both classes; the fine histogram folded down
    equals DeviceDelaySummary's hist for the same call's arguments."""
    d = np.repeat(EDGE_DELAYS_FINE, 2)
    reqs, _ = synth(len(d) + 1, 16, 70)
    reqs["mem_type"] = np.arange(len(reqs)) & 1
    delays = np.concatenate([[12345], d]).astype(np.int32)
    dev = _to_dev(reqs, delays, fmt)
    dsum = P.DeviceDelaySummary(1)
    try:
        with _open(1) as ds:
            b, e = _idx([1]), _idx([len(delays)])
            args = (dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr())
            ds.add(*args, fmt=fmt)
            dsum.add(*args, fmt=fmt)
            got = _verify(ds, [fold(reqs[1:], delays[1:])], "bucket edges")[0]
            for c in (0, 1):
                assert got[c][0] == 3 and (got[c][1:64] == 1).all() and (got[c][64:] == 2).all()
            np.testing.assert_array_equal(coarse(got), dsum.read()[0]["cls"]["hist"],
                                          err_msg="fine histogram folded down vs DeviceDelaySummary")
    finally:
        dsum.close()


def test_only_pu_wr_is_a_write_on_the_device():
    reqs, delays = synth(300, 4, 71)
    reqs["mem_type"] = np.resize(np.array([A.PU_RD, A.PU_WR, A.PU_WB, 3, 255], dtype=np.uint8), 300)
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(1) as ds:
        keep = _add(ds, dev, [0], [300], A.PU_REQ_FMT_32)
        got = _verify(ds, [fold(reqs, delays)], "mem_type values")
        assert got[0][1].sum() == 60
        del keep


# ---------------------------------------------------------------- state
@pytest.mark.parametrize("fmt", FMTS)
def test_accumulation_and_reset(fmt):
    """Three adds over consecutive thirds equal one add over the whole; reset starts over."""
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    zero = np.zeros((2, NB), dtype=np.uint64)
    with _open(2) as a, _open(2) as b:
        assert len(a) == 2 and a.state_bytes >= 2 * 2 * NB * 8
        keep = []
        for lo, hi in ((1, 1001), (1001, 2001), (2001, 3001)):
            keep.append(_add(a, dev, [lo, 7], [hi, 7], fmt))
        keep.append(_add(b, dev, [1, 0], [3001, 0], fmt))
        whole = _want(None, reqs, delays, 1, 3001)
        _verify(a, [whole, zero], "three thirds")
        _verify(b, [whole, zero], "the whole")
        a.reset()
        _verify(a, [zero, zero], "after reset")
        keep.append(_add(a, dev, [0, 500], [0, 777], fmt))
        _verify(a, [zero, _want(None, reqs, delays, 500, 777)], "an add after reset")
        del keep
    with pytest.raises(P.UncoreError, match="closed"):
        a.read()


def test_two_sets_on_two_streams():
    """Per-set state: interleaved calls on two sets, each on its own torch stream; then one
    set called on the other stream, ordered after its last call by the set's event."""
    import torch
    fmt = A.PU_REQ_FMT_32
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
    with _open(3) as x, _open(2) as y:
        plan, wx, wy = [], [None] * 3, [None] * 2
        for k in range(6):
            bx, ex = [k * 100, 1000 + k * 150, 2000 + k * 7], [k * 100 + 100, 1000 + k * 150 + 150, 2000 + k * 7 + 7]
            by, ey = [k * 400, 3001 - (k + 1) * 300], [k * 400 + 400, 3001 - k * 300]
            plan += [(x, bx, ex, sa), (y, by, ey, sb)]
            wx = [_want(w, reqs, delays, b, e) for w, b, e in zip(wx, bx, ex)]
            wy = [_want(w, reqs, delays, b, e) for w, b, e in zip(wy, by, ey)]
        for k in range(4):                         # x alternates between the two streams
            bx, ex = [2500 + k, 0, 2600], [2700, 0, 2600 + k]
            plan.append((x, bx, ex, sb if k % 2 == 0 else sa))
            wx = [_want(w, reqs, delays, b, e) for w, b, e in zip(wx, bx, ex)]
        # every index tensor exists before the first call: the calls follow each other with no host wait
        idx = [(_idx(b), _idx(e)) for _, b, e, _ in plan]
        for (ds, _, _, s), (b, e) in zip(plan, idx):
            ds.add(dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr(), fmt=fmt, stream_ptr=s.cuda_stream)
        _verify(x, wx, "set x")
        _verify(y, wy, "set y")
        del idx


# ---------------------------------------------------------------- quantiles
def _check_quantiles(ds, reqs, delays, ranges, what):
    """Device == pu_dhist_host_quantiles of the histograms read == the bucket of the sorted delays' value."""
    count, bucket = ds.quantiles(PPMS)
    hist = ds.read()
    assert count.shape == (len(ranges), 2) and bucket.shape == (len(ranges), 2, len(PPMS))
    hc, hb = P.histogram_quantiles(hist, PPMS)
    np.testing.assert_array_equal(count, hc, err_msg=f"{what}: count (device vs host)")
    np.testing.assert_array_equal(bucket, hb, err_msg=f"{what}: buckets (device vs host)")
    for r, (b, e) in enumerate(ranges):
        want = quantile_buckets(reqs[b:max(b, e)], delays[b:max(b, e)], PPMS)
        np.testing.assert_array_equal(bucket[r], want, err_msg=f"{what}: replica {r} (device vs np.sort)")
    return count, bucket


def test_quantiles_on_synthetic_data():
    reqs, delays = synth(6000, 70, 90)
    ranges = [(0, 3000), (3000, 6000), (10, 10), (100, 101), (5, 1500)]
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(len(ranges)) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], A.PU_REQ_FMT_32)
        count, bucket = _check_quantiles(ds, reqs, delays, ranges, "synthetic")
        assert count[2].sum() == 0 and (bucket[2] == -1).all()                       # an empty replica
        one = int(reqs["mem_type"][100] == A.PU_WR)                                   # one record in one class
        assert count[3][one] == 1 and count[3][1 - one] == 0 and (bucket[3][1 - one] == -1).all()
        assert (bucket[3][one] == buckets(delays[100:101])[0]).all()
        # the answering bucket contains the value np.sort gives
        d0 = delays[:3000][reqs["mem_type"][:3000] != A.PU_WR]
        for i, ppm in enumerate(PPMS):
            lo, hi = P.dhist_bucket_bounds(int(bucket[0][0][i]))
            assert lo <= sorted_quantile(d0, ppm) <= hi
        del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_quantiles_at_the_edges_of_a_lanes_buckets(fmt):
    """A lane of the scan takes buckets [14 l, 14 l + 14): answers in its first and last bucket (13, 14, 27,
    the class's last, 863), a class all in bucket 0, a class of one record, an empty class."""
    b863 = I32_MAX
    plans = [  # (delays of class 0, delays of class 1)
        ([13] * 10, [14] * 10),                          # the last bucket of lane 0, the first of lane 1
        ([27] * 5 + [1] * 2, [28] * 5 + [27] * 5),       # the last of lane 1 after a lower one; the lane boundary inside
        ([b863] * 3, [b863, 1, b863 - 1]),               # the last bucket of the last lane that has any
        ([0, -1, I32_MIN] * 4, [5]),                     # all in bucket 0; one record
        ([13, 14, 27, 28, b863, 0], []),                 # every edge once; an empty class
        ([1] * 999 + [2000], [1] * 999999 + [2000]),     # p99.9 at the step: rank 999 of 1,000; rank 999,000 of 10^6
    ]
    d, c, ranges = [], [], []
    for d0, d1 in plans:
        ranges.append((len(d), len(d) + len(d0) + len(d1)))
        d += list(d0) + list(d1)
        c += [0] * len(d0) + [1] * len(d1)
    delays = np.array(d, dtype=np.int32)
    reqs = np.zeros(len(delays), dtype=A.REQ_DTYPE)
    reqs["prog_id"] = 1
    reqs["mem_type"] = c
    dev = _to_dev(reqs, delays, fmt)
    with _open(len(ranges)) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        count, bucket = _check_quantiles(ds, reqs, delays, ranges, "lane edges")
        assert (bucket[0][0] == 13).all() and (bucket[0][1] == 14).all()
        assert bucket[1][0][0] == 1 and bucket[1][0][-1] == 27 and bucket[1][1][0] == 27 and bucket[1][1][-1] == 28
        assert (bucket[2][0] == 863).all() and bucket[2][1][0] == 1 and bucket[2][1][-1] == 863
        assert (bucket[3][0] == 0).all() and count[3][0] == 12 and (bucket[3][1] == 5).all() and count[3][1] == 1
        assert bucket[4][0][0] == 0 and bucket[4][0][-1] == 863 and (bucket[4][1] == -1).all() and count[4][1] == 0
        top = buckets(np.array([2000]))[0]
        assert list(bucket[5][0]) == [1, 1, 1, 1, 1, 1, top, top] and list(bucket[5][1]) == [1, 1, 1, 1, 1, 1, 1, top]
        del keep


def test_sub_ranges_leave_the_other_outputs_untouched():
    reqs, delays = synth(2500, 70, 92)
    ranges = [(k * 500, k * 500 + 400 + k) for k in range(5)]
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(5) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], A.PU_REQ_FMT_32)
        count, bucket = ds.quantiles(PPMS)
        hist = ds.read()
        c2, b2 = ds.quantiles(PPMS[2:5], first=1, n=3)
        np.testing.assert_array_equal(c2, count[1:4])
        np.testing.assert_array_equal(b2, bucket[1:4, :, 2:5])
        assert ds.quantiles([500000], first=5, n=0)[1].shape == (0, 2, 1)
        # straight through the C ABI into the middle of larger buffers
        L = U.lib()
        out = np.zeros((7, 2), dtype=A.DHIST_Q_DTYPE)
        out.view(np.uint8)[:] = 0xAB
        ppm = (C.c_uint32 * 2)(990000, 0)
        rc = L.pu_dhist_quantiles(ds._handle(), 2, 3, ppm, 2, out[2:].ctypes.data_as(C.POINTER(A.DhistQuantile)))
        assert rc == 0
        assert (out[:2].view(np.uint8) == 0xAB).all() and (out[5:].view(np.uint8) == 0xAB).all()
        np.testing.assert_array_equal(out[2:5]["count"], count[2:5])
        np.testing.assert_array_equal(out[2:5]["bucket"][:, :, 0], bucket[2:5, :, 4])
        np.testing.assert_array_equal(out[2:5]["bucket"][:, :, 1], bucket[2:5, :, 0])
        assert (out[2:5]["bucket"][:, :, 2:] == -1).all()                           # not asked for
        big = np.full((4, 2, NB), 0xABABABABABABABAB, dtype=np.uint64)
        assert L.pu_dhist_read(ds._handle(), 3, 2, big[1:].ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        np.testing.assert_array_equal(big[1:3], hist[3:5])
        assert (big[0] == 0xABABABABABABABAB).all() and (big[3] == 0xABABABABABABABAB).all()
        np.testing.assert_array_equal(ds.read(), hist)                              # reading changes nothing
        del keep


# ---------------------------------------------------------------- totals
@pytest.mark.parametrize("fmt", FMTS)
def test_ensemble_total_over_more_than_one_replica_group(fmt):
    """130 replicas (the first pass has at most 120 groups) with 300 records each."""
    R, n = 130, 300
    reqs, delays = _data(R * n, 93)
    dev = _to_dev(reqs, delays, fmt)
    with _open(R) as ds:
        keep = _add(ds, dev, [r * n for r in range(R)], [(r + 1) * n for r in range(R)], fmt)
        hist = ds.read()
        np.testing.assert_array_equal(hist.sum(axis=0), fold(reqs, delays), err_msg="the histograms read vs numpy")
        np.testing.assert_array_equal(ds.total(), hist.sum(axis=0), err_msg="total()")
        np.testing.assert_array_equal(ds.total(first=7, n=100), hist[7:107].sum(axis=0), err_msg="total(7, 100)")
        np.testing.assert_array_equal(ds.total(first=129, n=1), hist[129], err_msg="total(129, 1)")
        np.testing.assert_array_equal(ds.total(first=3, n=121), hist[3:124].sum(axis=0), err_msg="total(3, 121)")
        assert not ds.total(first=130, n=0).any()
        assert ds.total().sum() == R * n
        np.testing.assert_array_equal(ds.read(), hist)
        del keep


# ---------------------------------------------------------------- with the engine
def _run_and_count(c, d_reqs, fmt, s):
    """The golden's requests (already on the device) through run_device and DeviceDelayHistogram on stream s."""
    got, (_, bucket) = run_golden(c, d_reqs, fmt, s, lambda: P.DeviceDelayHistogram(1),
                                  lambda ds: (ds.read()[0], ds.quantiles([500000, 990000, 999000])))
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    np.testing.assert_array_equal(got, P.delay_histogram(reqs, delays), err_msg=f"{c.name}: device vs delay_histogram")
    np.testing.assert_array_equal(got, fold(reqs, delays), err_msg=f"{c.name}: device vs numpy")
    for cls in (0, 1):
        d = delays[(reqs["mem_type"] == A.PU_WR) == bool(cls)]
        for i, ppm in enumerate((500000, 990000, 999000)):
            v = sorted_quantile(d, ppm)
            if v is None:
                assert bucket[0][cls][i] == -1
            else:
                lo, hi = P.dhist_bucket_bounds(int(bucket[0][cls][i]))
                assert lo <= v <= hi, (c.name, cls, ppm, v, lo, hi)
    return got


@pytest.mark.parametrize("fmt", FMTS)
def test_golden_generated_run_and_counted_on_the_device(fmt):
    """c4_hotspot: neither a request nor a delay of the golden is on the host before the histogram is read."""
    import torch
    c = Case("c4_hotspot")
    n = len(c.reqs)
    s = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(s):
        d_reqs = torch.zeros((n + 4096, REC[fmt]), dtype=torch.uint8, device="cuda:0")
    dss = P.DeviceStreamSet([P.StreamSpec(**c.meta["stream"])])
    try:
        for at in range(0, n, 4096):
            dss.next_into(d_reqs[at:].data_ptr(), 4096, fmt=fmt, stream_ptr=s.cuda_stream)
        assert dss.positions()[0] == n
    finally:
        dss.close()
    got = _run_and_count(c, d_reqs, fmt, s)
    assert got.sum() == n


def test_overflow_halt_golden_from_the_host_copy():
    """Real zeros (the range after the halt) and a wrapped delay: both in bucket 0."""
    import torch
    c = Case("c4_overflow_halt")
    d_reqs, _ = _to_dev(c.reqs, np.zeros(len(c.reqs), dtype=np.int32), A.PU_REQ_FMT_32)
    got = _run_and_count(c, d_reqs, A.PU_REQ_FMT_32, torch.cuda.Stream("cuda:0"))
    zeros = int((c.delays <= 0).sum())
    assert zeros > 1 and c.delays.min() < 0 and got[:, 0].sum() == zeros


def test_ensemble_summary_tool_with_quantiles():
    """tools/ensemble_summary.py --quantiles in a child process: C1, 4 replicas, 2 chunks of 2,000; its
    quantile objects equal those of the host functions over a StreamSet -> run_device run of the same seeds."""
    import torch
    R, n, chunks, base, nc = 4, 2000, 2, 500, 16
    lines = [json.loads(x) for x in summary_tool("--seed-base", str(base), "--quantiles")]
    assert len(lines) == R + 1 and [x["replica"] for x in lines[:R]] == list(range(R))

    cfg = P.config_from_dict(CF.preset("C1"))
    specs = [P.StreamSpec(A.PU_STREAM_PRIVATE_STREAMING, nc, seed=base + k, num_quanta=8) for k in range(R)]
    hss = P.StreamSet(specs)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    hist = np.zeros((R, 2, NB), dtype=np.uint64)
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        d_off = torch.arange(R + 1, dtype=torch.int64, device="cuda:0") * n
        d_del = torch.zeros((R, n), dtype=torch.int32, device="cuda:0")
        for _ in range(chunks):
            h = np.ascontiguousarray(hss.next(n))
            d_reqs = torch.from_numpy(h.view(np.uint8).reshape(R, n, 32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr())
            um.synchronize()
            d = d_del.cpu().numpy()
            for k in range(R):
                hist[k] += P.delay_histogram(h[k], d[k])
    finally:
        um.close()
        hss.close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ensemble_summary import QUANTILE_PPM, QUANTILES, quantile_object, total_line
    assert [name for name, _ in QUANTILES] == ["p50", "p90", "p99", "p999"]
    _, bucket = P.histogram_quantiles(hist, QUANTILE_PPM)
    for k in range(R):
        for c, name in enumerate(("read", "write")):
            want = json.loads(json.dumps(quantile_object(bucket[k][c])))
            assert {q: lines[k][name][q] for q, _ in QUANTILES} == want, f"replica {k}, {name}"
            assert lines[k][name]["count"] == int(hist[k][c].sum())
        assert lines[k]["read"]["p50"]["ge"] <= lines[k]["read"]["p99"]["le"] and "p50_le" in lines[k]["read"]
    tc, tb = P.histogram_quantiles(hist.sum(axis=0), QUANTILE_PPM)
    assert lines[R] == json.loads(json.dumps(total_line(R, tc, tb)))
    assert lines[R]["quantiles"]["read"]["count"] + lines[R]["quantiles"]["write"]["count"] == R * n * chunks


def test_add_and_read_validate_their_arguments():
    reqs, delays = synth(64, 16, 91)
    d_reqs, d_del = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    idx = _idx([0, 64])
    zero = np.zeros((2, NB), dtype=np.uint64)
    with _open(1) as ds:
        good = (d_reqs.data_ptr(), d_del.data_ptr(), idx.data_ptr(), idx.data_ptr() + 8)
        for k in range(4):
            bad = list(good)
            bad[k] = 0
            with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
                ds.add(*bad)
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ds.add(good[0] + 8, *good[1:])                       # d_reqs not 16-byte aligned
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ds.add(*good, fmt=2)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ds.read(0, 2)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ds.total(1, 1)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ds.quantiles([500000], first=1, n=1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.read(-1, 1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.total(0, -1)
        with pytest.raises(P.UncoreError, match=r"between 1 and 8 quantiles \(-22\)"):
            ds.quantiles([])
        with pytest.raises(P.UncoreError, match=r"between 1 and 8 quantiles \(-22\)"):
            ds.quantiles(list(range(9)))
        with pytest.raises(P.UncoreError, match=r"above 1,000,000 ppm \(-22\)"):
            ds.quantiles([5, 1000001])
        _verify(ds, [zero], "nothing was added")
        ds.add(*good)
        _verify(ds, [fold(reqs, delays)], "the good call")
