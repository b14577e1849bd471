"""The epoch series kept on the device (DeviceDelaySeries, pu_dseries_*;
primesim_amd/csrc/delay_series.hip) equal an independent numpy statement of the rule
(tests/dseries_fold.py) bit for bit: any range and alignment, any pattern of equal cells in
a wave, both record formats, timers beyond pu_req16's 40 bits, accumulation over calls,
reset, per-set state and stream ordering; the ensemble total equals the merge of the rows
read; then on goldens run by the engine, and through tools/ensemble_summary.py --series.

The kernels need no engine: requests and delays are synthetic numpy arrays copied to the
device.  The kernels' marks: a wave is 64 records, a workgroup pass 256, a trip of the loop
1,024; every record does its own LDS atomics on its cell, so a wave's 64 records meet in
one cell, in two, or in 64; the total's first pass has at most 120 replica groups.
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
from dseries_fold import assert_same, fold, merged
from dsum_fold import I32_MAX, I32_MIN, synth
from golden_util import Case

pytestmark = pytest.mark.gpu

E64 = (64, 0, 4)      # (E, t0, shift): with synth's timer = arange an epoch is 16 records, a wave holds four


def _open(count, par=E64):
    return opened(P.DeviceDelaySeries, count, par[0], t0=par[1], shift=par[2])


def _data(n, seed):
    return data(n, 70, seed)


def _want(acc, reqs, delays, b, e, par=E64):
    """acc (or zeros) plus records [b, e); b >= e adds nothing."""
    if b >= e:
        return acc if acc is not None else np.zeros((2, par[0]), dtype=A.DSERIES_DTYPE)
    return fold(reqs[b:e], delays[b:e], *par, acc=acc)


def _verify(ds, wants, what):
    got = ds.read()
    assert got.shape == (len(wants), 2, ds.epochs) and got.dtype == A.DSERIES_DTYPE
    for r, w in enumerate(wants):
        assert_same(got[r], w, f"{what}: replica {r}")
    return got


# ---------------------------------------------------------------- ranges
@pytest.mark.parametrize("begin", [0, 1, 3, 5])
@pytest.mark.parametrize("fmt", FMTS)
def test_one_replica_any_length_and_alignment(fmt, begin):
    """Unaligned heads and tails; wave, workgroup-pass and trip edges."""
    reqs, delays = _data(1100, 21)
    dev = _to_dev(reqs, delays, fmt)
    with _open(1) as ds:
        assert ds.epochs == 64
        for n in LENGTHS:
            ds.reset()
            keep = _add(ds, dev, [begin], [begin + n], fmt)
            got = _verify(ds, [_want(None, reqs, delays, begin, begin + n)], f"begin {begin}, {n} records")
            assert got["count"].sum() == n
            del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_five_replicas_with_gaps_an_empty_and_a_reversed_range(fmt):
    """Different lengths in one call; the records between the ranges carry a delay and a timer that must not count."""
    par = (64, 0, 7)                                   # epochs of 128 records; the ranges end in epoch 39
    ranges = [(3, 260), (300, 1300), (1400, 1400), (2000, 1990), (2100, 5000)]
    reqs, delays = synth(5100, 70, 29)
    delays = delays.copy()
    between, between_epoch = 77777, 60
    assert not (delays == between).any()
    keep_mask = np.zeros(len(delays), dtype=bool)
    for b, e in ranges:
        keep_mask[b:max(b, e)] = True
    delays[~keep_mask] = between
    reqs["timer"][~keep_mask] = between_epoch * 128 + 5
    dev = _to_dev(reqs, delays, fmt)
    with _open(5, par) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        got = _verify(ds, [_want(None, reqs, delays, b, e, par) for b, e in ranges], "five replicas")
        assert got[0]["count"].sum() == 257 and got[1]["count"].sum() == 1000 and got[4]["count"].sum() == 2900
        assert not got[2].view(np.uint8).any() and not got[3].view(np.uint8).any()
        assert not got["count"][:, :, between_epoch].any() and not (got["max"] == between).any()
        assert_same(ds.read(3, 2)[1], got[4], "read(3, 2)")
        assert ds.read(1, 0).shape == (0, 2, 64)
        del keep


# ---------------------------------------------------------------- equal cells in a wave
def _pattern_delays(n):
    """0, -1, INT32_MIN and INT32_MAX among ordinary values, and a run of 100 INT32_MAX from record 64 on:
    more than a wave of them, so one wave's sum leaves 32 bits."""
    rng = np.random.default_rng(43)
    d = rng.choice(np.array([1, 5, 300, 7000, 0, -1, I32_MIN, I32_MAX], dtype=np.int64), n)
    d[64:164] = I32_MAX
    return d.astype(np.int32)


# name -> ((E, t0, shift), [(timer of record i, class of record i) per pattern, as functions of np.arange(n)])
PATTERNS = {
    "E64": ((64, 1000, 4), [
        lambda i: (np.full(len(i), 1005), np.zeros(len(i), dtype=np.int64)),          # all 64 records one (class, epoch)
        lambda i: (np.where(i & 1, 1016, 1000), np.ones(len(i), dtype=np.int64)),     # two epochs alternating
        lambda i: (np.full(len(i), 1100), i & 1),                                     # two classes in one epoch
        lambda i: (1000 + 16 * (i % 6), (i // 6) & 1),                                # 12 keys in a wave
        lambda i: (1000 + 16 * (i % 5), np.zeros(len(i), dtype=np.int64)),            # 5 keys in a wave
        lambda i: (i % 1000, i & 1),                                                  # all below t0: epoch 0
        lambda i: (1000 + 63 * 16 + 7 * i, i & 1),                                    # all in the last epoch
        lambda i: (990 + i // 3, (i // 7) & 1),                                       # across t0, ascending in runs
    ]),
    "E512_shift0": ((512, 0, 0), [
        lambda i: (i % 64, np.zeros(len(i), dtype=np.int64)),                         # 64 distinct epochs in a wave
        lambda i: (i, i & 1),                                                         # ascending, clamped at 511
        lambda i: (np.full(len(i), 511), np.ones(len(i), dtype=np.int64)),
    ]),
    "E1": ((1, 0, 0), [
        lambda i: (i, i & 1),
        lambda i: (np.full(len(i), 7), np.zeros(len(i), dtype=np.int64)),
    ]),
}


@pytest.mark.parametrize("name", list(PATTERNS))
@pytest.mark.parametrize("fmt", FMTS)
def test_equal_cell_patterns_in_a_wave(fmt, name):
    """A replica per pattern, 700 records each; every range starts 5 records in, so the patterns straddle the
    wave edges, and ends 27 records early, in the middle of a wave: dead lanes among live ones."""
    par, patterns = PATTERNS[name]
    n = 700
    i = np.arange(n)
    reqs, _ = synth(n * len(patterns), 70, 40)
    d1 = _pattern_delays(n)
    delays = np.tile(d1, len(patterns))
    for k, f in enumerate(patterns):
        t, c = f(i)
        reqs["timer"][k * n:(k + 1) * n] = t
        reqs["mem_type"][k * n:(k + 1) * n] = c
    ranges = [(k * n + 5, (k + 1) * n - 27) for k in range(len(patterns))]
    assert all((e - b) % 64 for b, e in ranges)
    dev = _to_dev(reqs, delays, fmt)
    with _open(len(ranges), par) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        got = _verify(ds, [_want(None, reqs, delays, b, e, par) for b, e in ranges], name)
        assert (got["count"].sum(axis=(1, 2)) == n - 32).all()
        assert got["sum"].max() > 1 << 32 and got["max"].max() == I32_MAX and got["nonpos"].sum() > 0
        if name == "E64":
            assert got[0]["count"][0][0] == n - 32 and got[0]["count"].sum() == n - 32          # one cell holds all
            assert got[0]["sum"][0][0] == d1[5:n - 27].astype(np.int64).sum()
            assert got[5]["count"][:, 1:].sum() == 0 and got[6]["count"][:, :63].sum() == 0       # the catch-alls
        del keep


def test_only_pu_wr_is_a_write_on_the_device():
    reqs, delays = synth(300, 4, 71)
    reqs["mem_type"] = np.resize(np.array([A.PU_RD, A.PU_WR, A.PU_WB, 3, 255], dtype=np.uint8), 300)
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(1) as ds:
        keep = _add(ds, dev, [0], [300], A.PU_REQ_FMT_32)
        got = _verify(ds, [fold(reqs, delays, *E64)], "mem_type values")
        assert got[0]["count"][1].sum() == 60
        del keep


@pytest.mark.parametrize("par", [(64, -5000, 6), (512, -(1 << 41), 33), (7, (1 << 40) - 100, 5)],
                         ids=["t0_negative", "t0_far_negative", "t0_near_2_40"])
def test_timers_beyond_40_bits_and_below_zero(par):
    """pu_req only: negative timers, timers at or beyond 2^40 and 2^62, a negative t0."""
    n = 2000
    reqs, delays = synth(n, 70, 72)
    i = np.arange(n, dtype=np.int64)
    reqs["timer"] = np.select([i % 4 == 0, i % 4 == 1, i % 4 == 2], [i - 6000, (1 << 40) - 300 + i, (1 << 62) + i], -(1 << 42) + i)
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(1, par) as ds:
        keep = _add(ds, dev, [3], [n - 1], A.PU_REQ_FMT_32)
        got = _verify(ds, [_want(None, reqs, delays, 3, n - 1, par)], "wide timers")
        assert got["count"].sum() == n - 4 and (got[0]["count"].sum(axis=0) > 0).sum() >= 2
        del keep


# ---------------------------------------------------------------- state
@pytest.mark.parametrize("fmt", FMTS)
def test_accumulation_and_reset(fmt):
    """Three adds over consecutive thirds equal one add over the whole; reset starts over."""
    par = (64, 0, 6)
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    zero = np.zeros((2, 64), dtype=A.DSERIES_DTYPE)
    with _open(2, par) as a, _open(2, par) as b:
        assert len(a) == 2 and a.state_bytes >= 2 * 2 * 64 * 32
        keep = []
        for lo, hi in ((1, 1001), (1001, 2001), (2001, 3001)):
            keep.append(_add(a, dev, [lo, 7], [hi, 7], fmt))
        keep.append(_add(b, dev, [1, 0], [3001, 0], fmt))
        whole = _want(None, reqs, delays, 1, 3001, par)
        _verify(a, [whole, zero], "three thirds")
        _verify(b, [whole, zero], "the whole")
        a.reset()
        _verify(a, [zero, zero], "after reset")
        keep.append(_add(a, dev, [0, 500], [0, 777], fmt))
        _verify(a, [zero, _want(None, reqs, delays, 500, 777, par)], "an add after reset")
        del keep
    with pytest.raises(P.UncoreError, match="closed"):
        a.read()


def test_two_sets_on_two_streams():
    """Per-set state: interleaved calls on two sets, each on its own torch stream; then one
    set called on the other stream, ordered after its last call by the set's event."""
    import torch
    fmt = A.PU_REQ_FMT_32
    px, py = (64, 0, 6), (16, 100, 8)
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
    with _open(3, px) as x, _open(2, py) as y:
        plan, wx, wy = [], [None] * 3, [None] * 2
        for k in range(6):
            bx, ex = [k * 100, 1000 + k * 150, 2000 + k * 7], [k * 100 + 100, 1000 + k * 150 + 150, 2000 + k * 7 + 7]
            by, ey = [k * 400, 3001 - (k + 1) * 300], [k * 400 + 400, 3001 - k * 300]
            plan += [(x, bx, ex, sa), (y, by, ey, sb)]
            wx = [_want(w, reqs, delays, b, e, px) for w, b, e in zip(wx, bx, ex)]
            wy = [_want(w, reqs, delays, b, e, py) for w, b, e in zip(wy, by, ey)]
        for k in range(4):                         # x alternates between the two streams
            bx, ex = [2500 + k, 0, 2600], [2700, 0, 2600 + k]
            plan.append((x, bx, ex, sb if k % 2 == 0 else sa))
            wx = [_want(w, reqs, delays, b, e, px) for w, b, e in zip(wx, bx, ex)]
        # every index tensor exists before the first call: the calls follow each other with no host wait
        idx = [(_idx(b), _idx(e)) for _, b, e, _ in plan]
        for (ds, _, _, s), (b, e) in zip(plan, idx):
            ds.add(dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr(), fmt=fmt, stream_ptr=s.cuda_stream)
        _verify(x, wx, "set x")
        _verify(y, wy, "set y")
        del idx


# ---------------------------------------------------------------- totals and readers
@pytest.mark.parametrize("fmt", FMTS)
def test_ensemble_total_over_more_than_one_replica_group(fmt):
    """130 replicas (the first pass has at most 120 groups) with 300 records each."""
    R, n = 130, 300
    par = (64, 0, 10)                                   # 39,000 timers: 39 epochs
    reqs, delays = _data(R * n, 93)
    dev = _to_dev(reqs, delays, fmt)
    with _open(R, par) as ds:
        keep = _add(ds, dev, [r * n for r in range(R)], [(r + 1) * n for r in range(R)], fmt)
        cells = ds.read()
        assert_same(merged(cells), fold(reqs, delays, *par), "the rows read vs numpy")
        assert_same(ds.total(), merged(cells), "total()")
        assert_same(ds.total(first=7, n=100), merged(cells[7:107]), "total(7, 100)")
        assert_same(ds.total(first=129, n=1), cells[129], "total(129, 1)")
        assert_same(ds.total(first=3, n=121), merged(cells[3:124]), "total(3, 121)")
        assert not ds.total(first=130, n=0).view(np.uint8).any()
        assert ds.total()["count"].sum() == R * n and (ds.total()["count"].sum(axis=0) > 0).sum() == 39
        assert_same(ds.read(), cells, "reading changes nothing")
        del keep


def test_sub_ranges_leave_the_other_outputs_untouched():
    par = (16, 0, 8)
    reqs, delays = synth(2500, 70, 92)
    ranges = [(k * 500, k * 500 + 400 + k) for k in range(5)]
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    PC = C.POINTER(A.DseriesCell)
    with _open(5, par) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], A.PU_REQ_FMT_32)
        cells = ds.read()
        assert_same(ds.read(1, 3), cells[1:4], "read(1, 3)")
        # straight through the C ABI into the middle of larger buffers
        L = U.lib()
        big = np.zeros((4, 2, 16), dtype=A.DSERIES_DTYPE)
        big.view(np.uint8)[:] = 0xAB
        assert L.pu_dseries_read(ds._handle(), 3, 2, big[1:].ctypes.data_as(PC)) == 0
        assert_same(big[1:3], cells[3:5], "pu_dseries_read(3, 2)")
        assert (big[0].view(np.uint8) == 0xAB).all() and (big[3].view(np.uint8) == 0xAB).all()
        tot = np.zeros((3, 2, 16), dtype=A.DSERIES_DTYPE)
        tot.view(np.uint8)[:] = 0xAB
        assert L.pu_dseries_read_total(ds._handle(), 1, 3, tot[1:].ctypes.data_as(PC)) == 0
        assert_same(tot[1], merged(cells[1:4]), "pu_dseries_read_total(1, 3)")
        assert (tot[0].view(np.uint8) == 0xAB).all() and (tot[2].view(np.uint8) == 0xAB).all()
        assert L.pu_dseries_read_total(ds._handle(), 5, 0, tot[1:].ctypes.data_as(PC)) == 0     # n == 0 fills zeros
        assert not tot[1].view(np.uint8).any() and (tot[2].view(np.uint8) == 0xAB).all()
        assert L.pu_dseries_epochs(ds._handle()) == 16
        assert_same(ds.read(), cells, "reading changes nothing")
        del keep


# ---------------------------------------------------------------- with the engine
def _golden_params(c, E=16):
    """(E, t0, shift) from the golden's own timer range: the span covers 8 .. 16 epochs."""
    t = np.ascontiguousarray(c.reqs)["timer"].astype(np.int64)
    t0, span = int(t.min()), int(t.max()) - int(t.min())
    return E, t0, max(span.bit_length() - 4, 0)


def _run_and_fold(c, d_reqs, fmt, s):
    """The golden's requests (already on the device) through run_device and DeviceDelaySeries on stream s."""
    par = _golden_params(c)
    got = run_golden(c, d_reqs, fmt, s, lambda: P.DeviceDelaySeries(1, par[0], t0=par[1], shift=par[2]), lambda ds: ds.read()[0])
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    assert_same(got, P.delay_series(reqs, delays, *par), f"{c.name}: device vs delay_series")
    assert_same(got, fold(reqs, delays, *par), f"{c.name}: device vs numpy")
    assert (got["count"].sum(axis=0) > 0).sum() >= 4, f"{c.name}: fewer than four epochs with records"
    return got


@pytest.mark.parametrize("fmt", FMTS)
def test_golden_generated_run_and_folded_on_the_device(fmt):
    """c4_hotspot: neither a request nor a delay of the golden is on the host before the series is read."""
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
    got = _run_and_fold(c, d_reqs, fmt, s)
    assert got["count"].sum() == n


def test_overflow_halt_golden_from_the_host_copy():
    """Real zeros (the range after the halt) and a wrapped delay: in nonpos of the epochs where the golden has them."""
    import torch
    c = Case("c4_overflow_halt")
    d_reqs, _ = _to_dev(c.reqs, np.zeros(len(c.reqs), dtype=np.int32), A.PU_REQ_FMT_32)
    got = _run_and_fold(c, d_reqs, A.PU_REQ_FMT_32, torch.cuda.Stream("cuda:0"))
    par = _golden_params(c)
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    zeros = int((delays <= 0).sum())
    assert zeros > 1 and delays.min() < 0 and got["nonpos"].sum() == zeros
    wrapped = int(np.argmin(delays))
    cls, ep = int(reqs["mem_type"][wrapped] == A.PU_WR), P.dseries_epoch_of(int(reqs["timer"][wrapped]), *par)
    assert got["nonpos"][cls][ep] >= 1 and got["sum"][cls][ep] == fold(reqs, delays, *par)["sum"][cls][ep]


def test_ensemble_summary_tool_with_series():
    """tools/ensemble_summary.py --series 8:<shift> in a child process: C1, 4 replicas, 2 chunks of 2,000; its
    "series" objects equal delay_series over a StreamSet -> run_device run of the same seeds; a run
    without --series prints no "series" key."""
    import torch
    R, n, chunks, base, nc, E = 4, 2000, 2, 500, 16, 8
    cfg = P.config_from_dict(CF.preset("C1"))
    specs = [P.StreamSpec(A.PU_STREAM_PRIVATE_STREAMING, nc, seed=base + k, num_quanta=8) for k in range(R)]
    hss = P.StreamSet(specs)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    runs = []
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
            runs.append((h.copy(), d_del.cpu().numpy().copy()))
    finally:
        um.close()
        hss.close()
    # the shift from this run's timers: the largest timer lies in epoch 4 .. 7 of 8 epochs from 0 on
    tmax = max(int(h["timer"].max()) for h, _ in runs)
    shift = max(tmax.bit_length() - 3, 0)
    cells = [None] * R
    for h, d in runs:
        for k in range(R):
            cells[k] = P.delay_series(h[k], d[k], E, 0, shift, acc=cells[k])
    cells = np.stack(cells)
    assert ((cells["count"].sum(axis=1) > 0).sum(axis=1) >= 3).all(), "fewer than three epochs with records"

    lines = [json.loads(x) for x in summary_tool("--seed-base", str(base), "--series", f"{E}:{shift}")]
    assert len(lines) == R + 1 and [x["replica"] for x in lines[:R]] == list(range(R))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ensemble_summary import series_object, series_total_line
    for k in range(R):
        for c, name in enumerate(("read", "write")):
            want = json.loads(json.dumps(series_object(cells[k][c])))
            assert lines[k][name]["series"] == want, f"replica {k}, {name}"
            assert len(want["count"]) == E and sum(want["count"]) == lines[k][name]["count"]
            assert sum(want["sum"]) == lines[k][name]["sum"]
    assert lines[R] == json.loads(json.dumps(series_total_line(R, E, shift, 0, merged(cells))))
    assert sum(lines[R]["series"]["read"]["count"]) + sum(lines[R]["series"]["write"]["count"]) == R * n * chunks

    without = summary_tool("--seed-base", str(base))
    assert len(without) == R and not any('"series"' in x for x in without)
    for x, y in zip(without, lines[:R]):
        for name in ("read", "write"):
            del y[name]["series"]
        assert x == json.dumps(y)                                # byte for byte


def test_add_and_read_validate_their_arguments():
    reqs, delays = synth(64, 16, 91)
    d_reqs, d_del = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    idx = _idx([0, 64])
    zero = np.zeros((2, 64), dtype=A.DSERIES_DTYPE)
    with _open(1) as ds:
        good = (d_reqs.data_ptr(), d_del.data_ptr(), idx.data_ptr(), idx.data_ptr() + 8)
        for k in range(4):
            bad = list(good)
            bad[k] = 0
            with pytest.raises(P.UncoreError, match=r"pu_dseries_add: bad arguments \(-22\)"):
                ds.add(*bad)
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ds.add(good[0] + 8, *good[1:])                       # d_reqs not 16-byte aligned
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ds.add(*good, fmt=2)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ds.read(0, 2)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ds.total(1, 1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.read(-1, 1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.total(0, -1)
        _verify(ds, [zero], "nothing was added")
        ds.add(*good)
        _verify(ds, [fold(reqs, delays, *E64)], "the good call")
