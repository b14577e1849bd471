"""The delay summaries kept on the device (DeviceDelaySummary, pu_dsum_*;
primesim_amd/csrc/delay_sum.hip) equal an independent numpy fold
(tests/dsum_fold.py) bit for bit: any range and alignment, any run pattern of core
ids, per-core tables in LDS and in device memory, both record formats, accumulation
over calls, reset, per-set state and stream ordering; then on goldens run by the
engine, and through tools/ensemble_summary.py.

The kernel needs no engine: requests and delays are synthetic numpy arrays copied
to the device.  The kernel's marks: a wave is 64 records, a workgroup pass 256, a
trip of the loop 1,024; per-core tables are in LDS up to 1,024 cores.
"""
import json
import os
import sys

import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import config as CF
from delay_stage_util import FMTS, LENGTHS, REC, ROOT, run_golden, summary_tool
from delay_stage_util import add as _add, data as _data, idx as _idx, to_dev as _to_dev
from dsum_fold import EDGE_DELAYS, I32_MAX, I32_MIN, assert_same, fold, synth
from golden_util import Case

pytestmark = pytest.mark.gpu

LDS_CORES = 1024       # delay_sum.hip: kLdsCores


def _empty(nc):
    return fold(np.zeros(0, dtype=A.REQ_DTYPE), np.zeros(0, dtype=np.int32), num_cores=nc)


def _want(acc, reqs, delays, b, e, nc):
    """acc (or the state after open) plus records [b, e); b >= e adds nothing."""
    if b >= e:
        return acc if acc is not None else _empty(nc)
    return fold(reqs[b:e], delays[b:e], num_cores=nc, acc=acc)


def _verify(ds, wants, what, tables=True):
    got = ds.read()
    assert len(got) == len(wants)
    for r, w in enumerate(wants):
        assert_same(got[r], w[0], f"{what}: replica {r}")
        if tables:
            cnt, sm = ds.cores(r)
            np.testing.assert_array_equal(cnt, w[1], err_msg=f"{what}: replica {r} per-core count")
            np.testing.assert_array_equal(sm, w[2], err_msg=f"{what}: replica {r} per-core sum")


# ---------------------------------------------------------------- ranges
@pytest.mark.parametrize("begin", [0, 1, 3, 5])
@pytest.mark.parametrize("fmt", FMTS)
def test_one_replica_any_length_and_alignment(fmt, begin):
    """Unaligned heads and tails; wave, workgroup-pass and trip edges."""
    nc = 70
    reqs, delays = _data(1100, nc, 21)
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(1, num_cores=[nc])
    try:
        for n in sorted(LENGTHS + (1000,)):
            ds.reset()
            keep = _add(ds, dev, [begin], [begin + n], fmt)
            _verify(ds, [_want(None, reqs, delays, begin, begin + n, nc)], f"begin {begin}, {n} records")
            del keep
    finally:
        ds.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_five_replicas_with_gaps_an_empty_and_a_reversed_range(fmt):
    """Different lengths and core counts in one call; records between the ranges must not count."""
    ncs = [70, 1, 1030, 16, 2000]
    ranges = [(3, 260), (300, 1300), (1400, 1400), (2000, 1990), (2100, 5000)]
    parts = []
    for k, (nc, (b, e)) in enumerate(zip(ncs, ranges)):
        parts.append(synth(max(e - b, 0), nc, 30 + k))
    reqs, delays = synth(5100, 65536, 29)         # what lies between the ranges: other cores, other delays
    delays = delays.copy()
    delays[:] = 77777
    for (b, e), (r, d) in zip(ranges, parts):
        if e > b:
            reqs[b:e], delays[b:e] = r, d
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(5, num_cores=ncs)
    try:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        wants = [_want(None, reqs, delays, b, e, nc) for nc, (b, e) in zip(ncs, ranges)]
        _verify(ds, wants, "five replicas")
        got = ds.read()
        assert got[0]["cls"]["count"].sum() == 257 and got[4]["cls"]["count"].sum() == 2900
        assert got[2]["cls"]["count"].sum() == 0 and got[3]["cls"]["count"].sum() == 0
        assert got[2]["cls"]["min"][0] == I32_MAX and got[3]["cls"]["max"][1] == I32_MIN
        assert got[:3].shape == (3,) and ds.read(3, 2).shape == (2,)
        assert_same(ds.read(3, 2), got[3:5], "read(first, n)")
        del keep
    finally:
        ds.close()


# ---------------------------------------------------------------- the run reduction
def _patterns(nc):
    """Core id sequences, concatenated: one core for 300 records; every lane another core; runs of
    1, 2, 63, 64, 65 and 100; A B A inside one wave; one run across wave, pass and trip boundaries."""
    seq = [np.full(300, 5), np.arange(448) % min(nc, 128)]
    core = 0
    for length in (1, 2, 63, 64, 65, 100, 1, 1, 2, 100, 64, 63):
        seq.append(np.full(length, core % nc))
        core += 3
    seq.append(np.tile(np.repeat([7 % nc, 9 % nc, 7 % nc], [5, 3, 6]), 10))
    seq.append(np.full(1500, nc - 1))              # crosses 64, 256 and 1,024 wherever it starts
    seq.append(np.arange(100) % nc)
    return np.concatenate(seq)


@pytest.mark.parametrize("begin", [0, 5])
@pytest.mark.parametrize("nc", [128, 2000])        # the table in LDS; in device memory
@pytest.mark.parametrize("fmt", FMTS)
def test_core_run_patterns(fmt, nc, begin):
    cores = _patterns(nc)
    n = len(cores)
    reqs, delays = synth(n, nc, 40, cores=cores)
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(1, num_cores=[nc])
    try:
        keep = _add(ds, dev, [begin], [n], fmt)
        want = _want(None, reqs, delays, begin, n, nc)
        _verify(ds, [want], f"patterns, {nc} cores")
        assert want[1][nc - 1] >= 1500 and int(want[1].sum()) == n - begin
        del keep
    finally:
        ds.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_table_sizes_around_the_lds_limit(fmt):
    """num_cores 1, 70, the LDS limit, one past it, 1,030 and the most a pu_req16 can name, in one set."""
    ncs = [1, 70, LDS_CORES, LDS_CORES + 1, 1030, 65536]
    n = 3000
    reqs = np.zeros(n * len(ncs), dtype=A.REQ_DTYPE)
    delays = np.zeros(n * len(ncs), dtype=np.int32)
    for k, nc in enumerate(ncs):
        r, d = synth(n, nc, 50 + k)
        r["core"][-70:] = nc - 1                   # the table's last entry is used
        r["core"][:3] = 0
        reqs[k * n:(k + 1) * n], delays[k * n:(k + 1) * n] = r, d
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(len(ncs), num_cores=ncs)
    try:
        assert ds.state_bytes >= 568 * len(ncs) + 16 * sum(ncs)
        keep = _add(ds, dev, [k * n for k in range(len(ncs))], [(k + 1) * n for k in range(len(ncs))], fmt)
        wants = [_want(None, reqs, delays, k * n, (k + 1) * n, nc) for k, nc in enumerate(ncs)]
        _verify(ds, wants, "table sizes")
        assert all(w[1][-1] >= 70 for w in wants)
        del keep
    finally:
        ds.close()


@pytest.mark.parametrize("nc", [70, 1100])          # the table in LDS; in device memory
@pytest.mark.parametrize("fmt", FMTS)
def test_cores_out_of_range_touch_no_table(fmt, nc):
    """Replica 1 gets records whose core ids are out of range; its neighbours' rows, filled by an
    earlier add, and its own stay as the numpy fold says."""
    n = 900
    reqs, delays = synth(3 * n + 600, nc, 60)
    bad = reqs[3 * n:]
    if fmt == A.PU_REQ_FMT_32:
        bad["core"] = np.resize(np.array([-1, nc, I32_MAX, I32_MIN, nc + 1, 0, nc - 1, -2], dtype=np.int64), 600)
    else:
        bad["core"] = np.resize(np.array([nc, 65535, nc + 1, 0, nc - 1, 40000], dtype=np.int64), 600)
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(3, num_cores=[nc] * 3)
    try:
        keep = [_add(ds, dev, [0, n, 2 * n], [n, 2 * n, 3 * n], fmt)]
        wants = [_want(None, reqs, delays, k * n, (k + 1) * n, nc) for k in range(3)]
        _verify(ds, wants, "before")
        keep.append(_add(ds, dev, [0, 3 * n, 0], [0, 3 * n + 600, 0], fmt))
        wants[1] = _want(wants[1], reqs, delays, 3 * n, 3 * n + 600, nc)
        _verify(ds, wants, "after the out-of-range records")
        oor = ds.read()["core_out_of_range"]
        assert oor[0] == 0 and oor[2] == 0 and oor[1] == (450 if fmt == A.PU_REQ_FMT_32 else 400)
        del keep
    finally:
        ds.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_bucket_edges_in_both_classes(fmt):
    d = np.repeat(EDGE_DELAYS, 2)
    reqs, _ = synth(len(d) + 1, 16, 70)
    reqs["mem_type"] = np.arange(len(reqs)) & 1
    delays = np.concatenate([[12345], d]).astype(np.int32)
    dev = _to_dev(reqs, delays, fmt)
    ds = P.DeviceDelaySummary(1)
    try:
        keep = _add(ds, dev, [1], [len(delays)], fmt)
        want = fold(reqs[1:], delays[1:])
        _verify(ds, [want], "bucket edges", tables=False)
        s = ds.read()[0]
        for c in (0, 1):
            assert s["cls"][c]["count"] == len(EDGE_DELAYS) and s["cls"][c]["min"] == I32_MIN
            assert s["cls"][c]["max"] == I32_MAX and s["cls"][c]["hist"][0] == 3 and s["cls"][c]["hist"][31] == 2
        del keep
    finally:
        ds.close()


def test_only_pu_wr_is_a_write_on_the_device():
    reqs, delays = synth(300, 4, 71)
    reqs["mem_type"] = np.resize(np.array([A.PU_RD, A.PU_WR, A.PU_WB, 3, 255], dtype=np.uint8), 300)
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    ds = P.DeviceDelaySummary(1)
    try:
        keep = _add(ds, dev, [0], [300], A.PU_REQ_FMT_32)
        _verify(ds, [fold(reqs, delays)], "mem_type values", tables=False)
        assert ds.read()[0]["cls"][1]["count"] == 60
        del keep
    finally:
        ds.close()


# ---------------------------------------------------------------- state
@pytest.mark.parametrize("nc", [70, 1100])
@pytest.mark.parametrize("fmt", FMTS)
def test_accumulation_and_reset(fmt, nc):
    """Three adds over consecutive thirds equal one add over the whole; reset starts over."""
    reqs, delays = _data(3001, nc, 80)
    dev = _to_dev(reqs, delays, fmt)
    a = P.DeviceDelaySummary(2, num_cores=[nc, nc])
    b = P.DeviceDelaySummary(2, num_cores=[nc, nc])
    try:
        keep = []
        for lo, hi in ((1, 1001), (1001, 2001), (2001, 3001)):
            keep.append(_add(a, dev, [lo, 7], [hi, 7], fmt))
        keep.append(_add(b, dev, [1, 0], [3001, 0], fmt))
        whole = _want(None, reqs, delays, 1, 3001, nc)
        _verify(a, [whole, _empty(nc)], "three thirds")
        _verify(b, [whole, _empty(nc)], "the whole")
        a.reset()
        _verify(a, [_empty(nc), _empty(nc)], "after reset")
        keep.append(_add(a, dev, [0, 500], [0, 777], fmt))
        _verify(a, [_empty(nc), _want(None, reqs, delays, 500, 777, nc)], "an add after reset")
        del keep
    finally:
        a.close()
        b.close()


def test_two_sets_on_two_streams():
    """Per-set state: interleaved calls on two sets, each on its own torch stream; then one
    set called on the other stream, ordered after its last call by the set's event."""
    import torch
    nc, fmt = 70, A.PU_REQ_FMT_32
    reqs, delays = _data(3001, nc, 80)
    dev = _to_dev(reqs, delays, fmt)
    sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
    x = P.DeviceDelaySummary(3, num_cores=[nc] * 3)
    y = P.DeviceDelaySummary(2)
    try:
        plan, wx, wy = [], [None] * 3, [None] * 2
        for k in range(6):
            bx, ex = [k * 100, 1000 + k * 150, 2000 + k * 7], [k * 100 + 100, 1000 + k * 150 + 150, 2000 + k * 7 + 7]
            by, ey = [k * 400, 3001 - (k + 1) * 300], [k * 400 + 400, 3001 - k * 300]
            plan += [(x, bx, ex, sa), (y, by, ey, sb)]
            wx = [_want(w, reqs, delays, b, e, nc) for w, b, e in zip(wx, bx, ex)]
            wy = [fold(reqs[b:e], delays[b:e], acc=w) for w, b, e in zip(wy, by, ey)]
        for k in range(4):                         # x alternates between the two streams
            bx, ex = [2500 + k, 0, 2600], [2700, 0, 2600 + k]
            plan.append((x, bx, ex, sb if k % 2 == 0 else sa))
            wx = [_want(w, reqs, delays, b, e, nc) for w, b, e in zip(wx, bx, ex)]
        # every index tensor exists before the first call: the calls follow each other with no host wait
        idx = [(_idx(b), _idx(e)) for _, b, e, _ in plan]
        for (ds, _, _, s), (b, e) in zip(plan, idx):
            ds.add(dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr(), fmt=fmt, stream_ptr=s.cuda_stream)
        _verify(x, wx, "set x")
        _verify(y, wy, "set y", tables=False)
        del idx
    finally:
        x.close()
        y.close()


def test_a_set_without_per_core_tables():
    reqs, delays = synth(500, 16, 90)
    reqs["core"][:5] = [-1, -7, I32_MIN, I32_MAX, 70000]
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    ds = P.DeviceDelaySummary(2)
    try:
        assert len(ds) == 2 and ds.state_bytes == 2 * 568
        keep = _add(ds, dev, [0, 100], [500, 200], A.PU_REQ_FMT_32)
        _verify(ds, [fold(reqs, delays), fold(reqs[100:200], delays[100:200])], "no tables", tables=False)
        assert ds.read()[0]["core_out_of_range"] == 3          # without num_cores: the negative ids
        with pytest.raises(P.UncoreError, match="without per-core tables"):
            ds.cores(0)
        del keep
    finally:
        ds.close()
    with pytest.raises(P.UncoreError, match="closed"):
        ds.read()


def test_add_and_read_validate_their_arguments():
    reqs, delays = synth(64, 16, 91)
    d_reqs, d_del = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    idx = _idx([0, 64])
    ds = P.DeviceDelaySummary(1, num_cores=[16])
    try:
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
            ds.cores(1)
        _verify(ds, [_empty(16)], "nothing was added")
        ds.add(*good)
        _verify(ds, [fold(reqs, delays, num_cores=16)], "the good call")
    finally:
        ds.close()


# ---------------------------------------------------------------- with the engine
def _run_and_summarise(c, d_reqs, fmt, s):
    """The golden's requests (already on the device) through run_device and DeviceDelaySummary on stream s."""
    nc = len(c.completion)
    got, (cnt, sm) = run_golden(c, d_reqs, fmt, s, lambda: P.DeviceDelaySummary(1, num_cores=[nc]),
                                lambda ds: (ds.read()[0], ds.cores(0)))
    want = fold(np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays), num_cores=nc)
    assert_same(got, want[0], c.name)
    np.testing.assert_array_equal(cnt, want[1])
    np.testing.assert_array_equal(sm, want[2])
    return got


@pytest.mark.parametrize("name,fmt", [("c4_hotspot", A.PU_REQ_FMT_32), ("c4_hotspot", A.PU_REQ_FMT_16),
                                      ("c3_multiprog", A.PU_REQ_FMT_32)])
def test_goldens_generated_run_and_summarised_on_the_device(name, fmt):
    """Neither a request nor a delay of the golden is on the host before the summary is read."""
    import torch
    c = Case(name)
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
    got = _run_and_summarise(c, d_reqs, fmt, s)
    assert got["cls"]["count"].sum() == n and got["core_out_of_range"] == 0


def test_overflow_halt_golden_from_the_host_copy():
    """Real zeros (the range after the halt) and a wrapped delay: bucket 0 and the negative min."""
    import torch
    c = Case("c4_overflow_halt")
    d_reqs, _ = _to_dev(c.reqs, np.zeros(len(c.reqs), dtype=np.int32), A.PU_REQ_FMT_32)
    got = _run_and_summarise(c, d_reqs, A.PU_REQ_FMT_32, torch.cuda.Stream("cuda:0"))
    zeros = int((c.delays <= 0).sum())
    assert zeros > 1 and got["cls"]["hist"][:, 0].sum() == zeros
    assert got["cls"]["min"].min() == c.delays.min() < 0


def test_ensemble_summary_tool():
    """tools/ensemble_summary.py in a child process: C1, 4 replicas, 2 chunks of 2,000; its JSON lines
    equal summarize_delays over a StreamSet -> run_device run of the same seeds."""
    import torch
    R, n, chunks, base, nc = 4, 2000, 2, 500, 16
    lines = [json.loads(x) for x in summary_tool("--seed-base", str(base))]
    assert [x["replica"] for x in lines] == list(range(R))

    cfg = P.config_from_dict(CF.preset("C1"))
    specs = [P.StreamSpec(A.PU_STREAM_PRIVATE_STREAMING, nc, seed=base + k, num_quanta=8) for k in range(R)]
    hss = P.StreamSet(specs)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        d_off = torch.arange(R + 1, dtype=torch.int64, device="cuda:0") * n
        d_del = torch.zeros((R, n), dtype=torch.int32, device="cuda:0")
        acc = [None] * R
        for _ in range(chunks):
            h = np.ascontiguousarray(hss.next(n))
            assert h.shape == (R, n)
            d_reqs = torch.from_numpy(h.view(np.uint8).reshape(R, n, 32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr())
            um.synchronize()
            d = d_del.cpu().numpy()
            for k in range(R):
                one = P.summarize_delays(h[k], d[k], num_cores=nc)[0]
                acc[k] = one if acc[k] is None else _merge(acc[k], one)
        flags = um.error_flags(R)
    finally:
        um.close()
        hss.close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ensemble_summary import replica_line
    for k in range(R):
        assert lines[k] == json.loads(json.dumps(replica_line(k, base + k, acc[k], int(flags[k])))), f"replica {k}"
        assert lines[k]["requests"] == n * chunks and lines[k]["read"]["mean"] > 0 and lines[k]["error_flags"] == 0


def _merge(a, b):
    """Two summaries of disjoint record sets as one (what accumulation over two calls gives)."""
    out = a.copy()
    for f in ("count", "sum", "hist"):
        out["cls"][f] = a["cls"][f] + b["cls"][f]
    out["cls"]["min"] = np.minimum(a["cls"]["min"], b["cls"]["min"])
    out["cls"]["max"] = np.maximum(a["cls"]["max"], b["cls"]["max"])
    out["core_out_of_range"] = a["core_out_of_range"] + b["core_out_of_range"]
    return out
