"""The slowest-request lists kept on the device (DeviceDelayTail, pu_dtail_*;
primesim_amd/csrc/delay_tail.hip) equal an independent numpy statement of the rule
(tests/dtail_fold.py) in every field of every entry and in every count: any range and
alignment, fewer records than a list holds, every tie and candidate pattern, both record
formats, accumulation over calls with positions carried on, reset, per-set state and
stream ordering, the ensemble total over more than one replica group; then on goldens run
by the engine, and through tools/ensemble_summary.py --tail.

The kernels need no engine: requests and delays are synthetic numpy arrays copied to the
device.  The kernels' marks: a wave is 64 records, a workgroup pass 256, a trip of the loop
1,024; a list has 1, 5 or 64 entries; the total's first pass has at most 120 replica groups.
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
from delay_stage_util import FMTS, LENGTHS, REC, ROOT, data, opened, run_golden
from delay_stage_util import add as _add, idx as _idx, summary_tool as _tool, to_dev as _to_dev
from dsum_fold import I32_MAX, synth
from dtail_fold import assert_same, fold, total
from golden_util import Case

pytestmark = pytest.mark.gpu


def _open(count, k):
    return opened(P.DeviceDelayTail, count, k)


def _data(n, seed):
    return data(n, 70, seed)


def _want(acc, reqs, delays, k, b, e):
    """acc (or empty lists) continued with records [b, e); b >= e adds nothing."""
    return fold(reqs[b:max(b, e)], delays[b:max(b, e)], k, acc=acc)


def _verify(ds, wants, what):
    """Every field of every entry, every count, and zero bytes past the counts."""
    entries, counts = ds.read()
    k = ds.k
    assert entries.shape == (len(wants), 2, k) and entries.dtype == A.DTAIL_DTYPE
    assert counts.shape == (len(wants), 2) and counts.dtype == np.uint32
    for r, w in enumerate(wants):
        assert_same((entries[r], counts[r]), w, f"{what}: replica {r} (device vs numpy)")
        for c in (0, 1):
            assert not entries[r][c][int(counts[r][c]):].view(np.uint8).any(), f"{what}: replica {r} past the count"
    return entries, counts


# ---------------------------------------------------------------- ranges
@pytest.mark.parametrize("begin,k", [(0, 5), (1, 5), (3, 5), (5, 5), (5, 1), (5, 64)])
@pytest.mark.parametrize("fmt", FMTS)
def test_one_replica_any_length_and_alignment(fmt, begin, k):
    """Unaligned heads and tails; wave, workgroup-pass and trip edges."""
    reqs, delays = _data(1100, 21)
    dev = _to_dev(reqs, delays, fmt)
    with _open(1, k) as ds:
        assert ds.k == k and len(ds) == 1
        for n in LENGTHS:
            ds.reset()
            keep = _add(ds, dev, [begin], [begin + n], fmt)
            _, counts = _verify(ds, [_want(None, reqs, delays, k, begin, begin + n)], f"begin {begin}, {n} records, k {k}")
            assert counts.sum() <= n
            del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_fewer_records_than_a_list_holds(fmt):
    """k = 64 with 10, 64 and 65 records: the counts, and the unused entries zeroed, straight through
    the C ABI into a buffer of 0xAB whose bytes outside [first, first + n) stay."""
    k = 64
    reqs, delays = _data(1100, 21)
    dev = _to_dev(reqs, delays, fmt)
    L = U.lib()
    with _open(3, k) as ds:
        keep = _add(ds, dev, [7, 100, 300], [17, 164, 365], fmt)
        wants = [_want(None, reqs, delays, k, b, e) for b, e in ((7, 17), (100, 164), (300, 365))]
        _, counts = _verify(ds, wants, "10, 64 and 65 records")
        assert list(counts.sum(axis=1)) == [10, 64, 65]                 # 65 records: both classes below 64
        ent = np.zeros((4, 2, k), dtype=A.DTAIL_DTYPE)
        ent.view(np.uint8)[:] = 0xAB
        cnt = np.full((4, 2), 0xABABABAB, dtype=np.uint32)
        rc = L.pu_dtail_read(ds._handle(), 0, 2, ent[1:].ctypes.data_as(C.POINTER(A.DtailEntry)),
                             cnt[1:].ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0
        for at, r in ((1, 0), (2, 1)):
            assert_same((ent[at], cnt[at]), wants[r], f"C ABI, replica {r}")
            for c in (0, 1):
                assert not ent[at][c][int(cnt[at][c]):].view(np.uint8).any()
        assert (ent[0].view(np.uint8) == 0xAB).all() and (ent[3].view(np.uint8) == 0xAB).all()
        assert (cnt[0] == 0xABABABAB).all() and (cnt[3] == 0xABABABAB).all()
        assert cnt[1].sum() == 10 and cnt[2].sum() == 64
        del keep


# ---------------------------------------------------------------- ties and candidates
def _plateau(k):
    """Range indices of k + 3 equal maxima, dealt in turn to the four waves of the first workgroup pass."""
    j = np.arange(k + 3)
    return (j % 4) * 64 + 3 + j // 4


def _patterns(k):
    """(delays, classes, ranges): 1,500 records per pattern, a range per pattern."""
    n = 1500
    rng = np.random.default_rng(43)
    both = np.arange(n) & 1
    reads = np.zeros(n, dtype=np.int64)
    plateau = rng.integers(1, 500, n)
    plateau[5 + _plateau(k)] = 900000                       # (the ranges start 5 records in)
    last = rng.integers(1, 500, n)
    parts = [
        (np.full(n, 321), both),                           # all equal, both classes alternating
        (np.arange(n) - 700, reads),                       # ascending: every record is a candidate
        (700 - np.arange(n), reads),                       # descending: only the first k are
        (np.tile([100, 300], n // 2), rng.integers(0, 2, n)),
        (plateau, reads),
        (last, both),                                      # (the maxima of these two are placed below)
        (last.copy(), reads),
    ]
    d = np.concatenate([p[0] for p in parts]).astype(np.int32)
    c = np.concatenate([p[1] for p in parts])
    return d, c, [(i * n, (i + 1) * n) for i in range(len(parts))]


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("fmt", FMTS)
def test_tie_and_candidate_patterns(fmt, k):
    """A replica per pattern; each range starts 5 records in and ends 27 records early, in the middle of a wave."""
    delays, cls, ranges = _patterns(k)
    reqs, _ = synth(len(delays), 70, 44)
    reqs["mem_type"] = cls
    ranges = [(b + 5, e - 27) for b, e in ranges]
    assert all((e - b) % 64 for b, e in ranges)
    # the maximum as the last record of the range, which is the last live lane of a partial wave
    # (1,468 records: the last wave instruction has 60 live lanes); in one of two classes, and in the only one
    delays[ranges[5][1] - 1] = I32_MAX
    delays[ranges[6][1] - 1] = I32_MAX - 1
    dev = _to_dev(reqs, delays, fmt)
    with _open(len(ranges), k) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        ent, cnt = _verify(ds, [_want(None, reqs, delays, k, b, e) for b, e in ranges], f"patterns, k {k}")
        n = ranges[0][1] - ranges[0][0]
        # all equal: the first k positions of each class (the range starts at an odd record: a write first)
        np.testing.assert_array_equal(ent[0][1]["position"], 2 * np.arange(k))
        np.testing.assert_array_equal(ent[0][0]["position"], 2 * np.arange(k) + 1)
        np.testing.assert_array_equal(ent[1][0]["position"], n - 1 - np.arange(k))       # ascending: the last k
        np.testing.assert_array_equal(ent[2][0]["position"], np.arange(k))               # descending: the first k
        assert (ent[3]["delay"][cnt[3] > 0][:, 0] == 300).all()
        assert (ent[4][0]["delay"] == 900000).all()                                      # position decides across the waves
        np.testing.assert_array_equal(ent[4][0]["position"], np.sort(_plateau(k))[:k])
        c5 = int(cls[ranges[5][1] - 1])
        assert ent[5][c5][0]["delay"] == I32_MAX and ent[5][c5][0]["position"] == n - 1
        assert ent[6][0][0]["delay"] == I32_MAX - 1 and ent[6][0][0]["position"] == n - 1
        del keep


@pytest.mark.parametrize("fmt", FMTS)
def test_five_replicas_with_gaps_an_empty_and_a_reversed_range(fmt):
    """Different lengths in one call; the records between the ranges carry INT32_MAX, which must be in no list."""
    k = 5
    ranges = [(3, 260), (300, 1300), (1400, 1400), (2000, 1990), (2100, 5000)]
    reqs, delays = synth(5100, 70, 29)
    delays = delays.copy()
    assert not (delays == I32_MAX).any()
    keep_mask = np.zeros(len(delays), dtype=bool)
    for b, e in ranges:
        keep_mask[b:max(b, e)] = True
    delays[~keep_mask] = I32_MAX
    dev = _to_dev(reqs, delays, fmt)
    with _open(5, k) as ds:
        keep = _add(ds, dev, [b for b, _ in ranges], [e for _, e in ranges], fmt)
        ent, cnt = _verify(ds, [_want(None, reqs, delays, k, b, e) for b, e in ranges], "five replicas")
        assert (cnt[[0, 1, 4]] == k).all() and not cnt[2].any() and not cnt[3].any()
        assert not (ent["delay"] == I32_MAX).any()
        e2, c2 = ds.read(3, 2)
        np.testing.assert_array_equal(e2, ent[3:5])
        np.testing.assert_array_equal(c2, cnt[3:5])
        assert ds.read(1, 0)[0].shape == (0, 2, k)
        del keep


def test_only_pu_wr_is_a_write_on_the_device():
    reqs, delays = synth(300, 4, 71)
    reqs["mem_type"] = np.resize(np.array([A.PU_RD, A.PU_WR, A.PU_WB, 3, 255], dtype=np.uint8), 300)
    dev = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    with _open(1, 64) as ds:
        keep = _add(ds, dev, [0], [300], A.PU_REQ_FMT_32)
        ent, cnt = _verify(ds, [fold(reqs, delays, 64)], "mem_type values")
        assert list(cnt[0]) == [64, 60] and (ent[0][1]["position"][:60] % 5 == 1).all()
        del keep


# ---------------------------------------------------------------- state
@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("fmt", FMTS)
def test_accumulation_and_reset(fmt, k):
    """Three adds over consecutive thirds equal one add over the whole, positions included; reset starts over."""
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    empty = fold(reqs[:0], delays[:0], k)
    with _open(2, k) as a, _open(2, k) as b:
        assert len(a) == 2 and a.state_bytes >= 2 * (2 * k * 32 + 16)
        keep = []
        for lo, hi in ((1, 1001), (1001, 2001), (2001, 3001)):
            keep.append(_add(a, dev, [lo, 7], [hi, 7], fmt))
        keep.append(_add(b, dev, [1, 0], [3001, 0], fmt))
        whole = _want(None, reqs, delays, k, 1, 3001)
        ea, _ = _verify(a, [whole, empty], "three thirds")
        _verify(b, [whole, empty], "the whole")
        assert ea[0]["position"].max() >= 1000                    # positions carry on from call to call
        a.reset()
        _verify(a, [empty, empty], "after reset")
        keep.append(_add(a, dev, [0, 500], [0, 777], fmt))
        er, _ = _verify(a, [empty, _want(None, reqs, delays, k, 500, 777)], "an add after reset")
        assert er[1]["position"].max() < 277                      # seen was back at 0
        keep.append(_add(a, dev, [0, 900], [0, 950], fmt))
        _verify(a, [empty, _want(_want(None, reqs, delays, k, 500, 777), reqs, delays, k, 900, 950)], "a second add after reset")
        del keep
    with pytest.raises(P.UncoreError, match="closed"):
        a.read()


@pytest.mark.parametrize("k", [1, 5, 64])
def test_equal_delays_across_calls_keep_the_earlier_call(k):
    """Full stored lists bar a later call: a delay equal to the stored k-th stays out (the stored entry is
    earlier), one above it gets in, in the wave that meets it and at the rank the order gives it."""
    fmt = A.PU_REQ_FMT_32
    reqs, _ = synth(1000, 8, 45)
    reqs["mem_type"] = np.arange(1000) & 1
    delays = np.full(1000, 77, dtype=np.int32)
    delays[[350, 351, 613, 900]] = [78, 77, 78, 76]
    dev = _to_dev(reqs, delays, fmt)
    with _open(1, k) as ds:
        keep = [_add(ds, dev, [0], [300], fmt)]
        first = _want(None, reqs, delays, k, 0, 300)
        ent, _ = _verify(ds, [first], "the first call")
        np.testing.assert_array_equal(ent[0][0]["position"], 2 * np.arange(k))
        keep.append(_add(ds, dev, [300], [1000], fmt))
        ent, _ = _verify(ds, [_want(first, reqs, delays, k, 300, 1000)], "the second call")
        assert list(ent[0][0]["position"][:1]) == [350] and list(ent[0][1]["position"][:1]) == [613]
        if k > 1:
            np.testing.assert_array_equal(ent[0][0]["position"][1:], 2 * np.arange(k - 1))      # then the first call's
        del keep


def test_two_sets_on_two_streams():
    """Per-set state: interleaved calls on two sets, each on its own torch stream; then one
    set called on the other stream, ordered after its last call by the set's event."""
    import torch
    fmt, k = A.PU_REQ_FMT_32, 5
    reqs, delays = _data(3001, 80)
    dev = _to_dev(reqs, delays, fmt)
    sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
    with _open(3, k) as x, _open(2, k) as y:
        plan, wx, wy = [], [None] * 3, [None] * 2
        for j in range(6):
            bx, ex = [j * 100, 1000 + j * 150, 2000 + j * 7], [j * 100 + 100, 1000 + j * 150 + 150, 2000 + j * 7 + 7]
            by, ey = [j * 400, 3001 - (j + 1) * 300], [j * 400 + 400, 3001 - j * 300]
            plan += [(x, bx, ex, sa), (y, by, ey, sb)]
            wx = [_want(w, reqs, delays, k, b, e) for w, b, e in zip(wx, bx, ex)]
            wy = [_want(w, reqs, delays, k, b, e) for w, b, e in zip(wy, by, ey)]
        for j in range(4):                         # x alternates between the two streams
            bx, ex = [2500 + j, 0, 2600], [2700, 0, 2600 + j]
            plan.append((x, bx, ex, sb if j % 2 == 0 else sa))
            wx = [_want(w, reqs, delays, k, b, e) for w, b, e in zip(wx, bx, ex)]
        # every index tensor exists before the first call: the calls follow each other with no host wait
        idx = [(_idx(b), _idx(e)) for _, b, e, _ in plan]
        for (ds, _, _, s), (b, e) in zip(plan, idx):
            ds.add(dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr(), fmt=fmt, stream_ptr=s.cuda_stream)
        _verify(x, wx, "set x")
        _verify(y, wy, "set y")
        del idx


# ---------------------------------------------------------------- totals
def _check_total(ds, ent, cnt, first, n, what):
    k = ds.k
    te, tr, tc = ds.total(first=first, n=n)
    we, wr, wc = total(ent[first:first + n], cnt[first:first + n], k)
    assert te.shape == (2, k) and tr.shape == (2, k) and tr.dtype == np.int32 and tc.shape == (2,)
    assert_same((te, tc), (we, wc), what)
    np.testing.assert_array_equal(tr, np.where(wr >= 0, wr + first, -1), err_msg=f"{what}: replicas")
    for c in (0, 1):
        assert not te[c][int(tc[c]):].view(np.uint8).any() and (tr[c][int(tc[c]):] == -1).all()
    return te, tr, tc


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("fmt", FMTS)
def test_ensemble_total_over_more_than_one_replica_group(fmt, k):
    """130 replicas (the first pass has at most 120 groups) with 300 records each; one delay value shared by
    three replicas at the cut, where the replica and then the position decide."""
    R, n = 130, 300
    reqs, delays = _data(R * n, 93)
    delays = delays.copy()
    reqs = reqs.copy()
    delays[delays > 5000] = 4000                     # the large values of synth out of the way
    top = 100000
    # k - 2 reads above everything, in replicas all over the range ...
    for j in range(k - 2):
        at = ((j * 37) % R) * n + 17 + j
        delays[at], reqs["mem_type"][at] = top + 1 + j, 0
    # ... then six equal ones in replicas 90, 20 and 20 again, 55 (two) and 8: the cut takes replica 8's and replica 20's first
    for r, off in ((90, 5), (20, 250), (20, 9), (55, 100), (55, 101), (8, 290)):
        delays[r * n + off], reqs["mem_type"][r * n + off] = top, 0
    dev = _to_dev(reqs, delays, fmt)
    with _open(R, k) as ds:
        keep = _add(ds, dev, [r * n for r in range(R)], [(r + 1) * n for r in range(R)], fmt)
        ent, cnt = ds.read()
        for r in (0, 8, 20, 129):
            assert_same((ent[r], cnt[r]), fold(reqs[r * n:(r + 1) * n], delays[r * n:(r + 1) * n], k), f"replica {r}")
        te, tr, tc = _check_total(ds, ent, cnt, 0, R, "total()")
        assert list(tc) == [k, k] and list(te[0]["delay"][-2:]) == [top, top] and list(tr[0][-2:]) == [8, 20]
        assert te[0]["position"][-1] == 9                           # replica 20's earlier one
        _check_total(ds, ent, cnt, 7, 100, "total(7, 100)")
        _check_total(ds, ent, cnt, 129, 1, "total(129, 1)")
        _, tr3, _ = _check_total(ds, ent, cnt, 3, 121, "total(3, 121)")
        assert tr3.max() <= 123 and tr3[tr3 >= 0].min() >= 3
        e0, r0, c0 = ds.total(first=130, n=0)
        assert not e0.view(np.uint8).any() and (r0 == -1).all() and not c0.any()
        e2, c2 = ds.read()
        np.testing.assert_array_equal(e2, ent)                      # forming the total changes nothing
        np.testing.assert_array_equal(c2, cnt)
        del keep


# ---------------------------------------------------------------- with the engine
def _run_and_list(c, d_reqs, fmt, s, k=16):
    """The golden's requests (already on the device) through run_device and DeviceDelayTail on stream s."""
    ent, cnt = run_golden(c, d_reqs, fmt, s, lambda: P.DeviceDelayTail(1, k), lambda ds: ds.read())
    reqs, delays = np.ascontiguousarray(c.reqs), np.ascontiguousarray(c.delays)
    host = reqs if fmt == A.PU_REQ_FMT_32 else U.pack_req16(reqs)
    assert_same((ent[0], cnt[0]), P.delay_tail(host, delays, k, fmt=fmt), f"{c.name}: device vs delay_tail")
    assert_same((ent[0], cnt[0]), fold(reqs, delays, k), f"{c.name}: device vs numpy")
    return ent[0], cnt[0]


@pytest.mark.parametrize("fmt", FMTS)
def test_golden_generated_run_and_listed_on_the_device(fmt):
    """c4_hotspot: neither a request nor a delay of the golden is on the host before the lists are read."""
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
    ent, cnt = _run_and_list(c, d_reqs, fmt, s)
    assert ent[0]["delay"][0] == c.delays[c.reqs["mem_type"] != A.PU_WR].max()


def test_overflow_halt_golden_from_the_host_copy():
    """A wrapped negative delay and the zeros after the halt are ordinary values: with more entries than the
    class has positive delays they are in the list, the zeros by position."""
    import torch
    c = Case("c4_overflow_halt")
    d_reqs, _ = _to_dev(c.reqs, np.zeros(len(c.reqs), dtype=np.int32), A.PU_REQ_FMT_32)
    ent, cnt = _run_and_list(c, d_reqs, A.PU_REQ_FMT_32, torch.cuda.Stream("cuda:0"), k=64)
    assert c.delays.min() < 0 and int((c.delays <= 0).sum()) > 1


# ---------------------------------------------------------------- the tool
def test_ensemble_summary_tool_with_tail():
    """tools/ensemble_summary.py --tail 8 in a child process: its "slowest" lists and its last line equal
    delay_tail over a StreamSet -> run_device run of the same seeds; without --tail the output is that of
    --tail less the "slowest" keys and the last line."""
    import torch
    R, n, chunks, base, nc, k = 4, 2000, 2, 1, 16, 8
    with_tail = _tool("--tail", str(k))
    without = _tool()
    lines = [json.loads(x) for x in with_tail]
    assert len(lines) == R + 1 and [x["replica"] for x in lines[:R]] == list(range(R))

    stripped = []
    for x in with_tail[:R]:
        obj = json.loads(x)
        for name in ("read", "write"):
            del obj[name]["slowest"]
        stripped.append(json.dumps(obj))
    assert stripped == without

    cfg = P.config_from_dict(CF.preset("C1"))
    specs = [P.StreamSpec(A.PU_STREAM_PRIVATE_STREAMING, nc, seed=base + j, num_quanta=8) for j in range(R)]
    hss = P.StreamSet(specs)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    acc = [None] * R
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
            for j in range(R):
                acc[j] = P.delay_tail(h[j], d[j], k, acc=acc[j])
    finally:
        um.close()
        hss.close()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ensemble_summary import slowest_list, tail_total_line
    for j in range(R):
        for c, name in enumerate(("read", "write")):
            want = json.loads(json.dumps(slowest_list(acc[j][0][c], acc[j][1][c])))
            assert lines[j][name]["slowest"] == want, f"replica {j}, {name}"
            assert len(want) == min(k, lines[j][name]["count"])
            assert [x["delay"] for x in want] == sorted((x["delay"] for x in want), reverse=True)
        assert lines[j]["read"]["slowest"][0]["delay"] == lines[j]["read"]["max"]
        assert set(lines[j]["read"]["slowest"][0]) == {"delay", "core", "addr", "timer", "position"}
    te, tr, tc = total(np.stack([a[0] for a in acc]), np.stack([a[1] for a in acc]), k)
    assert lines[R] == json.loads(json.dumps(tail_total_line(R, te, tr, tc)))
    assert lines[R]["replicas"] == R and "replica" in lines[R]["slowest"]["read"][0]
    assert lines[R]["slowest"]["read"][0]["delay"] == max(x["read"]["max"] for x in lines[:R])


# ---------------------------------------------------------------- arguments
def test_add_and_read_validate_their_arguments():
    k = 5
    reqs, delays = synth(64, 16, 91)
    d_reqs, d_del = _to_dev(reqs, delays, A.PU_REQ_FMT_32)
    idx = _idx([0, 64])
    empty = fold(reqs[:0], delays[:0], k)
    L = U.lib()
    with _open(1, k) as ds:
        good = (d_reqs.data_ptr(), d_del.data_ptr(), idx.data_ptr(), idx.data_ptr() + 8)
        for j in range(4):
            bad = list(good)
            bad[j] = 0
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
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.read(-1, 1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            ds.total(0, -1)
        ent = np.zeros((2, k), dtype=A.DTAIL_DTYPE)
        rep = np.zeros((2, k), dtype=np.int32)
        cnt = np.zeros(2, dtype=np.uint32)
        pe, pr, pc = ent.ctypes.data_as(C.POINTER(A.DtailEntry)), rep.ctypes.data_as(C.POINTER(C.c_int32)), \
            cnt.ctypes.data_as(C.POINTER(C.c_uint32))
        assert L.pu_dtail_read(ds._handle(), 0, 1, None, pc) == -22 and L.pu_dtail_read(ds._handle(), 0, 1, pe, None) == -22
        assert L.pu_dtail_read_total(ds._handle(), 0, 1, None, pr, pc) == -22
        assert L.pu_dtail_read_total(ds._handle(), 0, 1, pe, None, pc) == -22
        assert L.pu_dtail_read_total(ds._handle(), 0, 1, pe, pr, None) == -22
        _verify(ds, [empty], "nothing was added")
        ds.add(*good)
        _verify(ds, [fold(reqs, delays, k)], "the good call")
