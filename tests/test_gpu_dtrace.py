"""One recorded trace replayed across replicas on the device (DeviceTraceSet,
pu_dtrace_*; primesim_amd/csrc/trace_place.hip): every replica's records equal
place_trace of the same slice byte for byte, in both record formats and under any
chunking, and a placed replica is the simulation of the placed trace.

Shapes: the smallest at which each mechanism of the kernel can go wrong.  A tile is
1,024 records (four per lane of a workgroup of 256); the rows are gathered from global
memory or, with PRIMEUNCORE_TRACE_ROWS=lds, staged in LDS up to 2,560 cores (past that
they are gathered whatever is asked): the look-up tests run under both settings.
Device output lands in uint8 tensors pre-filled with 0xA5, so unwritten bytes show.
"""
import functools

import numpy as np
import pytest

import oracle as O
import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from golden_util import Case

pytestmark = pytest.mark.gpu

FILL = 0xA5
TILE = 1024
CAP_CORES = 2560          # trace_place_step.h: kStageCapBytes / 8
F32, F16 = A.PU_REQ_FMT_32, A.PU_REQ_FMT_16


@functools.lru_cache(maxsize=None)
def _trace(n, nc, seed=3):
    """A trace of n records over nc cores whose cores include 0 and the last one; made once, never changed."""
    rng = np.random.default_rng(seed + 1000 * nc + n)
    r = np.zeros(n, dtype=A.REQ_DTYPE)
    r["addr"] = rng.integers(0, 1 << 48, n, dtype=np.uint64)
    r["timer"] = np.sort(rng.integers(0, 1 << 30, n))
    r["core"] = rng.integers(0, nc, n)
    r["core"][0], r["core"][-1] = nc - 1, 0
    r["prog_id"] = rng.integers(1, 64, n)
    r["mem_type"] = rng.integers(0, 2, n)
    r["batch_start"] = rng.integers(0, 2, n)
    r.setflags(write=False)
    return r


def _rows(count, nc, kind, seed=5):
    """(placements, skews) of `count` replicas that all differ: "placement", "skew", "both" or "neither"."""
    place = P.random_placements(count, nc, seed) if kind in ("placement", "both") else None
    skew = None
    if kind in ("skew", "both"):
        skew = (np.arange(count)[:, None] * 1000 + (np.arange(nc)[None, :] * 37 + 11) % 977).astype(np.int32)
        skew[0] = 0
    return place, skew


def _wants(reqs, count, place, skew, fmt):
    """Per replica the bytes [n, rec] place_trace gives for the whole trace."""
    out = []
    for r in range(count):
        w = P.place_trace(reqs, None if place is None else place[r], None if skew is None else skew[r], fmt=fmt)
        out.append(w.view(np.uint8).reshape(len(reqs), 32 if fmt == F32 else 16))
    return out


def _drive(ts, wants, chunk, fmt=F32, gap=0, streams=(None,), extra_calls=2, start=0):
    """Calls next_into until the trace has answered 0 (the first of the extra calls) and extra_calls - 1 times
    more, each call into its own 0xA5-filled slab, call k on streams[k % len] (a torch stream; None is the
    set's own).  Then checks, per replica: d_got = min(chunk, left) on every call, the records are the
    wanted slice, every byte the call does not own still holds 0xA5, position() ends at the trace's length."""
    import torch
    dev = torch.device("cuda", 0)
    rec = 32 if fmt == F32 else 16
    count, stride, T = len(wants), chunk + gap, len(wants[0])
    ncalls = -(-(T - start) // chunk) + extra_calls
    out = torch.full((ncalls, count, stride, rec), FILL, dtype=torch.uint8, device=dev)
    got = torch.full((ncalls, count), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)             # the fills are done before any stream writes records
    for k in range(ncalls):
        s = streams[k % len(streams)]
        ts.next_into(out[k].data_ptr(), chunk, stride=stride, fmt=fmt, d_got_ptr=got[k].data_ptr(),
                     stream_ptr=s.cuda_stream if s is not None else 0)
    assert ts.position() == T               # waits for the set's outstanding calls
    o, g = out.cpu().numpy(), got.cpu().numpy()
    for i, w in enumerate(wants):
        at = start
        for k in range(ncalls):
            n = min(chunk, T - at)
            assert g[k, i] == n, f"replica {i} call {k}: d_got {g[k, i]}, expected {n}"
            np.testing.assert_array_equal(o[k, i, :n], w[at:at + n], err_msg=f"replica {i} call {k}")
            assert np.all(o[k, i, n:] == FILL), f"replica {i} call {k}: bytes past record {n} were written"
            at += n
        assert at == T and g[-1, i] == 0 and g[-2, i] == 0      # two calls past the end answered 0 and wrote nothing
    return o


def _set(reqs, nc, count, kind, **kw):
    place, skew = _rows(count, nc, kind)
    return P.DeviceTraceSet(reqs, nc, count, placements=place, skews=skew, **kw), place, skew


# ------------------------------------------------------------------ records
def test_one_record_one_core():
    reqs = _trace(1, 1)
    ts = P.DeviceTraceSet(reqs, 1, 2, placements=[[0], [0]], skews=[[0], [5]])
    try:
        assert len(ts) == 2 and ts.trace_len == 1 and ts.fits_req16()
        assert ts.state_bytes == 32 + 16 + 16
        wants = _wants(reqs, 2, np.zeros((2, 1), np.int32), np.array([[0], [5]], np.int32), F32)
        assert wants[1].view(A.REQ_DTYPE)["timer"][0] == reqs["timer"][0] + 5
        _drive(ts, wants, 1)
        ts.seek(0)
        _drive(ts, wants, 4, gap=3)
    finally:
        ts.close()


@pytest.mark.parametrize("rows_in", ["lds", "global"])
@pytest.mark.parametrize("fmt", [F32, F16])
@pytest.mark.parametrize("T", [255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_workgroup_and_tile_edges(monkeypatch, T, fmt, rows_in):
    """One call larger than the trace, stride = n_each + 3; then seek(0) replays the same bytes in chunks of a tile."""
    monkeypatch.setenv("PRIMEUNCORE_TRACE_ROWS", rows_in)
    reqs = _trace(T, 48)
    ts, place, skew = _set(reqs, 48, 3, "both")
    try:
        wants = _wants(reqs, 3, place, skew, fmt)
        a = _drive(ts, wants, T + 5, fmt=fmt, gap=3)
        ts.seek(0)
        assert ts.position() == 0
        b = _drive(ts, wants, T + 5, fmt=fmt, gap=3)
        np.testing.assert_array_equal(a, b)
        ts.seek(0)
        _drive(ts, wants, TILE, fmt=fmt, gap=3)
    finally:
        ts.close()


@pytest.mark.parametrize("T,chunk", [(257, 1), (2 * TILE + 3, 7), (2 * TILE + 3, TILE), (2 * TILE + 3, 100)])
def test_chunking(T, chunk):
    reqs = _trace(T, 70)
    ts, place, skew = _set(reqs, 70, 2, "both")
    try:
        _drive(ts, _wants(reqs, 2, place, skew, F32), chunk, gap=3)
        ts.seek(T // 2)                                   # a replay from the middle
        assert ts.position() == T // 2
        _drive(ts, _wants(reqs, 2, place, skew, F16), chunk, fmt=F16, gap=3, start=T // 2)
        with pytest.raises(P.UncoreError, match=r"outside \[0, %d\].*\(-34\)" % T):
            ts.seek(T + 1)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            ts.seek(-1)
        assert ts.position() == T
    finally:
        ts.close()


@pytest.mark.parametrize("rows_in", ["lds", "global"])
@pytest.mark.parametrize("kind", ["placement", "skew", "both", "neither"])
@pytest.mark.parametrize("nc", [48, 64, 70, 1030, CAP_CORES, CAP_CORES + 1])
def test_lookup_tables(monkeypatch, nc, kind, rows_in):
    """Cores against a wave and against the LDS cap (one core past it is the gathered path whatever is asked);
    5 replicas whose rows all differ in one set; a few hundred records whose cores include 0 and the last one."""
    monkeypatch.setenv("PRIMEUNCORE_TRACE_ROWS", rows_in)
    reqs = _trace(300, nc)
    ts, place, skew = _set(reqs, nc, 5, kind)
    try:
        rows = (place is not None) + (skew is not None)
        assert ts.state_bytes == 300 * 32 + rows * ((5 * nc * 4 + 15) & ~15)      # the trace once, not per replica
        w32 = _wants(reqs, 5, place, skew, F32)
        if kind != "neither":
            assert len({w.tobytes() for w in w32}) == 5
        _drive(ts, w32, 128, gap=3)
        ts.seek(0)
        _drive(ts, _wants(reqs, 5, place, skew, F16), 300, fmt=F16)
    finally:
        ts.close()


@pytest.mark.parametrize("fmt", [F32, F16])
def test_staged_and_gathered_rows_give_the_same_bytes(monkeypatch, fmt):
    """PRIMEUNCORE_TRACE_ROWS selects the instantiation where the rows fit LDS; unset is the shipped default."""
    reqs = _trace(TILE + 1, 70)
    ts, place, skew = _set(reqs, 70, 3, "both")
    try:
        wants = _wants(reqs, 3, place, skew, fmt)
        monkeypatch.setenv("PRIMEUNCORE_TRACE_ROWS", "global")
        a = _drive(ts, wants, 500, fmt=fmt)
        monkeypatch.setenv("PRIMEUNCORE_TRACE_ROWS", "lds")
        ts.seek(0)
        b = _drive(ts, wants, 500, fmt=fmt)
        np.testing.assert_array_equal(a, b)
        monkeypatch.delenv("PRIMEUNCORE_TRACE_ROWS")
        ts.seek(0)
        np.testing.assert_array_equal(a, _drive(ts, wants, 500, fmt=fmt))
    finally:
        ts.close()


def test_a_set_that_does_not_fit_is_refused_for_16_and_served_for_32():
    import torch
    reqs = _trace(300, 48).copy()
    reqs["prog_id"][123] = 64
    ts, place, skew = _set(reqs, 48, 2, "both")
    try:
        assert not ts.fits_req16() and "record 123 does not fit pu_req16" in U.last_error()
        buf = torch.full((2, 64, 16), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(P.UncoreError, match=r"does not fit pu_req16: record 123.*\(-34\)"):
            ts.next_into(buf.data_ptr(), 64, fmt=F16)
        torch.cuda.synchronize()
        assert bool((buf == FILL).all()) and ts.position() == 0
        _drive(ts, _wants(reqs, 2, place, skew, F32), 128)
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ts.next_into(buf.data_ptr(), 64, stride=63)
        with pytest.raises(P.UncoreError, match=r"bad arguments \(-22\)"):
            ts.next_into(buf.data_ptr() + 8, 64)
    finally:
        ts.close()
    late = _trace(300, 48).copy()
    late["timer"][-1] = (1 << 40) - 1000
    ts = P.DeviceTraceSet(late, 48, 2, skews=_rows(2, 48, "skew")[1])      # the largest skew is 1,976
    try:
        assert not ts.fits_req16() and "not below 2^40" in U.last_error()
    finally:
        ts.close()


def test_calls_alternating_between_streams_give_the_same_bytes():
    import torch
    reqs = _trace(2 * TILE + 3, 1030)
    ts, place, skew = _set(reqs, 1030, 3, "both")
    try:
        wants = _wants(reqs, 3, place, skew, F32)
        s1, s2 = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
        a = _drive(ts, wants, 300)
        ts.seek(0)
        b = _drive(ts, wants, 300, streams=(None, s1, s2, s1))
        np.testing.assert_array_equal(a, b)
    finally:
        ts.close()


def test_offsets_past_4_gib():
    """count = 2, pu_req16, stride = 2^28 + 1 records: replica 1's row starts 16 bytes past 2^32.  Only its
    100 records and 4 KB on either side are filled and read back."""
    import torch
    stride, n, pad = (1 << 28) + 1, 100, 4096
    reqs = _trace(300, 70)
    try:
        buf = torch.empty(2 * stride * 16, dtype=torch.uint8, device="cuda:0")
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
        pytest.skip(f"no {2 * stride * 16} bytes of device memory for the output: {e}")
    ts, place, skew = _set(reqs, 70, 2, "both")
    try:
        lo = stride * 16
        assert lo > 1 << 32
        windows = [buf[0:n * 16 + pad], buf[lo - pad:lo + n * 16 + pad]]
        for w in windows:
            w.fill_(FILL)
        got = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ts.seek(17)
        ts.next_into(buf.data_ptr(), n, stride=stride, fmt=F16, d_got_ptr=got.data_ptr())
        assert ts.position() == 17 + n
        wants = _wants(reqs, 2, place, skew, F16)
        assert got.cpu().tolist() == [n, n]
        w0, w1 = windows[0].cpu().numpy(), windows[1].cpu().numpy()
        np.testing.assert_array_equal(w0[:n * 16].reshape(n, 16), wants[0][17:17 + n])
        assert np.all(w0[n * 16:] == FILL)
        assert np.all(w1[:pad] == FILL) and np.all(w1[pad + n * 16:] == FILL)
        np.testing.assert_array_equal(w1[pad:pad + n * 16].reshape(n, 16), wants[1][17:17 + n])
    finally:
        ts.close()
        del buf


# ------------------------------------------------------------------ end to end
def _e2e_rows(nc):
    place = np.stack([np.arange(nc), np.arange(nc)[::-1], P.random_placements(2, nc, 21)[1], np.arange(nc)]).astype(np.int32)
    skew = np.zeros((4, nc), dtype=np.int32)
    skew[3] = np.arange(nc) % 5
    return place, skew


@functools.lru_cache(maxsize=None)
def _e2e_reference(name):
    """Per replica 1 .. 3: the host-placed trace and oracle.CpuRef's delays, completion cycles and counters for
    it; computed once per golden, never changed."""
    c = Case(name)
    cfg = P.load_config(c.xml_path)
    nc = cfg.sys.num_cores
    place, skew = _e2e_rows(nc)
    refs = {}
    for r in (1, 2, 3):
        placed = P.place_trace(np.ascontiguousarray(c.reqs), place[r], skew[r], num_cores=nc)
        ref = O.CpuRef(cfg)
        ref.set_mode(O.MODE_CLOSED if c.closed else 0)
        for prog, th in c.threads:
            ref.alloc_core(prog, th)
        d, rc = ref.run(placed)
        assert rc == 0
        d.setflags(write=False)
        refs[r] = (placed, d, ref.completion(), ref.stats().as_dict())
        ref.close()
    return c, cfg, nc, place, skew, refs


@pytest.mark.parametrize("name,fmt", [("c1_stream", F32), ("c1_closed", F32), ("c1_stream", F16)])
def test_a_placed_replica_is_the_simulation_of_the_placed_trace(name, fmt):
    """Four replicas of one handle over one golden's requests: identity, reversal, a seeded shuffle, identity
    with a skew of core % 5.  DeviceTraceSet.next_into in chunks that cut inside a message, then run_device."""
    import torch
    c, cfg, nc, place, skew, refs = _e2e_reference(name)
    assert nc == 16
    n, R, rec, chunk = len(c.reqs), 4, 32 if fmt == F32 else 16, 777
    assert any(c.reqs["batch_start"][at] == 0 for at in range(chunk, n, chunk))      # a chunk ends inside a message
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)                    # one stream orders the replay, the engine and the summary
    d_reqs = torch.full((R, n, rec), FILL, dtype=torch.uint8, device=dev)
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
    d_del = torch.full((R, n), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ts = P.DeviceTraceSet(np.ascontiguousarray(c.reqs), nc, R, placements=place, skews=skew)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    dsum = P.DeviceDelaySummary(R, num_cores=[nc] * R)
    try:
        if c.closed:
            um.set_replay_mode(U.PU_REPLAY_CLOSED)
        for prog, th in c.threads:
            um.allocCore(prog, th)
        um.set_device_req_format(fmt)
        for at in range(0, n, chunk):
            ts.next_into(d_reqs.data_ptr() + at * rec, chunk, stride=n, fmt=fmt, stream_ptr=s.cuda_stream)
        um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), s.cuda_stream)
        dsum.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt, stream_ptr=s.cuda_stream)
        s.synchronize()
        assert ts.position() == n
        delays = d_del.cpu().numpy()
        # replica 0 is the golden itself
        c.check_delays(delays[0])
        np.testing.assert_array_equal(um.completion(0), c.completion)
        assert um.report(0) == c.report
        # every other replica is the CPU restatement's run of the host-placed trace
        for r, (placed, want, completion, stats) in refs.items():
            np.testing.assert_array_equal(delays[r], want, err_msg=f"replica {r}")
            np.testing.assert_array_equal(um.completion(r), completion, err_msg=f"replica {r}")
            gs = um.stats(r).as_dict()
            assert gs.keys() == stats.keys()
            bad = {k: (gs[k], stats[k]) for k in stats if k != "requests" and gs[k] != stats[k]}
            assert not bad, f"replica {r}: counters differ (engine, CPU restatement): {bad}"
            assert gs["requests"] == n and gs["error_flags"] == stats["error_flags"]
        assert any((delays[r] != delays[0]).any() for r in (1, 2, 3))                # the rows are not a no-op
        # the later stages see the placed core ids: the reversed replica's per-core table
        placed, want = refs[1][0], refs[1][1]
        _, cnt, sm = P.summarize_delays(placed, want, num_cores=nc)
        got_cnt, got_sm = dsum.cores(1)
        np.testing.assert_array_equal(got_cnt, cnt)
        np.testing.assert_array_equal(got_sm, sm)
        np.testing.assert_array_equal(got_cnt, np.bincount(c.reqs["core"], minlength=nc)[::-1])
    finally:
        um.set_device_req_format(F32)
        dsum.close()
        ts.close()
        um.close()
