"""The end-of-run results gathered on the device (DeviceRunResults, pu_dres_*;
primesim_amd/csrc/run_results.hip) against three independent answers: the host
gather by plain copies (pu_dres_host_gather) byte for byte, the counters and
completion cycles the goldens pin to the reference, and the per-link visit and
flit counts of the traced CPU restatement (tests/link_oracle.py) edge by edge
through pu_config_queue_ends.  Then the header placements (HBM, LDS, a running
resident kernel), five replicas on a torch stream, the snapshot semantics, the
pool path and tools/ensemble_summary.py --results.

Only golden configurations and presets, so no test compiles an engine.  The
kernel's marks: a wave is 64 queues, a workgroup pass 256, a trip of the loop
1,024 (c4_hotspot: 1,984 queues, 1,024 cores)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import link_oracle as LO
import primesim_amd as P
from golden_util import Case, assert_stats_match
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
GOLDENS = ["c1_stream", "nonsquare_12", "mesh3d", "l2_shared_bus", "bus_l2_shared", "verbose", "verbose_l2",
           "tlb_verbose", "bus_tlb_verbose", "dir_only", "c4_overflow_halt", "c4_hotspot"]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LO.load(tmp_path_factory.mktemp("link_oracle"))


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _stats_dict(rec) -> dict:
    return A.Stats.from_buffer_copy(rec["stats"].tobytes()).as_dict()


def _fold(completion: np.ndarray):
    """(cores done, max, min, sum) over the cores that completed a request (cycle != -1)."""
    c = completion[completion != -1]
    if len(c) == 0:
        return 0, I64_MIN, I64_MAX, 0
    return len(c), int(c.max()), int(c.min()), int(c.sum())


def _completion_fields(rec):
    return (int(rec["cores_done"]), int(rec["completion_max"]), int(rec["completion_min"]), int(rec["completion_sum"]))


def _assert_equals_host(dr, um, replicas, what, records=None, rows=True):
    """Every record of `replicas` (and, with rows, its map row) equals the host gather's."""
    got = dr.read() if records is None else records
    for r in replicas:
        host, hn, hn1 = P.host_run_results(um, r, queues=True)
        assert got[r].tobytes() == host.tobytes(), f"{what}: replica {r}: {got[r]} != {host}"
        if rows:
            n, n1 = dr.queues(r)
            np.testing.assert_array_equal(n, hn, err_msg=f"{what}: replica {r} n")
            np.testing.assert_array_equal(n1, hn1, err_msg=f"{what}: replica {r} n1")
    return got


def _links(cfg, nq):
    """[(q, kind, a, b)] of the link queues and of the bus queues."""
    ends = [(q,) + P.queue_ends(cfg, q) for q in range(nq)]
    assert all(e[1] in (0, 1, 2, 3) for e in ends)
    links, buses = [e for e in ends if e[1] != 3], [e for e in ends if e[1] == 3]
    assert [e[0] for e in links] == list(range(len(links)))           # links first, then buses
    return links, buses


def _run_golden(c, um):
    if c.closed:
        um.set_replay_mode(U.PU_REPLAY_CLOSED)
    for prog, th in c.threads:
        um.allocCore(prog, th)
    parts = [um.access_batch(c.reqs[a:a + 200_000]) for a in range(0, len(c.reqs), 200_000)]
    c.check_delays(np.concatenate(parts))


def _check_golden(c, um, oracle, what):
    """The gather of replica 0 after the golden ran on it, against every answer there is."""
    cfg = um.cfg
    dr = P.DeviceRunResults(um, queues=True)
    try:
        dr.gather()
        rec = _assert_equals_host(dr, um, [0], what)[0]
        n, n1 = dr.queues(0)
        tn, tn1 = dr.queue_totals()
    finally:
        dr.close()
    np.testing.assert_array_equal(tn, n)                               # one replica: the totals are its row
    np.testing.assert_array_equal(tn1, n1)
    st = _stats_dict(rec)
    assert st == um.stats().as_dict()
    assert_stats_match(st, c)
    halt = c.meta.get("halt_index")
    assert int(rec["halted"]) == (0 if halt is None else 1)
    assert st["requests"] == int(rec["processed"]) == (len(c.reqs) if halt is None else halt + 1)
    assert _completion_fields(rec) == _fold(um.completion()) == _fold(c.completion)
    assert int(rec["cores_done"]) > 0 and int(rec["completion_max"]) == int(c.completion.max())

    links, buses = _links(cfg, len(n))
    t = LO.trace_case(oracle, c, cfg)
    c.check_delays(t.delays)
    net = cfg.sys.network
    hf = net.header_flits
    pb = hf + -(-cfg.sys.cache[cfg.sys.num_levels - 1].block_size // net.data_width)
    want = [t.edges.get((a, b), (0, 0)) for _, _, a, b in links]
    got = [(int(n[q]), hf * int(n[q]) + (pb - hf) * int(n1[q])) for q, _, _, _ in links]
    assert got == want
    assert set(t.edges) <= {(a, b) for _, _, a, b in links}            # no visited edge without a record
    nl = len(links)
    assert int(rec["link_visits"]) == int(n[:nl].sum()) == c.counters["link_visits"]
    assert int(rec["link_block_visits"]) == int(n1[:nl].sum())
    assert sum(f for _, f in got) == c.counters["link_flits"]
    assert int(rec["links_used"]) == sum(1 for v, _ in want if v)
    if nl:
        wv = [v for v, _ in want]
        assert (int(rec["link_max_visits"]), int(rec["link_max_id"])) == (max(wv), wv.index(max(wv)))
    else:
        assert (int(rec["link_max_visits"]), int(rec["link_max_id"])) == (0, -1)
    assert int(rec["bus_visits"]) == int(n[nl:].sum()) == c.counters["bus_accesses"]
    assert not n1[nl:].any()
    assert int(rec["buses_used"]) == int((n[nl:] > 0).sum())
    if buses:
        bv = [int(v) for v in n[nl:]]
        assert (int(rec["bus_max_visits"]), int(rec["bus_max_id"])) == (max(bv), nl + bv.index(max(bv)))
    else:
        assert (int(rec["bus_max_visits"]), int(rec["bus_max_id"])) == (0, -1)
    return rec


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_one_replica(name, oracle):
    c = _case(name)
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    try:
        _run_golden(c, um)
        rec = _check_golden(c, um, oracle, name)
        if name == "c4_hotspot":
            assert int(rec["links_used"]) == 1984 and len(c.completion) == 1024   # several passes, a ragged tail
            assert int(rec["cores_done"]) == int((c.completion != -1).sum())
        if name == "bus_l2_shared":
            assert int(rec["link_max_id"]) == -1 and int(rec["bus_visits"]) > 0
        if name == "c4_overflow_halt":
            assert int(rec["halted"]) == 1 and int(rec["stats"]["error_flags"]) == A.PU_ERRF_NEG_DELAY
    finally:
        um.close()


@pytest.mark.parametrize("mode,kernel", [("0", "pu_jit_uncore_s0_h0"), ("2", "pu_jit_uncore_s0_h1")])
def test_header_placements(mode, kernel, oracle, monkeypatch):
    """The headers kept in HBM for every launch, and in LDS (latency mode) for short batches too."""
    c = _case("c1_stream")
    monkeypatch.delenv("PRIMEUNCORE_RESIDENT", raising=False)
    monkeypatch.setenv("PRIMEUNCORE_LDS_HEADERS", mode)
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    monkeypatch.delenv("PRIMEUNCORE_LDS_HEADERS")
    try:
        if mode == "2":
            um.set_resident(0)
        _run_golden(c, um)
        assert um.last_launch_kernel() == kernel
        _check_golden(c, um, oracle, f"headers {mode}")
    finally:
        um.close()


def test_gather_stops_a_running_resident_kernel():
    """A few hundred uncore_access calls served by the resident kernel, which holds the queue headers
    on chip; the gather joins it and sees the current headers."""
    c = _case("c1_stream")
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    dr = P.DeviceRunResults(um, queues=True)
    try:
        um.set_resident(1)
        for prog, th in c.threads:
            um.allocCore(prog, th)
        k = 300
        for q in c.reqs[:k]:
            um.uncore_access(int(q["core"]), P.InsMem(int(q["mem_type"]), int(q["prog_id"]), int(q["addr"])), int(q["timer"]))
        info = um.resident_info()
        assert info["running"] and info["commands"] == k, "the calls were not served by a resident kernel"
        dr.gather()
        rec = dr.read()[0]
        assert not um.resident_info()["running"]
        n, _ = dr.queues(0)
        assert int(rec["stats"]["requests"]) == k == int(rec["processed"])
        assert int(rec["link_visits"]) == int(n.sum()) == int(rec["stats"]["net_distance"]) > 0
        _assert_equals_host(dr, um, [0], "after the resident kernel")
    finally:
        dr.close()
        um.close()


# ---------------------------------------------------------------- several replicas on a stream
LENGTHS = [3000, 1500, 0, 2500, 700]


def _five(chunks):
    """C1, five replicas with their own seeds and lengths (one has no requests): per chunk the host
    records [sum(LENGTHS)] and the offsets."""
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 16, seed=400 + r, num_quanta=8, max_requests=max(n, 1) * chunks)
             for r, n in enumerate(LENGTHS)]
    streams = [P.generate_stream(sp) for sp in specs]
    assert all(len(s) >= n * chunks for s, n in zip(streams, LENGTHS))
    out = []
    for k in range(chunks):
        out.append(np.concatenate([s[k * n:(k + 1) * n] for s, n in zip(streams, LENGTHS)]))
        assert len(out[-1]) == sum(LENGTHS)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return specs, out, off


def _empty_record(um):
    e = np.zeros(1, dtype=A.DRES_DTYPE)[0]
    e["stats"]["num_levels"] = um.cfg.sys.num_levels
    e["completion_max"], e["completion_min"] = I64_MIN, I64_MAX
    nq, nl = int(U.lib().pu_num_queues(um._handle())), int(U.lib().pu_num_links(um._handle()))
    e["link_max_id"] = 0 if nl else -1                       # unvisited links: 0 visits at the lowest id
    e["bus_max_id"] = nl if nq > nl else -1
    return e


def test_five_replicas_on_a_torch_stream():
    import torch
    dev = torch.device("cuda", 0)
    specs, chunks, off = _five(2)
    um = P.UncoreManager()
    um.init(P.config_from_dict(CF.preset("C1")), replicas=5)
    dr, dr0 = P.DeviceRunResults(um, queues=True), P.DeviceRunResults(um, queues=False)
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        s = torch.cuda.Stream(dev)
        d_off = torch.from_numpy(off).to(dev)
        d_del = torch.zeros(int(off[-1]), dtype=torch.int32, device=dev)
        d_reqs = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).copy()).to(dev) for h in chunks]
        torch.cuda.synchronize(dev)

        # the run and both gathers on one stream, no synchronise between
        um.run_device(d_reqs[0].data_ptr(), d_off.data_ptr(), d_del.data_ptr(), s.cuda_stream)
        dr.gather(stream_ptr=s.cuda_stream)
        dr0.gather(stream_ptr=s.cuda_stream)
        first = dr.read()
        plain = dr0.read()
        totals, totals0 = dr.queue_totals(), dr0.queue_totals()
        s.synchronize()
        _assert_equals_host(dr, um, range(5), "first chunk", records=first)
        assert first.tobytes() == plain.tobytes()            # the map changes no record
        assert [int(x) for x in first["stats"]["requests"]] == LENGTHS
        assert first[2].tobytes() == _empty_record(um).tobytes()
        assert int(first[2]["cores_done"]) == 0 and int(first[2]["completion_min"]) == I64_MAX
        assert int(first[2]["link_max_id"]) == 0 and int(first[2]["link_max_visits"]) == 0   # 24 links, none visited
        rows = [dr.queues(r) for r in range(5)]
        np.testing.assert_array_equal(totals[0], np.sum([n for n, _ in rows], axis=0))
        np.testing.assert_array_equal(totals[1], np.sum([n1 for _, n1 in rows], axis=0))
        np.testing.assert_array_equal(totals0[0], totals[0])  # from the headers: the same sums
        np.testing.assert_array_equal(totals0[1], totals[1])
        assert totals[0].sum() == first["link_visits"].sum() > 0 and not rows[2][0].any()
        with pytest.raises(P.UncoreError, match=r"PU_DRES_QUEUES \(-95\)"):
            dr0.queues(0)
        assert dr.state_bytes - dr0.state_bytes == 5 * 24 * 16 and dr0.state_bytes >= 5 * 448
        assert dr.num_queues == dr0.num_queues == 24 and len(dr) == 5

        # a second chunk changes every running replica; a gather of [1, 3) renews only records 1 and 2
        um.run_device(d_reqs[1].data_ptr(), d_off.data_ptr(), d_del.data_ptr(), s.cuda_stream)
        dr.gather(first=1, n=2, stream_ptr=s.cuda_stream)
        part = dr.read()
        part_rows = [dr.queues(r) for r in range(5)]
        part_totals = dr.queue_totals()
        s.synchronize()
        for r in (0, 3, 4):
            assert part[r].tobytes() == first[r].tobytes(), f"replica {r} was outside the gather"
            np.testing.assert_array_equal(part_rows[r][0], rows[r][0])
        _assert_equals_host(dr, um, [1, 2], "the partial gather", records=part)
        assert int(part[1]["stats"]["requests"]) == 2 * LENGTHS[1]
        np.testing.assert_array_equal(part_totals[0], part_rows[1][0] + part_rows[2][0])   # the last gather's replicas
        assert dr.read(3, 2).tobytes() == part[3:5].tobytes()
        dr.gather(stream_ptr=s.cuda_stream)
        s.synchronize()
        _assert_equals_host(dr, um, range(5), "second chunk")
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            dr.gather(first=4, n=2)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            dr.gather(first=-1, n=1)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            dr.read(0, 6)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            dr.queues(5)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            dr.gather(first=0, n=-1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            dr.read(0, -1)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            dr.read(-1, 1)
        _assert_equals_host(dr, um, range(5), "after the refused calls")     # they changed nothing

        # room for fewer queues than a replica has: -34 from all three entries, the buffers untouched
        L, nq = U.lib(), dr.num_queues
        P64, PREC = C.POINTER(C.c_uint64), C.POINTER(A.DresReplica)
        poison = np.uint64(0xA5A5A5A5A5A5A5A5)
        bn, bn1 = np.full(nq, poison), np.full(nq, poison)
        pn, pn1 = bn.ctypes.data_as(P64), bn1.ctypes.data_as(P64)
        rec = np.zeros(1, dtype=A.DRES_DTYPE)
        for cap in (nq - 1, 0):
            assert L.pu_dres_read_queues(dr._handle(), 1, pn, pn1, cap) == -34
            assert L.pu_dres_read_queue_totals(dr._handle(), pn, pn1, cap) == -34
            assert L.pu_dres_read_queue_totals(dr0._handle(), pn, pn1, cap) == -34
            assert L.pu_dres_host_gather(um._handle(), 1, rec.ctypes.data_as(PREC), pn, pn1, cap) == -34
            assert L.pu_dres_host_gather(um._handle(), 1, rec.ctypes.data_as(PREC), None, pn1, cap) == -34
            assert "fewer queues" in U.last_error()
        assert (bn == poison).all() and (bn1 == poison).all() and not rec.view(np.uint8).any()
        assert L.pu_dres_host_gather(um._handle(), 5, rec.ctypes.data_as(PREC), None, None, 0) == -34
        assert L.pu_dres_host_gather(um._handle(), -1, rec.ctypes.data_as(PREC), None, None, 0) == -34
        assert L.pu_dres_host_gather(um._handle(), 1, None, None, None, 0) == -22
        assert L.pu_dres_read(dr._handle(), 0, 1, None) == -22
        assert L.pu_dres_read_queues(dr._handle(), -1, pn, pn1, nq) == -22
        assert L.pu_dres_read_queues(dr0._handle(), 1, pn, pn1, nq - 1) == -95       # no map comes first
        assert (bn == poison).all() and (bn1 == poison).all()
        assert L.pu_dres_host_gather(um._handle(), 1, rec.ctypes.data_as(PREC), None, None, 0) == 0   # record only: no cap needed
        assert L.pu_dres_read_queues(dr._handle(), 1, pn, pn1, nq) == 0 and (bn != poison).all()
        assert dr.num_links == 24 == int(L.pu_num_links(um._handle()))
    finally:
        dr.close()
        dr0.close()
        um.close()
    with pytest.raises(P.UncoreError, match="closed"):
        dr.read()


def test_snapshot_semantics():
    """Gathering twice gives the same bytes; a second chunk shows; after a reset everything is the empty record."""
    c = _case("c1_stream")
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    dr = P.DeviceRunResults(um, queues=True)
    try:
        for prog, th in c.threads:
            um.allocCore(prog, th)
        assert dr.read()[0].tobytes() == bytes(448)          # before any gather
        assert not dr.queue_totals()[0].any()
        dr.gather()
        assert dr.read()[0].tobytes() == _empty_record(um).tobytes()
        half = len(c.reqs) // 2
        um.access_batch(c.reqs[:half])
        dr.gather()
        a, rows_a = dr.read()[0], dr.queues(0)
        dr.gather()
        b, rows_b = dr.read()[0], dr.queues(0)
        assert a.tobytes() == b.tobytes() and int(a["stats"]["requests"]) == half
        np.testing.assert_array_equal(rows_a[0], rows_b[0])
        np.testing.assert_array_equal(rows_a[1], rows_b[1])
        um.access_batch(c.reqs[half:])
        assert dr.read()[0].tobytes() == a.tobytes()         # a run alone changes no record
        dr.gather()
        full = _assert_equals_host(dr, um, [0], "after the second chunk")[0]
        assert int(full["stats"]["requests"]) == len(c.reqs) == half + len(c.reqs[half:])
        assert _completion_fields(full) == _fold(c.completion)
        um.reset()
        dr.gather()
        after = _assert_equals_host(dr, um, [0], "after reset")[0]
        assert after.tobytes() == _empty_record(um).tobytes()
        assert not dr.queues(0)[0].any() and not dr.queue_totals()[0].any()
    finally:
        dr.close()
        um.close()


def test_pool_path_c4_req16():
    """8 C4 replicas of 2,000 requests as pu_req16 through pu_run_device_pool, gathered on the run's stream."""
    import torch
    R, n, slots = 8, 2000, 4
    dev = torch.device("cuda", 0)
    cfg = P.config_from_dict(CF.preset("C4"))
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 1024, seed=900 + r, max_requests=n) for r in range(R)]
    host = np.stack([P.generate_stream(sp) for sp in specs])
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    dr = P.DeviceRunResults(um, queues=False)
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        um.set_device_req_format(A.PU_REQ_FMT_16)
        off = np.arange(R + 1, dtype=np.uint64) * np.uint64(n)
        d_reqs = torch.from_numpy(np.ascontiguousarray(U.pack_req16(host)).reshape(-1).view(np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_pos = torch.from_numpy(off[:-1].copy().view(np.int64)).to(dev)
        d_del = torch.zeros(R * n, dtype=torch.int32, device=dev)
        d_sched = torch.zeros(um.pool_words(slots), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        for _ in range(20000):
            um.run_device_pool(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(),
                               d_sched.data_ptr(), slots, 300, s.cuda_stream)
            s.synchronize()
            if np.array_equal(d_pos.cpu().numpy().view(np.uint64), off[1:]):
                break
        else:
            raise AssertionError("the runs did not finish")
        assert um.last_launch_kernel() == "pu_jit_uncore_s2_h0"
        dr.gather(stream_ptr=s.cuda_stream)
        got = dr.read()
        totals = dr.queue_totals()                           # no map: from the 8 x 1,984 headers
        s.synchronize()
        want_n = np.zeros(dr.num_queues, dtype=np.uint64)
        for r in range(R):
            host_rec, hn, _ = P.host_run_results(um, r, queues=True)
            assert got[r].tobytes() == host_rec.tobytes(), f"replica {r}"
            want_n += hn
        np.testing.assert_array_equal(totals[0], want_n)
        assert [int(x) for x in got["stats"]["requests"]] == [n] * R and not got["halted"].any()
        assert dr.num_queues == 1984 and (got["link_visits"] > 0).all()
    finally:
        um.set_device_req_format(A.PU_REQ_FMT_32)
        dr.close()
        um.close()


# ---------------------------------------------------------------- the tool
def _tool(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ensemble_summary.py"), "--preset", "C1", "--kind", "1",
                        "--chunk", "2000", *extra], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]


def test_ensemble_summary_tool_results(monkeypatch):
    """--results: the records the tool prints equal a DeviceRunResults gather of the same ensemble
    made here; without the flag the lines have exactly the keys they had before."""
    import torch
    R, n, chunks, base, nc = 3, 2000, 2, 1, 16
    lines = _tool("--results", "--replicas", str(R), "--chunks", str(chunks))
    assert [x.get("replica") for x in lines[:-1]] == list(range(R)) and len(lines) == R + 1
    plain = _tool("--replicas", "1", "--chunks", "1")
    assert len(plain) == 1 and list(plain[0]) == ["replica", "seed", "requests", "read", "write", "core_out_of_range",
                                                   "error_flags"]
    assert all(list(x) == list(plain[0]) + ["results"] for x in lines[:-1])

    cfg = P.config_from_dict(CF.preset("C1"))
    quantum = cfg.thread_sync_interval
    quanta = -(-n * chunks * 4 // (nc * quantum)) + 1          # as the tool sizes its streams
    specs = [P.StreamSpec(A.PU_STREAM_PRIVATE_STREAMING, nc, seed=base + k, quantum=quantum, num_quanta=quanta,
                          max_msg=cfg.max_msg_size) for k in range(R)]
    hss = P.StreamSet(specs)
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    dr = P.DeviceRunResults(um, queues=True)
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
        dr.gather()
        recs = dr.read()
        totals = dr.queue_totals()
        _assert_equals_host(dr, um, range(R), "the tool's ensemble", records=recs)
    finally:
        dr.close()
        um.close()
        hss.close()
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    from ensemble_summary import hottest_links, results_object
    for k in range(R):
        want = json.loads(json.dumps(results_object(cfg, recs[k])))
        assert lines[k]["results"] == want, f"replica {k}"
        assert want["requests"] == n * chunks and want["end_cycle"] == int(recs[k]["completion_max"]) > 0
        hot = want["hottest_link"]
        assert hot["visits"] == int(recs[k]["link_max_visits"]) > 0 and hot["kind"] in ("x", "y")
        assert (hot["kind"], hot["a"], hot["b"]) == (U.QUEUE_KINDS[P.queue_ends(cfg, hot["id"])[0]],) + P.queue_ends(cfg, hot["id"])[1:]
    last = lines[-1]
    assert last == json.loads(json.dumps({"replicas": R, "hottest_links": hottest_links(cfg, totals[0], totals[1], 24)}))
    top = last["hottest_links"]
    assert len(top) == 10 and [t["visits"] for t in top] == sorted((t["visits"] for t in top), reverse=True)
    assert top[0]["visits"] == int(totals[0].max())
