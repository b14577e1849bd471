"""Forking a warmed replica and its request stream on the device
(UncoreManager.fork_replica / pu_replica_fork, primesim_amd/csrc/replica_fork.hip;
DeviceStreamSet.fork / pu_dstream_fork, primesim_amd/csrc/stream_gen.hip).

A fork must be the state of an uncore that lived through the prefix itself: a replica
forked part-way through a golden (inside a message, so the run state carries the open
message) continues to the reference's delays, completion cycles and report, whatever
the destination held before.  The kernel is checked against its twin
(PU_FORK_BY_COPIES), at one destination, at more destinations than groups, with the
source inside the range, past 4 GiB of arena, after resident mode, with per-replica
schedulers and from a halted source.  The stream fork equals the host's
(tests/test_fork_abi.py pins that one), and the two together equal the CPU restatement
run on the warm-up followed by the forked continuation.

Engine runs use the engine's own stream (stream_ptr = 0) unless a test is about another.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle as O
import primesim_amd as P
from abi_helpers import ROOT
from dram_cases import STREAM_CASES, bank_config
from golden_util import Case
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FILL = 0xA5


def _run(um, parts, stream_ptr=0):
    """Replica r runs parts[r] (None or empty: nothing) through run_device; returns the delays per replica."""
    parts = [np.zeros(0, dtype=A.REQ_DTYPE) if p is None else p for p in parts]
    assert len(parts) == um.replicas
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    allr = np.concatenate(parts)
    d_reqs = torch.from_numpy(allr.view(np.uint8).copy()).to(DEV)
    d_off = torch.from_numpy(off).to(DEV)
    d_del = torch.full((max(len(allr), 1),), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), stream_ptr)
    um.synchronize()
    host = d_del.cpu().numpy()
    return [host[off[r]:off[r + 1]] for r in range(len(parts))]


def _only(R, **at):
    """parts for _run: replica r runs at[r] (keys "r<index>"), the others nothing."""
    parts = [None] * R
    for k, v in at.items():
        parts[int(k[1:])] = v
    return parts


def _cut(reqs, at=None):
    """The first index at or after half the stream (or `at`) that is not a batch start: a fork there
    carries an open message."""
    k = len(reqs) // 2 if at is None else at
    while reqs["batch_start"][k]:
        k += 1
    assert 0 < k < len(reqs) - 1
    return k


def _stale(reqs):
    """A different stream of the same length and shape: every address moved by 1 MiB."""
    s = reqs.copy()
    s["addr"] += 1 << 20
    return s


def _engine(cfg, threads, R, closed=False):
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    if closed:
        um.set_replay_mode(U.PU_REPLAY_CLOSED)
    for prog, th in threads:
        um.allocCore(prog, th)
    return um


def _same_state(um, a, b):
    """Replicas a and b answer alike: statistics, completion cycles, the end-of-run record."""
    assert um.stats(a).as_dict() == um.stats(b).as_dict()
    np.testing.assert_array_equal(um.completion(a), um.completion(b))
    assert P.host_run_results(um, a).tobytes() == P.host_run_results(um, b).tobytes()
    assert um.report(a) == um.report(b)


# ------------------------------------------------------------------ 1. a fork is the state of the prefix
GOLDENS = ["c1_stream", "tlb_c1", "bus_c1", "c2_canneal", "c1_closed", "verbose", "limited_ptr"]


@functools.lru_cache(maxsize=None)
def _golden(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _bank_case():
    """One bank-model case of tests/dram_cases.py with what oracle.CpuRef says of it."""
    name, preset, over, kind, cores, progs, n = STREAM_CASES[0]
    cfg = bank_config(preset, **over)
    spec = P.StreamSpec(kind, cores, seed=11, num_progs=progs, max_requests=n)
    reqs = P.generate_stream(spec)
    ref = O.CpuRef(cfg)
    for prog, th in P.stream_threads(spec):
        ref.alloc_core(prog, th)
    delays, rc = ref.run(reqs)
    assert rc == 0
    st = ref.stats().as_dict()
    assert st["dram_row_hits"] + st["dram_row_conflicts"] > 0          # the banks are in play
    return cfg, P.stream_threads(spec), reqs, delays, ref.completion(), st


def _fork_mid_stream(cfg, threads, closed, reqs, by_copies):
    """Three replicas; 1 and 2 hold another stream's state; 0 runs reqs[:k]; 0 -> 1, 2; 1 runs reqs[k:].
    Returns (engine, k, replica 1's delays over reqs[k:])."""
    k = _cut(reqs)
    um = _engine(cfg, threads, 3, closed)
    try:
        stale = _stale(reqs)
        _run(um, [None, stale, stale])
        assert um.stats(1).requests == len(reqs) and um.stats(0).requests == 0
        head = _run(um, _only(3, r0=reqs[:k]))[0]
        um.fork_replica(0, 1, 2, by_copies=by_copies)
        _same_state(um, 0, 2)
        _same_state(um, 0, 1)
        assert um.stats(2).requests == k
        tail = _run(um, _only(3, r1=reqs[k:]))[1]
        _same_state(um, 0, 2)                                      # running replica 1 moved neither
    except BaseException:
        um.close()
        raise
    return um, k, head, tail


@pytest.mark.parametrize("by_copies", [False, True], ids=["kernel", "copies"])
@pytest.mark.parametrize("name", GOLDENS)
def test_fork_inside_a_golden_continues_to_the_reference(name, by_copies):
    c = _golden(name)
    um, k, head, tail = _fork_mid_stream(P.load_config(c.xml_path), c.threads, c.closed, c.reqs, by_copies)
    try:
        np.testing.assert_array_equal(head, c.delays[:k])
        np.testing.assert_array_equal(tail, c.delays[k:])
        np.testing.assert_array_equal(um.completion(1), c.completion)
        assert um.report(1) == c.report
        assert um.stats(1).error_flags == 0
    finally:
        um.close()


@pytest.mark.parametrize("by_copies", [False, True], ids=["kernel", "copies"])
def test_fork_carries_the_dram_banks(by_copies):
    cfg, threads, reqs, delays, completion, stats = _bank_case()
    um, k, head, tail = _fork_mid_stream(cfg, threads, False, reqs, by_copies)
    try:
        np.testing.assert_array_equal(head, delays[:k])
        np.testing.assert_array_equal(tail, delays[k:])
        np.testing.assert_array_equal(um.completion(1), completion)
        gs = um.stats(1).as_dict()
        assert {k: gs[k] for k in stats if k != "requests"} == {k: stats[k] for k in stats if k != "requests"}
        assert gs["requests"] == len(reqs)
    finally:
        um.close()


# ------------------------------------------------------------------ 2. kernel shapes
# (replicas, src, first, n, destinations that go on with the golden's tail); the kernel deals the
# destinations to at most 64 groups, so 130 of them make a group walk up to three
SHAPES = [(3, 0, 2, 1, [2]),
          (132, 0, 1, 130, [1, 64, 65, 66, 129, 130]),
          (5, 2, 0, 5, [0, 1, 2, 3, 4]),
          (4, 3, 0, 4, [0, 1, 2, 3])]


@pytest.mark.parametrize("R,src,first,n,check", SHAPES, ids=["one", "130", "src-in-the-middle", "src-last"])
def test_kernel_shapes(R, src, first, n, check):
    c = _golden("c1_stream")
    k = _cut(c.reqs)
    outside = [r for r in range(R) if r != src and not first <= r < first + n]
    k2 = _cut(c.reqs, len(c.reqs) // 4)                            # the outsiders' own cut
    um = _engine(P.load_config(c.xml_path), c.threads, R)
    try:
        assert um.replica_bytes % 4096 == 0
        parts = _only(R, **{f"r{src}": c.reqs[:k]})
        for r in outside:
            parts[r] = c.reqs[:k2]
        _run(um, parts)
        um.fork_replica(src, first, n)
        parts = [None] * R
        for r in check:
            parts[r] = c.reqs[k:]
        for r in outside:
            parts[r] = c.reqs[k2:]
        got = _run(um, parts)
        for r in check:
            np.testing.assert_array_equal(got[r], c.delays[k:], err_msg=f"replica {r}")
        for r in outside:                                          # not in the range: its own continuation
            np.testing.assert_array_equal(got[r], c.delays[k2:], err_msg=f"replica {r} (outside the range)")
        for r in check + outside:
            np.testing.assert_array_equal(um.completion(r), c.completion)
            assert um.report(r) == c.report
        rest = [r for r in range(first, first + n) if r not in check and r != src]
        for r in rest[:: max(1, len(rest) // 8)]:                  # forked and left alone: still the source at the fork
            assert um.stats(r).requests == k
    finally:
        um.close()


def test_fork_arguments_with_a_handle():
    c = _golden("c1_stream")
    um = _engine(P.load_config(c.xml_path), c.threads, 3)
    try:
        h = um._handle()
        assert lib().pu_replica_fork(h, 3, 0, 1, 0, None) == -34 and "source replica out of range" in U.last_error()
        assert lib().pu_replica_fork(h, 0, 1, 3, 0, None) == -34 and "more replicas" in U.last_error()
        assert lib().pu_replica_fork(h, 0, 3, 1, 0, None) == -34
        assert lib().pu_replica_fork(h, 0, 0, 1, 2, None) == -22 and "unknown flags" in U.last_error()
        assert lib().pu_replica_fork(h, 0, 0, -1, 0, None) == -22
        for flags in (0, A.PU_FORK_BY_COPIES):
            assert lib().pu_replica_fork(h, 0, 3, 0, flags, None) == 0      # n == 0: nothing to do
            assert lib().pu_replica_fork(h, 1, 1, 1, flags, None) == 0      # only the source itself
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            um.fork_replica(0, 2, 2)
        np.testing.assert_array_equal(_run(um, _only(3, r1=c.reqs))[1], c.delays)   # nothing was touched
    finally:
        um.close()


# ------------------------------------------------------------------ 3. offsets past 4 GiB
def test_fork_past_4_gib():
    cfg = P.config_from_dict(CF.preset("C4"))
    R, n = 260, 2000
    spec = P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 1024, seed=21, num_quanta=64, max_requests=2 * n)
    reqs = P.generate_stream(spec)
    assert len(reqs) == 2 * n
    ref = O.CpuRef(cfg)
    for prog, th in P.stream_threads(spec):
        ref.alloc_core(prog, th)
    want, rc = ref.run(reqs)
    assert rc == 0
    um = _engine(cfg, P.stream_threads(spec), R)
    try:
        assert um.replica_bytes * (R - 1) > 4 << 30
        np.testing.assert_array_equal(_run(um, _only(R, r0=reqs[:n]))[0], want[:n])
        um.fork_replica(0, 0, R)
        got = _run(um, _only(R, r0=reqs[n:], r1=reqs[n:], r131=reqs[n:], r259=reqs[n:]))
        for r in (0, 1, 131, 259):
            np.testing.assert_array_equal(got[r], want[n:], err_msg=f"replica {r}")
            np.testing.assert_array_equal(um.completion(r), ref.completion())
        assert um.stats(258).requests == n and um.stats(259).requests == 2 * n
    finally:
        um.close()


# ------------------------------------------------------------------ 4. resident mode
def test_fork_after_resident_mode():
    """Replica 0 is fed request by request through the resident kernel, whose queue headers live in
    LDS until it is joined.  uncore_access treats every request as a message of its own (the caller
    carries the running delay), so no message is open in the engine at the cut: the cut is the first
    batch start at or after half the stream, where access_batch can take over."""
    c = _golden("c1_stream")
    k = len(c.reqs) // 2
    while not c.reqs["batch_start"][k]:
        k += 1
    um = _engine(P.load_config(c.xml_path), c.threads, 2)
    try:
        if not um.resident_info()["eligible"]:
            pytest.fail("c1_stream is expected to be eligible for resident mode")
        D = 0
        for i in range(k):
            q = c.reqs[i]
            if q["batch_start"]:
                D = 0
            d = um.uncore_access(int(q["core"]), P.InsMem(int(q["mem_type"]), int(q["prog_id"]), int(q["addr"])),
                                 int(q["timer"]) + D)
            assert d == c.delays[i], i
            D += d - 1
        assert um.resident_info()["running"]
        um.fork_replica(0, 1, 1)
        assert not um.resident_info()["running"]                   # joined: the headers were in device memory
        np.testing.assert_array_equal(um.access_batch(c.reqs[k:], replica=1), c.delays[k:])
        np.testing.assert_array_equal(um.completion(1), c.completion)
        assert um.report(1) == c.report
    finally:
        um.close()


# ------------------------------------------------------------------ 5. per-replica scheduler
def test_fork_copies_or_drops_the_per_replica_scheduler():
    L = lib()
    um = P.UncoreManager()
    um.init(P.config_from_dict(CF.preset("C1")), replicas=3)
    try:
        h = um._handle()
        assert [um.allocCore(1, t) for t in range(2)] == [0, 1]             # the shared scheduler: two cores taken
        assert L.pu_alloc_core_replica(h, 1, 5, 0) == 2                     # replica 1's own copy knows (5, 0)
        assert L.pu_get_core_id_replica(h, 1, 5, 0) == 2
        um.fork_replica(0, 1, 1)                                           # replica 0 reads the shared one
        assert L.pu_get_core_id_replica(h, 1, 5, 0) == 0                    # unknown there: ThreadSched's 0
        assert L.pu_alloc_core_replica(h, 0, 7, 3) == 2                     # now replica 0 has its own
        assert L.pu_alloc_core_replica(h, 0, 7, 4) == 3
        um.fork_replica(0, 1, 2)
        for r in (1, 2):
            assert L.pu_get_core_id_replica(h, r, 7, 4) == L.pu_get_core_id_replica(h, 0, 7, 4) == 3
            assert L.pu_alloc_core_replica(h, r, 9, 0) == 4                 # a copy, not the source's own
        assert L.pu_alloc_core_replica(h, 0, 9, 1) == 4
    finally:
        um.close()


# ------------------------------------------------------------------ 6. a halted source
def test_fork_of_a_halted_replica_is_halted():
    c = _golden("c4_overflow_halt")
    halt = c.meta["halt_index"]
    assert halt == 34904
    um = _engine(P.load_config(c.xml_path), c.threads, 2)
    try:
        np.testing.assert_array_equal(_run(um, [c.reqs, None])[0], c.delays)
        um.fork_replica(0, 1, 1)
        flags = um.error_flags()
        assert flags[0] == flags[1] and flags[1] & A.PU_ERRF_NEG_DELAY
        lim = um.limit_positions()
        assert lim[0] == lim[1]
        a, b = P.host_run_results(um, 0), P.host_run_results(um, 1)
        assert a.tobytes() == b.tobytes() and b["halted"] != 0 and b["stats"]["requests"] == halt + 1
        more = c.reqs[:500]
        got = _run(um, [more, more])
        assert not got[0].any() and not got[1].any()
    finally:
        um.close()


# ------------------------------------------------------------------ 7. DeviceStreamSet.fork
KINDS = [A.PU_STREAM_PRIVATE_STREAMING, A.PU_STREAM_SHARED_UNIFORM, A.PU_STREAM_MULTIPROGRAM,
         A.PU_STREAM_UNIFORM_HOTSPOT, A.PU_STREAM_PRODUCER_CONSUMER, A.PU_STREAM_UNIFORM]
#                  cores quantum quanta max_msg progs      (tests/test_gpu_dstream.py)
STREAM_SHAPES = {"S1": (48, 200, 3, 9, 2), "S2": (1, 50, 4, 3, 1), "S3": (70, 2, 40, 5, 3),
                 "S4": (1030, 40, 2, 100, 4), "S5": (64, 3, 30, 2, 1)}
ADVANCE = [7, 100, 4096]
LATER = 600                                                        # records of each later chunk


def _spec(kind, shape, seed=7):
    c, q, nq, mm, pr = STREAM_SHAPES[shape]
    return P.StreamSpec(kind, c, seed=seed, quantum=q, num_quanta=nq, max_msg=mm, num_progs=pr)


def _dev_chunk(dss, n, fmt=A.PU_REQ_FMT_32, stream=None):
    """The next n records of every stream as bytes [count, got, rec]; a row of FILL above and below
    every stream's records and the records past got must still hold FILL."""
    rec = 32 if fmt == A.PU_REQ_FMT_32 else 16
    count = len(dss)
    buf = torch.full((count, n + 2, rec), FILL, dtype=torch.uint8, device=DEV)
    got = torch.full((count,), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    dss.next_into(buf[0, 1:].data_ptr(), n, stride=n + 2, fmt=fmt, d_got_ptr=got.data_ptr(),
                  stream_ptr=stream.cuda_stream if stream is not None else 0)
    dss.positions()                                                # waits for the call
    if stream is not None:
        stream.synchronize()
    b, g = buf.cpu().numpy(), got.cpu().numpy()
    out = []
    for i in range(count):
        assert np.all(b[i, 0] == FILL) and np.all(b[i, 1 + g[i]:] == FILL), f"stream {i}: bytes outside its records"
        out.append(b[i, 1:1 + g[i]])
    return out


def _host_chunk(ss, n, fmt=A.PU_REQ_FMT_32):
    """StreamSet's next n records of every stream, stream by stream, as the same bytes."""
    out = []
    for h in ss._h:
        r = np.zeros(n, dtype=A.REQ_DTYPE)
        got = lib().pu_stream_next(h, r.ctypes.data, n)
        r = r[:got]
        out.append(r.view(np.uint8).reshape(got, 32) if fmt == A.PU_REQ_FMT_32 else
                   U.pack_req16(np.ascontiguousarray(r)).view(np.uint8).reshape(got, 16))
    return out


@pytest.mark.parametrize("shape", list(STREAM_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_device_clone_continues_the_source(kind, shape):
    specs = [_spec(kind, shape), _spec(kind, shape, seed=99), _spec(kind, shape, seed=5)]
    for adv in ADVANCE:
        dss, hss = P.DeviceStreamSet(specs), P.StreamSet(specs)
        try:
            for a, b in zip(_dev_chunk(dss, adv), _host_chunk(hss, adv)):
                np.testing.assert_array_equal(a, b)
            dss.fork(0, 1, 1)
            pos = dss.positions()
            assert pos[1] == pos[0] == hss.position(0) and pos[2] == hss.position(2)
            for fmt in (A.PU_REQ_FMT_32, A.PU_REQ_FMT_16, A.PU_REQ_FMT_32):
                d, h = _dev_chunk(dss, LATER, fmt), _host_chunk(hss, LATER, fmt)
                np.testing.assert_array_equal(d[1], d[0], err_msg=f"adv {adv} fmt {fmt}: the clone")
                np.testing.assert_array_equal(d[0], h[0], err_msg=f"adv {adv} fmt {fmt}: the source")
                np.testing.assert_array_equal(d[2], h[2], err_msg=f"adv {adv} fmt {fmt}: the bystander")
            pos = dss.positions()
            assert pos[1] == pos[0] == hss.position(0) and pos[2] == hss.position(2)
        finally:
            dss.close()
            hss.close()


@pytest.mark.parametrize("shape", list(STREAM_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_device_reseeded_fork_equals_the_host_fork(kind, shape):
    """Four streams, the source second: fork(1, 0, 3) leaves it alone and ignores its seed; stream 3 is outside."""
    specs = [_spec(kind, shape, seed=s) for s in (99, 7, 5, 3)]
    seeds = [1234567, 1, (1 << 40) + 17]
    s = torch.cuda.Stream(DEV)
    for adv in ADVANCE:
        dss, hss = P.DeviceStreamSet(specs), P.StreamSet(specs)
        try:
            for a, b in zip(_dev_chunk(dss, adv, stream=s), _host_chunk(hss, adv)):
                np.testing.assert_array_equal(a, b)
            dss.fork(1, 0, 3, seeds=seeds, stream_ptr=s.cuda_stream)
            hss.fork(1, 0, 3, seeds=seeds)
            np.testing.assert_array_equal(dss.positions(), [hss.position(i) for i in range(4)])
            for fmt in (A.PU_REQ_FMT_32, A.PU_REQ_FMT_16):
                for i, (a, b) in enumerate(zip(_dev_chunk(dss, LATER, fmt, stream=s), _host_chunk(hss, LATER, fmt))):
                    np.testing.assert_array_equal(a, b, err_msg=f"adv {adv} fmt {fmt} stream {i}")
            np.testing.assert_array_equal(dss.positions(), [hss.position(i) for i in range(4)])
        finally:
            dss.close()
            hss.close()


def test_device_fork_refusals_change_nothing():
    kind = A.PU_STREAM_SHARED_UNIFORM
    specs = [_spec(kind, "S1"), _spec(kind, "S1", seed=8), _spec(kind, "S5", seed=9)]
    dss, hss = P.DeviceStreamSet(specs), P.StreamSet(specs)
    try:
        _dev_chunk(dss, 100), _host_chunk(hss, 100)
        before = dss.positions()
        with pytest.raises(P.UncoreError, match=r"stream 2 differ.*\(-22\)"):
            dss.fork(0, seeds=[1, 2, 3])                            # stream 1 would fit: all or nothing
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            dss.fork(3, 0, 1)
        with pytest.raises(P.UncoreError, match=r"\(-34\)"):
            dss.fork(0, 1, 3)
        with pytest.raises(P.UncoreError, match=r"\(-22\)"):
            dss.fork(0, 0, -1)
        dss.fork(0, 1, 0)                                           # no destination: nothing to do
        dss.fork(1, 1, 1, seeds=[5])                                # only the source itself
        np.testing.assert_array_equal(dss.positions(), before)
        for a, b in zip(_dev_chunk(dss, LATER), _host_chunk(hss, LATER)):
            np.testing.assert_array_equal(a, b)
    finally:
        dss.close()
        hss.close()


# ------------------------------------------------------------------ 8. end to end
def test_warm_once_fork_and_run_equals_the_oracle():
    """C2, six replicas: replica 0 runs one warm-up chunk of device stream 0; the engine fork and the
    stream fork (seeds 300 + r) follow on the same torch stream; then two chunks for everyone."""
    R, n, chunks = 6, 2000, 2
    cfg = P.config_from_dict(CF.preset("C2"))
    specs = [P.StreamSpec(A.PU_STREAM_SHARED_UNIFORM, 64, seed=300 + r) for r in range(R)]
    seeds = [300 + r for r in range(R)]
    um = _engine(cfg, P.stream_threads(specs[0]), R)
    dss = P.DeviceStreamSet(specs)
    try:
        d_reqs = torch.full((R, n, 32), FILL, dtype=torch.uint8, device=DEV)
        d_off = torch.arange(R + 1, dtype=torch.int64, device=DEV) * n
        d_warm = d_off.clamp(max=n)
        d_del = torch.full((R, n), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        s = torch.cuda.Stream(DEV)
        sp = s.cuda_stream
        dss.next_into(d_reqs.data_ptr(), n, stream_ptr=sp)
        um.run_device(d_reqs.data_ptr(), d_warm.data_ptr(), d_del.data_ptr(), sp)
        s.synchronize()
        delays = [[d_del[r].cpu().numpy().copy()] if r == 0 else [] for r in range(R)]
        um.fork_replica(0, stream_ptr=sp)
        dss.fork(0, seeds=seeds, stream_ptr=sp)
        for _ in range(chunks):
            dss.next_into(d_reqs.data_ptr(), n, stream_ptr=sp)
            um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sp)
            s.synchronize()
            got = d_del.cpu().numpy()
            for r in range(R):
                delays[r].append(got[r].copy())
        np.testing.assert_array_equal(dss.positions(), [n * (1 + chunks)] * R)

        hss = P.StreamSet(specs)
        try:
            warm = hss.next(n)[0].copy()
            hss.fork(0, seeds=seeds)
            cont = np.concatenate([hss.next(n) for _ in range(chunks)], axis=1)
        finally:
            hss.close()
        for r in range(R):
            reqs = np.concatenate([warm, cont[r]])
            ref = O.CpuRef(cfg)
            for prog, th in P.stream_threads(specs[0]):
                ref.alloc_core(prog, th)
            want, rc = ref.run(reqs)
            assert rc == 0
            np.testing.assert_array_equal(np.concatenate(delays[r]), want if r == 0 else want[n:], err_msg=f"replica {r}")
            gs, ws = um.stats(r).as_dict(), ref.stats().as_dict()
            assert {k: gs[k] for k in ws if k != "requests"} == {k: ws[k] for k in ws if k != "requests"}, r
            assert gs["requests"] == n * (1 + chunks) and gs["error_flags"] == 0
            np.testing.assert_array_equal(um.completion(r), ref.completion())
    finally:
        dss.close()
        um.close()


def test_ensemble_tool_with_a_shared_warm_up():
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ensemble_summary.py"), "--preset", "C2", "--kind", "2",
           "--replicas", "4", "--chunk", "2000", "--chunks", "2", "--warmup-chunks", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [l["replica"] for l in lines] == [0, 1, 2, 3]
    assert all(l["error_flags"] == 0 and l["requests"] == 4000 for l in lines)
    assert len({l["read"]["sum"] for l in lines}) == 4                 # four seeds, four different runs
