"""The sweep x kernel matrix: the seeded sweep's 64 small random configurations
(tests/config_sweep.py) through every engine kernel.

The golden x kernel matrix (kernel_matrix.py) pins chosen configurations; the
sweep crosses every axis pu::config_geometry accepts and reaches values no
golden holds (16-byte blocks, 3-way sets, directories of 12 sets, 27-, 36- and
70-core meshes, ...).  tests/test_config_sweep_oracle.py holds the CPU
restatement (oracle/cpu_ref.cpp) equal to the reference on these draws; here
the same draws run on each of the six kernels of kernel_matrix.KERNELS and must
equal the restatement: every delay, completion cycle, counter, error flag and
the request count.  Nothing here reads the reference.

The streams are short (12 to 4,000 requests) and 27 of them hold no request
inside a message, so the cells have a driver of their own instead of
kernel_matrix's (whose cuts and resume counts assume long streams of
multi-request messages):

  host kernels    one replica, access_batch in two chunks cut at n // 2, the
                  cut moved forward to a request inside a message when one
                  follows (an open message then carries across the calls);
  device kernels  three replicas from device buffers, replicas 0 and 2 the
                  whole stream and replica 1 its second half from a message
                  start, time-sliced until every position reaches its end.

A trial on which the restatement raises a reference-undefined flag (any bit
besides PU_ERRF_NEG_DELAY) is "flagged": the engine must raise the same flags,
report the same first position p (pu_limit_positions) and agree on the delays
[0, p), as include/primeuncore.h promises; nothing after p is compared.

This module holds no test: tests/test_gpu_config_sweep.py runs the cells on the
GPU, tests/test_config_sweep_table.py checks the table on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import config_sweep as CS
import kernel_matrix as KM
from kernel_matrix import KERNELS, POOL_SLOTS, REPLICAS, RESIDENT_CAP, S0_H0, S0_H1, S1_H0, S1_H1, S2_H0, S3_H1

PU_ESTATE = -71           # include/primeuncore.h
MAX_UNDEFINED = 0.30      # the CPU sweep's bound on the share of flagged trials
LAUNCH_CAP = 20000        # launches of one device cell (kernel_matrix's)
NO_LIMIT = np.uint64(2**64 - 1)


def cells() -> list[tuple[int, str]]:
    """Every (trial, kernel) pair: none is left out (the largest sweep mesh has
    70 nodes, far under the 3,400 queues of the LDS header image)."""
    return [(i, k) for i in range(CS.TRIALS) for k in KERNELS]


@dataclass
class Trial:
    index: int
    cfg: object            # SimCfg
    reqs: np.ndarray       # read-only
    threads: list
    closed: bool
    what: str              # the CPU sweep's name of the trial


@dataclass
class Expected:
    """A cold run of the CPU restatement on one replica's stream."""
    delays: np.ndarray
    rc: int                # 0, or the request count at the prime.cpp:130-134 halt
    flags: int
    completion: np.ndarray
    stats: dict
    limit_at: int | None   # flagged: the first request that raised a reference-undefined flag


_TRIALS: list[Trial] = []
_EXPECTED: dict[tuple[int, int], Expected] = {}


def trial(i: int) -> Trial:
    """Trial i, drawn once and shared (nothing writes to it)."""
    import primesim_amd as P
    if not _TRIALS:
        for k, (sim, spec, replay, _) in enumerate(CS.trials()):
            sp = P.StreamSpec(**spec)
            reqs = P.generate_stream(sp)
            reqs.setflags(write=False)
            _TRIALS.append(Trial(k, P.config_from_dict(sim), reqs, P.stream_threads(sp), replay == "closed",
                                 CS.what(k, sim, spec, replay)))
    return _TRIALS[i]


def host_cuts(reqs: np.ndarray) -> list[int]:
    """Chunk bounds for access_batch: two chunks cut at n // 2, the cut moved
    forward to the next request inside a message if there is one; one chunk
    for a stream of fewer than two requests."""
    n = len(reqs)
    if n < 2:
        return [0, n]
    cut = n // 2
    inside = np.nonzero(reqs["batch_start"][cut:] == 0)[0]
    if len(inside):
        cut += int(inside[0])
    return [0, cut, n]


def second_half_start(reqs: np.ndarray) -> int:
    """Replica 1's stream: from the first message that starts at or after
    n // 2; the whole stream when none does."""
    n = len(reqs)
    starts = np.nonzero(reqs["batch_start"][n // 2:])[0]
    return n // 2 + int(starts[0]) if len(starts) else 0


def _cold(t: Trial):
    import oracle as O
    ref = O.CpuRef(t.cfg)
    if t.closed:
        ref.set_mode(O.MODE_CLOSED)
    for prog, th in t.threads:
        ref.alloc_core(prog, th)
    return ref


def expected(i: int, start: int) -> Expected:
    """The restatement's results for trial i's stream from request `start`
    (0, or second_half_start), from a cold state in the trial's replay mode;
    computed once and shared."""
    from primesim_amd import _abi as A
    if (i, start) not in _EXPECTED:
        t = trial(i)
        reqs = t.reqs[start:]
        ref = _cold(t)
        delays, rc = ref.run(reqs)
        st = ref.stats().as_dict()
        flags, limit_at = int(st["error_flags"]), None
        if flags & ~A.PU_ERRF_NEG_DELAY:
            # where: a second cold run, one request a call (the restatement keeps
            # an open message's state across calls), up to the first such flag.
            # The restatement goes on past it; the engine stops there, so the
            # flags to expect are those raised so far.
            step = _cold(t)
            for k in range(len(reqs)):
                d, r = step.run(reqs[k:k + 1])
                assert r == 0 and d[0] == delays[k], f"{t.what}: the restatement differs from itself at request {k}"
                flags = int(step.stats().error_flags)
                if flags & ~A.PU_ERRF_NEG_DELAY:
                    limit_at = k
                    break
            assert limit_at is not None
        delays.setflags(write=False)
        _EXPECTED[(i, start)] = Expected(delays, rc, flags, ref.completion(), st, limit_at)
    return _EXPECTED[(i, start)]


def flagged_trials() -> list[int]:
    """The trials whose whole stream the restatement leaves at a reference-undefined flag."""
    return [i for i in range(CS.TRIALS) if expected(i, 0).limit_at is not None]


def check_cap() -> None:
    """At most 30 % of the trials may be flagged: the file can never pass by comparing mostly nothing."""
    f = flagged_trials()
    assert len(f) <= MAX_UNDEFINED * CS.TRIALS, \
        f"{len(f)} of {CS.TRIALS} sweep trials stop at a reference-undefined flag: {f}"


def _assert_delays(got: np.ndarray, want: np.ndarray, what: str) -> None:
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else []
    if len(bad):
        k = int(bad[0])
        what += (f": {len(bad)} of {len(want)} delays differ, the first at request {k}: "
                 f"engine {int(got[k])}, CPU restatement {int(want[k])}")
    np.testing.assert_array_equal(got, want, err_msg=what)


def _check_replica(um, replica: int, got: np.ndarray, limit, want: Expected, what: str) -> None:
    """One replica's results against the restatement's.  `limit`: the position
    (in the replica's stream) pu_limit_positions reported, None if it never
    reported one."""
    from primesim_amd import _abi as A
    what = f"{what}, replica {replica}"
    n = len(want.delays)
    assert len(got) == n, what
    gs = um.stats(replica).as_dict()
    if want.limit_at is not None:           # flagged: the engine noticed too, and was exact up to there
        assert gs["error_flags"] == want.flags, \
            f"{what}: error flags, engine {gs['error_flags']:#x}, CPU restatement {want.flags:#x}"
        assert limit is not None, f"{what}: no limit position, the CPU restatement stops at request {want.limit_at}"
        assert limit < n, f"{what}: limit position {limit} of {n} requests"
        _assert_delays(got[:limit], want.delays[:limit], f"{what}, before the limit position {limit}")
        assert limit == want.limit_at, f"{what}: limit position, engine {limit}, CPU restatement {want.limit_at}"
        return
    assert limit is None, f"{what}: the engine reported a limit at request {limit}, the CPU restatement none"
    _assert_delays(got, want.delays, what)
    np.testing.assert_array_equal(um.completion(replica), want.completion, err_msg=f"{what}: completion cycles")
    assert gs.keys() == want.stats.keys(), what
    bad = {k: (gs[k], want.stats[k]) for k in want.stats if k != "requests" and gs[k] != want.stats[k]}
    assert not bad, f"{what}: counters differ (engine, CPU restatement): {bad}"
    if want.rc == 0:
        assert gs["error_flags"] == 0 and gs["requests"] == n, what
    else:                                   # the prime.cpp:130-134 halt
        assert want.rc > 0, what
        assert gs["error_flags"] == A.PU_ERRF_NEG_DELAY and gs["requests"] == want.rc, what


def _init(t: Trial, replicas: int, lds_headers: str | None, monkeypatch):
    """A handle on the trial's configuration, created under the given
    PRIMEUNCORE_LDS_HEADERS (None: the default environment), its code objects
    the build-time warm-up's: a trial the warm-up misses fails here instead of
    compiling on the GPU machine."""
    import primesim_amd as P
    from primesim_amd import uncore
    monkeypatch.delenv("PRIMEUNCORE_RESIDENT", raising=False)
    if lds_headers is None:
        monkeypatch.delenv("PRIMEUNCORE_LDS_HEADERS", raising=False)
    else:
        monkeypatch.setenv("PRIMEUNCORE_LDS_HEADERS", lds_headers)
    um = P.UncoreManager()
    um.init(t.cfg, replicas=replicas)
    try:
        assert um.last_launch_kernel() == "", "a new handle has launched nothing"
        if t.closed:
            um.set_replay_mode(uncore.PU_REPLAY_CLOSED)
        for prog, th in t.threads:
            um.allocCore(prog, th)
        assert uncore.lib().pu_compiled_config(um._handle()) == 2, t.what
        compiler = uncore.lib().pu_compiled_compiler(um._handle())
        assert compiler == 2, (f"{t.what}: pu_compiled_compiler {compiler}, not 2 (hipcc): "
                               "the build-time warm-up did not compile this configuration")
    except BaseException:
        um.close()
        raise
    return um


def _limit(um, replica: int):
    p = um.limit_positions()[replica]
    return None if p == NO_LIMIT else int(p)


def _run_host(t: Trial, kernel: str, monkeypatch) -> None:
    """s0_h0, s0_h1, s3_h1: access_batch in two chunks on one replica."""
    from primesim_amd import uncore
    env = {S0_H0: "0", S0_H1: "2", S3_H1: None}[kernel]
    want = expected(t.index, 0)
    what = f"{t.what} on {kernel}"
    um = _init(t, 1, env, monkeypatch)
    try:
        if kernel == S0_H1:
            um.set_resident(0)       # resident mode takes precedence over the launch (access_batch)
        cuts = host_cuts(t.reqs)
        assert max(b - a for a, b in zip(cuts, cuts[1:])) <= RESIDENT_CAP
        got = np.zeros(len(t.reqs), np.int32)
        limit = None
        for a, b in zip(cuts, cuts[1:]):
            chunk = np.ascontiguousarray(t.reqs[a:b])
            rc = uncore.lib().pu_access_batch(um._handle(), 0, chunk.ctypes.data, b - a, got[a:b].ctypes.data)
            assert um.last_launch_kernel() == kernel, f"{what}, requests [{a}, {b})"
            if rc == PU_ESTATE:      # an engine limit: its position is an index into this call's requests
                p = _limit(um, 0)
                assert p is not None and p < b - a, f"{what}, requests [{a}, {b}): {uncore.last_error()}, position {p}"
                limit = a + p
                break
            assert rc == 0, f"{what}, requests [{a}, {b}): {uncore.last_error()} ({rc})"
        _check_replica(um, 0, got, limit, want, what)
    finally:
        um.close()


def _run_device(t: Trial, kernel: str, monkeypatch) -> None:
    """s1_h0, s1_h1, s2_h0: three replicas of unequal length from device
    buffers, time-sliced until every replica reaches its end."""
    import torch
    env = {S1_H0: "0", S1_H1: None, S2_H0: None}[kernel]
    h = second_half_start(t.reqs)
    starts = [0, h, 0]
    streams = [t.reqs[s:] for s in starts]
    R = len(streams)
    assert R == REPLICAS
    wants = [expected(t.index, s) for s in starts]
    what = f"{t.what} on {kernel}"
    off = np.zeros(R + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in streams])
    budget = KM.slice_budget_us(min(len(s) for s in streams))

    um = _init(t, R, env, monkeypatch)
    try:
        dev = torch.device("cuda", 0)
        d_reqs = torch.from_numpy(np.concatenate(streams).view(np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_pos = torch.from_numpy(off[:-1].copy().view(np.int64)).to(dev)
        d_del = torch.full((int(off[-1]),), -7, dtype=torch.int32, device=dev)
        d_sched = torch.zeros(um.pool_words(POOL_SLOTS), dtype=torch.int32, device=dev) if kernel == S2_H0 else None
        s = torch.cuda.Stream(dev)
        pos = off[:-1].copy()
        limits = [None] * R      # per replica: the first limit position a launch reported, in its own stream
        launches = 0
        while not np.array_equal(pos, off[1:]):
            if d_sched is not None:
                um.run_device_pool(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(),
                                   d_sched.data_ptr(), POOL_SLOTS, budget, s.cuda_stream)
            else:
                um.run_device_sliced(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(), budget,
                                     s.cuda_stream)
            assert um.last_launch_kernel() == kernel, f"{what}, launch {launches}"
            torch.cuda.synchronize(dev)
            launches += 1
            new = d_pos.cpu().numpy().view(np.uint64)
            assert np.all(new >= pos) and np.all(new <= off[1:]), f"{what}, launch {launches}: {pos} -> {new}"
            # a limit position belongs to the launch that met it (an index into
            # the launch's request array): read after every launch, for the
            # replicas that launch advanced (a pool replica no wavefront has
            # taken yet has no run state of a launch to report), the first kept
            for r, p in enumerate(um.limit_positions()):
                if new[r] > pos[r] and p != NO_LIMIT and limits[r] is None:
                    assert off[r] <= p < off[r + 1], f"{what}, launch {launches}: replica {r} limit position {p}"
                    limits[r] = int(p - off[r])
            pos = new.copy()
            assert launches < LAUNCH_CAP, f"{what}: the replicas did not finish: {pos} of {off[1:]}"
        if d_sched is not None:
            sched = d_sched.cpu().numpy().view(np.uint32)
            assert sched[0] >= R and np.all(sched[2:2 + POOL_SLOTS] == 0), what   # every replica taken, every slot idle
        got = d_del.cpu().numpy()
        for r in range(R):
            _check_replica(um, r, got[int(off[r]):int(off[r + 1])], limits[r], wants[r], what)
    finally:
        um.close()


def run_cell(i: int, kernel: str, monkeypatch) -> None:
    t = trial(i)
    if kernel in (S0_H0, S0_H1, S3_H1):
        _run_host(t, kernel, monkeypatch)
    else:
        assert kernel in (S1_H0, S1_H1, S2_H0)
        _run_device(t, kernel, monkeypatch)
