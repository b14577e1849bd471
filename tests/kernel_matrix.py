"""The golden x kernel matrix: every golden fixture through every engine kernel.

The engine has six compiled kernels per configuration (jit.cpp):

    pu_jit_uncore_s0_h0   unsliced launch, queue headers in HBM
    pu_jit_uncore_s0_h1   unsliced launch, headers in LDS (latency kernel)
    pu_jit_uncore_s1_h0   pu_run_device_sliced, headers in HBM
    pu_jit_uncore_s1_h1   pu_run_device_sliced, headers in LDS
    pu_jit_uncore_s2_h0   pu_run_device_pool (the benchmark's headline kernel)
    pu_jit_uncore_s3_h1   the resident mailbox kernel

Which one a call gets is decided in uncore.cpp (launch, access_batch) and
resident.cpp (resident_eligible).  `run_cell` drives a golden through the calls that reach one of
them, checks after every launch that pu_last_launch_kernel names that kernel
(a cell that ran another kernel fails), and checks the results against the
fixture with equality: every delay, completion cycle, counter, error flag, the
request count and the report text.

This module holds no test: tests/test_gpu_kernel_matrix.py runs the cells on
the GPU, tests/test_kernel_matrix_table.py checks the table below on the CPU.
"""
from __future__ import annotations

import numpy as np

from golden_util import Case, assert_stats_match, case_names

S0_H0 = "pu_jit_uncore_s0_h0"
S0_H1 = "pu_jit_uncore_s0_h1"
S1_H0 = "pu_jit_uncore_s1_h0"
S1_H1 = "pu_jit_uncore_s1_h1"
S2_H0 = "pu_jit_uncore_s2_h0"
S3_H1 = "pu_jit_uncore_s3_h1"
KERNELS = (S0_H0, S0_H1, S1_H0, S1_H1, S2_H0, S3_H1)

# The only cells left out: configurations whose queue headers cannot fit the
# LDS image of the latency kernels (engine.hip PU_LDS_Q = 3,400 queues), so the
# library has no way to run them with the headers in LDS.  A literal table,
# never computed from the library under test.
_C5 = "64x64 mesh: 8,064 link queues, over the 3,400 of the LDS header image"
_M8 = "8,192 nodes on a 91x91 mesh: 16,380 link queues, over the 3,400 of the LDS header image"
EXCLUDED = {
    ("c5_prodcons", S0_H1): _C5,
    ("c5_prodcons", S1_H1): _C5,
    ("c5_prodcons", S3_H1): _C5,
    ("mesh_8192", S0_H1): _M8,
    ("mesh_8192", S1_H1): _M8,
    ("mesh_8192", S3_H1): _M8,
}

RESIDENT_CAP = 16384      # requests per resident command (resident.cpp kResCap)
REPLICAS = 3              # the device-path cells: replicas 0 and 2 the golden, replica 1 its second half
POOL_SLOTS = 2            # ... on two wavefronts in the pool: one takes the third replica mid-slice


def cells() -> list[tuple[str, str]]:
    """Every (golden, kernel) pair the matrix runs: all but EXCLUDED."""
    return [(g, k) for g in case_names() for k in KERNELS if (g, k) not in EXCLUDED]


def host_cuts(reqs: np.ndarray, max_len: int | None = None) -> list[int]:
    """Chunk bounds [0, ..., n] for access_batch: thirds of the stream, the
    first cut moved forward to a request that does not start a message (so the
    open message's running delay has to carry across calls), and no chunk
    longer than max_len."""
    n = len(reqs)
    mid = np.nonzero(reqs["batch_start"][n // 3:] == 0)[0]
    assert len(mid), "no request inside a message after the first third"
    cuts = {0, n // 3 + int(mid[0]), 2 * n // 3, n}
    out = sorted(cuts)
    if max_len:
        fine = [0]
        for b in out[1:]:
            while b - fine[-1] > max_len:
                fine.append(fine[-1] + max_len)
            fine.append(b)
        out = fine
    assert any(0 < c < n and reqs["batch_start"][c] == 0 for c in out)
    return out


def second_half_start(reqs: np.ndarray) -> int:
    """Replica 1's stream: from the first message that starts in the second half."""
    n = len(reqs)
    starts = np.nonzero(reqs["batch_start"][n // 2:])[0]
    assert len(starts), "no message starts in the second half"
    return n // 2 + int(starts[0])


def slice_budget_us(shortest: int) -> int:
    """The time slice of the device-path cells, from the shortest replica's
    request count.  A request costs a lone wavefront at least 0.5 us (several
    dependent HBM reads; the measured single-instance rate is about 6 us a
    request on C4), so `shortest` requests need more than four slices of
    shortest/8 us: the replica is stopped and resumed at least twice.  Never
    under 50 us, so that a slice always outlasts the launch's start-up (the
    latency kernels copy the header image in first, ~17 us) and every launch
    makes progress."""
    return max(50, shortest // 8)


def _check_fixture_replica(um, c: Case, delays: np.ndarray, replica: int) -> None:
    from primesim_amd import _abi as A
    c.check_delays(delays)
    np.testing.assert_array_equal(um.completion(replica), c.completion)
    st = um.stats(replica).as_dict()
    halt = c.meta.get("halt_index")
    assert st["error_flags"] == (0 if halt is None else A.PU_ERRF_NEG_DELAY)
    assert st["requests"] == (len(c.reqs) if halt is None else halt + 1)
    assert_stats_match(st, c)
    assert um.report(replica) == c.report


def _init(c: Case, replicas: int, lds_headers: str | None, monkeypatch):
    """A handle on the golden's configuration, created under the given
    PRIMEUNCORE_LDS_HEADERS (None: the default environment; pu_create reads it)."""
    import primesim_amd as P
    from primesim_amd import uncore
    monkeypatch.delenv("PRIMEUNCORE_RESIDENT", raising=False)
    if lds_headers is None:
        monkeypatch.delenv("PRIMEUNCORE_LDS_HEADERS", raising=False)
    else:
        monkeypatch.setenv("PRIMEUNCORE_LDS_HEADERS", lds_headers)
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=replicas)
    try:
        assert um.last_launch_kernel() == "", "a new handle has launched nothing"
        assert uncore.lib().pu_compiled_config(um._handle()) == 2
        if c.closed:
            um.set_replay_mode(uncore.PU_REPLAY_CLOSED)
        for prog, th in c.threads:
            um.allocCore(prog, th)
    except BaseException:
        um.close()
        raise
    return um


def _run_host(c: Case, kernel: str, monkeypatch) -> None:
    """s0_h0, s0_h1, s3_h1: access_batch in chunks on one replica."""
    env = {S0_H0: "0", S0_H1: "2", S3_H1: None}[kernel]
    um = _init(c, 1, env, monkeypatch)
    try:
        if kernel == S0_H1:
            um.set_resident(0)       # resident mode takes precedence over the launch (access_batch)
        cuts = host_cuts(c.reqs, RESIDENT_CAP if kernel == S3_H1 else None)
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            parts.append(um.access_batch(c.reqs[a:b]))
            assert um.last_launch_kernel() == kernel, f"requests [{a}, {b})"
        _check_fixture_replica(um, c, np.concatenate(parts), 0)
    finally:
        um.close()


def _run_device(c: Case, kernel: str, monkeypatch) -> None:
    """s1_h0, s1_h1, s2_h0: three replicas of unequal length from device
    buffers, time-sliced so that each is stopped and resumed at least twice."""
    import torch

    import oracle as O
    from primesim_amd import _abi as A
    env = {S1_H0: "0", S1_H1: None, S2_H0: None}[kernel]
    h = second_half_start(c.reqs)
    streams = [c.reqs, c.reqs[h:], c.reqs]
    R = len(streams)
    assert R == REPLICAS
    off = np.zeros(R + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in streams])
    budget = slice_budget_us(min(len(s) for s in streams))

    # replica 1's reference: the CPU restatement from a cold state, in the golden's replay mode
    ref = O.CpuRef(_cfg(c))
    if c.closed:
        ref.set_mode(O.MODE_CLOSED)
    for prog, th in c.threads:
        ref.alloc_core(prog, th)
    want1, rc1 = ref.run(streams[1])
    assert rc1 >= 0

    um = _init(c, R, env, monkeypatch)
    try:
        dev = torch.device("cuda", 0)
        d_reqs = torch.from_numpy(np.concatenate(streams).view(np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_pos = torch.from_numpy(off[:-1].copy().view(np.int64)).to(dev)
        d_del = torch.full((int(off[-1]),), -7, dtype=torch.int32, device=dev)
        d_sched = torch.zeros(um.pool_words(POOL_SLOTS), dtype=torch.int32, device=dev) if kernel == S2_H0 else None
        s = torch.cuda.Stream(dev)
        progressed = np.zeros(R, np.int64)        # launches in which the replica advanced
        pos = off[:-1].copy()
        launches = 0
        while not np.array_equal(pos, off[1:]):
            if d_sched is not None:
                um.run_device_pool(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(),
                                   d_sched.data_ptr(), POOL_SLOTS, budget, s.cuda_stream)
            else:
                um.run_device_sliced(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(), budget,
                                     s.cuda_stream)
            assert um.last_launch_kernel() == kernel, f"launch {launches}"
            torch.cuda.synchronize(dev)
            launches += 1
            new = d_pos.cpu().numpy().view(np.uint64)
            assert np.all(new >= pos) and np.all(new <= off[1:])
            progressed += new > pos
            pos = new.copy()
            assert launches < 20000, f"the replicas did not finish: {pos} of {off[1:]}"
        # progress in three launches or more = stopped and resumed at least twice
        assert np.all(progressed >= 3), f"{budget}-us slices, launches with progress per replica: {progressed}"
        if d_sched is not None:
            sched = d_sched.cpu().numpy().view(np.uint32)
            assert sched[0] >= R and np.all(sched[2:2 + POOL_SLOTS] == 0)   # every replica taken, every slot idle
        got = d_del.cpu().numpy()
        for r in (0, 2):
            _check_fixture_replica(um, c, got[int(off[r]):int(off[r + 1])], r)
        np.testing.assert_array_equal(got[int(off[1]):int(off[2])], want1, err_msg="replica 1")
        gs, ws = um.stats(1).as_dict(), ref.stats().as_dict()
        assert gs.keys() == ws.keys()
        bad = {k: (gs[k], ws[k]) for k in ws if k != "requests" and gs[k] != ws[k]}
        assert not bad, f"{c.name} replica 1: counters differ (engine, CPU restatement): {bad}"
        np.testing.assert_array_equal(um.completion(1), ref.completion())
        if rc1 == 0:
            assert gs["error_flags"] == 0 and gs["requests"] == len(streams[1])
        else:                    # the second half alone also runs into the prime.cpp:130-134 halt
            assert gs["error_flags"] == A.PU_ERRF_NEG_DELAY and gs["requests"] == rc1
    finally:
        um.close()


def _cfg(c: Case):
    import primesim_amd as P
    return P.load_config(c.xml_path)


_CASES: dict[str, Case] = {}


def case(name: str) -> Case:
    """The golden fixture, loaded once and shared (nothing writes to it)."""
    if name not in _CASES:
        c = Case(name)
        for a in (c.reqs, c.delays, c.completion):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def run_cell(golden: str, kernel: str, monkeypatch) -> None:
    assert (golden, kernel) not in EXCLUDED
    c = case(golden)
    if kernel in (S0_H0, S0_H1, S3_H1):
        _run_host(c, kernel, monkeypatch)
    else:
        assert kernel in (S1_H0, S1_H1, S2_H0)
        _run_device(c, kernel, monkeypatch)
