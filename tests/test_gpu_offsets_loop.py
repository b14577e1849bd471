"""The throughput kernels' 32-bit replica offsets and their request loop
(engine.hip PU_OFF32, replica_steps), bit-exact: equality everywhere, no tolerance.

* Offsets: four goldens whose address forms differ, each on the default build
  and on the 64-bit build (PRIMEUNCORE_JIT_EXTRA=-DPU_OFF32=0), against the
  fixture in delays, completion cycles, every counter, error flags and report.
* Loop: the plain path and the general path (closed loop) of the request loop
  hand the loop state in LDS and in the replica's run state to each other,
  across launches that cut inside a message, against the CPU restatement
  driven through the same calls; and prime.cpp's halt (130-134) on the plain
  path through time-sliced launches, with 32-B and with 16-B records.

One replica throughout; the throughput kernels are forced with
PRIMEUNCORE_LDS_HEADERS=0 (a lone replica otherwise gets the latency kernels).
"""
import numpy as np
import pytest

import kernel_matrix as KM
import oracle as O
import primesim_amd as P
from golden_util import extended_stream
from offsets_loop_cases import HALT_GOLDEN, HALT_REQUESTS, JIT_EXTRA_OFF64, LOOP_GOLDEN, OFFSET_GOLDENS
from primesim_amd import _abi as A
from primesim_amd import uncore as U

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("build", ["off32", "off64"])
@pytest.mark.parametrize("golden", OFFSET_GOLDENS)
def test_offsets_match_golden(golden, build, monkeypatch):
    """kernel_matrix's host cell of pu_jit_uncore_s0_h0: the golden in three
    access_batch calls, the kernel named after each, everything against the fixture."""
    if build == "off64":
        monkeypatch.setenv("PRIMEUNCORE_JIT_EXTRA", JIT_EXTRA_OFF64)
    else:
        monkeypatch.delenv("PRIMEUNCORE_JIT_EXTRA", raising=False)
    KM.run_cell(golden, KM.S0_H0, monkeypatch)


def _throughput_handle(cfg, threads, monkeypatch):
    monkeypatch.delenv("PRIMEUNCORE_JIT_EXTRA", raising=False)
    monkeypatch.delenv("PRIMEUNCORE_RESIDENT", raising=False)
    monkeypatch.setenv("PRIMEUNCORE_LDS_HEADERS", "0")
    um = P.UncoreManager()
    um.init(cfg, replicas=1)
    monkeypatch.delenv("PRIMEUNCORE_LDS_HEADERS")
    try:
        for prog, th in threads:
            um.allocCore(prog, th)
    except BaseException:
        um.close()
        raise
    return um


def test_loop_paths_hand_over_across_launches(monkeypatch):
    c = KM.case(LOOP_GOLDEN)
    cfg = P.load_config(c.xml_path)
    cuts = KM.host_cuts(c.reqs)
    assert len(cuts) == 4 and c.reqs["batch_start"][cuts[1]] == 0      # three launches, the first cut inside a message
    ref = O.CpuRef(cfg)
    for prog, th in c.threads:
        ref.alloc_core(prog, th)
    um = _throughput_handle(cfg, c.threads, monkeypatch)
    OPEN, CLOSED = U.PU_REPLAY_OPEN, U.PU_REPLAY_CLOSED
    # the stream four times on the same state: plain, closed loop, plain, and
    # once with the middle launch alone closed loop (the paths change inside a message)
    passes = [("plain", (OPEN, OPEN, OPEN)), ("closed", (CLOSED, CLOSED, CLOSED)), ("plain again", (OPEN, OPEN, OPEN)),
              ("closed inside a message", (OPEN, CLOSED, OPEN))]
    try:
        for p, (name, modes) in enumerate(passes):
            for k, mode in enumerate(modes):
                a, b = cuts[k], cuts[k + 1]
                um.set_replay_mode(mode)
                ref.set_mode(O.MODE_CLOSED if mode == CLOSED else 0)
                got = um.access_batch(c.reqs[a:b])
                assert um.last_launch_kernel() == KM.S0_H0
                want, rc = ref.run(c.reqs[a:b])
                assert rc == 0
                np.testing.assert_array_equal(got, want, err_msg=f"{name}, launch {k}")
                np.testing.assert_array_equal(um.completion(), ref.completion(), err_msg=f"{name}, launch {k}")
            gs, ws = um.stats().as_dict(), ref.stats().as_dict()
            assert gs.keys() == ws.keys()
            bad = {k: (gs[k], ws[k]) for k in ws if k != "requests" and gs[k] != ws[k]}
            assert not bad, f"{name}: counters differ (engine, CPU restatement): {bad}"
            assert gs["error_flags"] == 0
            assert gs["requests"] == (p + 1) * len(c.reqs)     # every request of every launch so far was run
    finally:
        um.close()


_HALT = {}


def _halt_reference():
    """The halting stream and the CPU restatement's run of it, once for both record formats."""
    if not _HALT:
        c = KM.case(HALT_GOLDEN)
        reqs = extended_stream(c, HALT_REQUESTS)
        ref = O.CpuRef(P.load_config(c.xml_path))
        for prog, th in c.threads:
            ref.alloc_core(prog, th)
        want, rc = ref.run(reqs)
        halt = c.meta["halt_index"]
        assert rc == halt + 1 and halt + 1 < len(reqs)
        np.testing.assert_array_equal(want[:len(c.delays)], c.delays)      # ... which is the reference's
        assert (want[halt + 1:] == 0).all()
        for a in (reqs, want):
            a.setflags(write=False)
        _HALT.update(c=c, reqs=reqs, want=want, halt=halt, completion=ref.completion(), stats=ref.stats().as_dict())
    return _HALT


@pytest.mark.parametrize("fmt", [U.PU_REQ_FMT_32, U.PU_REQ_FMT_16], ids=["req32", "req16"])
def test_plain_path_halts_in_sliced_launches(fmt, monkeypatch):
    import torch
    h = _halt_reference()
    c, reqs, want, halt = h["c"], h["reqs"], h["want"], h["halt"]
    n = len(reqs)
    um = _throughput_handle(P.load_config(c.xml_path), c.threads, monkeypatch)
    try:
        um.set_device_req_format(fmt)
        dev = torch.device("cuda", 0)
        rec = reqs if fmt == U.PU_REQ_FMT_32 else U.pack_req16(reqs)
        d_reqs = torch.from_numpy(np.ascontiguousarray(rec).reshape(-1).view(np.uint8).copy()).to(dev)
        off = np.array([0, n], np.uint64)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_pos = torch.from_numpy(off[:-1].copy().view(np.int64)).to(dev)
        d_del = torch.full((n,), -7, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        # a lone wavefront runs a request in about 6 us: 3-ms slices stop and
        # resume the replica dozens of times before the halt
        launches, pos = 0, 0
        while pos < n:
            um.run_device_sliced(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), d_pos.data_ptr(), 3000,
                                 s.cuda_stream)
            assert um.last_launch_kernel() == KM.S1_H0
            torch.cuda.synchronize(dev)
            launches += 1
            new = int(d_pos.cpu().numpy().view(np.uint64)[0])
            # a slice ends before a request it did not run; the halt ends the range
            assert pos <= new <= halt or new == n
            pos = new
            assert launches < 5000, f"the replica did not finish: {pos} of {n}"
        assert launches >= 3, "the stream was meant to be stopped and resumed"
        got = d_del.cpu().numpy()
        np.testing.assert_array_equal(got, want)           # the tail past the halt zero-filled
        st = um.stats().as_dict()
        assert st["error_flags"] == A.PU_ERRF_NEG_DELAY
        assert st["requests"] == halt + 1
        ws = h["stats"]
        bad = {k: (st[k], ws[k]) for k in ws if k != "requests" and st[k] != ws[k]}
        assert not bad, f"counters differ (engine, CPU restatement): {bad}"
        np.testing.assert_array_equal(um.completion(), h["completion"])
    finally:
        um.close()
