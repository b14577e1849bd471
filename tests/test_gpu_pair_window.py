"""The pair window of the throughput kernels (engine.hip net_transmit): a probe's
forward and back legs in one route window, bit-exact against the oracle.

Every delay, every core's completion cycle, every counter and (where the
reference build is present) the report text, with equality and no tolerance.
The throughput kernels are forced (PRIMEUNCORE_LDS_HEADERS=0: a lone replica
otherwise gets the latency kernel, which keeps the one-route window).  The
shapes are those of pair_window_cases.py."""
import numpy as np
import pytest

import oracle as O
import primesim_amd as P
from pair_window_cases import CASES, sim_dict, stream_spec
from primesim_amd import config as CF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_pair_window_matches_oracle(name, monkeypatch, tmp_path):
    closed = CASES[name][4]
    sim = sim_dict(name)
    cfg = P.config_from_dict(sim)
    spec = stream_spec(name)
    reqs = P.generate_stream(spec)
    assert len(reqs) == CASES[name][3]
    assert (reqs["mem_type"] != reqs["mem_type"][0]).mean() > 0.2     # reads and writes mixed

    cpu = O.CpuRef(cfg)
    ref = O.RefUncore(CF.write_xml(sim, str(tmp_path / "cfg.xml"))) if O.ref_available() else None
    monkeypatch.setenv("PRIMEUNCORE_LDS_HEADERS", "0")
    um = P.UncoreManager()
    um.init(cfg, replicas=1)
    monkeypatch.delenv("PRIMEUNCORE_LDS_HEADERS")
    try:
        if closed:
            cpu.set_mode(O.MODE_CLOSED)
            if ref:
                ref.set_mode(O.MODE_CLOSED)
            um.set_replay_mode(P.uncore.PU_REPLAY_CLOSED)
        for prog, th in P.stream_threads(spec):
            core = um.allocCore(prog, th)
            assert cpu.alloc_core(prog, th) == core
            if ref:
                assert ref.alloc_core(prog, th) == core
        want, rc = cpu.run(reqs)
        assert rc == 0
        if ref:                                   # the restatement against the reference itself
            want_ref, rc = ref.run(reqs)
            assert rc == 0
            np.testing.assert_array_equal(want, want_ref)
        got = um.access_batch(reqs)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(um.completion(), cpu.completion())
        gs, ws = um.stats().as_dict(), cpu.stats().as_dict()
        assert gs["error_flags"] == 0
        assert gs.keys() == ws.keys()
        bad = {k: (gs[k], ws[k]) for k in ws if gs[k] != ws[k]}    # every pu_stats field
        assert not bad, f"{name}: counters differ (engine, oracle): {bad}"
        assert ws["lockdown_calls"] > len(reqs) // 20       # the stream does probe
        if name == "limited_8x8":
            assert ws["total_num_broadcast"] > 0            # ... and broadcasts
        if ref:
            np.testing.assert_array_equal(um.completion(), ref.completion())
            assert um.report() == ref.report()
    finally:
        um.close()
