"""tools/ensemble_summary.py --msglog: one recorded message log replayed across replicas
under seeded placements (DeviceTraceSet in the place of DeviceStreamSet).  The golden
c1_stream is written as a message log; replica 0 runs it as recorded whatever the
placement seed, and replicas 1 - 2 agree with a host restatement of the same placement:
place_trace, then oracle.CpuRef, then summarize_delays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import primesim_amd as P
from abi_helpers import ROOT
from golden_util import Case

pytestmark = pytest.mark.gpu

R, CHUNK, CHUNKS, SEED = 3, 500, 2, 5


def _tool(c, log, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ensemble_summary.py"), "--xml", c.xml_path, "--msglog", str(log),
           "--replicas", str(R), "--chunk", str(CHUNK), "--chunks", str(CHUNKS), "--quantiles", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(lines) == R + 1 and [l["replica"] for l in lines[:R]] == list(range(R))
    return lines


def _log(tmp_path):
    """c1_stream as a message log: (case, path, the requests msglog_read replays from it)."""
    c = Case("c1_stream")
    spec = P.StreamSpec(**c.meta["stream"])
    log = tmp_path / "c1_stream.msglog"
    P.msglog_from_stream(str(log), np.ascontiguousarray(c.reqs), spec)
    trace = P.msglog_read(str(log), num_cores=spec.num_cores)
    n = CHUNK * CHUNKS
    assert len(trace) >= n and trace[:n].tobytes() == np.ascontiguousarray(c.reqs[:n]).tobytes()
    return c, spec, log, trace


def test_warm_up_forks_the_replicas_and_all_continue_from_one_position(tmp_path):
    """--warmup-chunks 1 --chunks 1: replica 0 alone runs the log's first chunk and is forked; every replica's
    line is then the second chunk's summary on a replica that has seen the first."""
    c, spec, log, trace = _log(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ensemble_summary.py"), "--xml", c.xml_path, "--msglog", str(log),
           "--replicas", str(R), "--chunk", str(CHUNK), "--chunks", "1", "--warmup-chunks", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(lines) == R and all(l == {**lines[0], "replica": i} for i, l in enumerate(lines))
    ref = O.CpuRef(P.load_config(c.xml_path))
    for prog, th in c.threads:
        ref.alloc_core(prog, th)
    assert ref.run(trace[:CHUNK])[1] == 0
    d, rc = ref.run(trace[CHUNK:2 * CHUNK])
    assert rc == 0
    ref.close()
    s, _, _ = P.summarize_delays(np.ascontiguousarray(trace[CHUNK:2 * CHUNK]), d)
    assert lines[0]["requests"] == CHUNK and lines[0]["error_flags"] == 0
    for k, name in enumerate(("read", "write")):
        assert (lines[0][name]["count"], lines[0][name]["sum"]) == (int(s["cls"][k]["count"]), int(s["cls"][k]["sum"]))


def test_message_log_under_seeded_placements(tmp_path):
    c, spec, log, trace = _log(tmp_path)
    n = CHUNK * CHUNKS

    placed = _tool(c, log, "--placement-seed", str(SEED))
    plain = _tool(c, log)
    assert placed[0] == plain[0]                                   # replica 0 runs the trace as recorded
    assert all(l["placement_seed"] == 0 for l in plain[:R]) and plain[1] == {**plain[0], "replica": 1}
    assert [l["placement_seed"] for l in placed[:R]] == [P.placement_seed(SEED, r) for r in range(R)]

    cfg = P.load_config(c.xml_path)
    rows = P.random_placements(R, spec.num_cores, SEED)
    for r in range(R):
        reqs = P.place_trace(trace[:n], rows[r])
        ref = O.CpuRef(cfg)
        for prog, th in c.threads:
            ref.alloc_core(prog, th)
        delays = []
        for k in range(CHUNKS):                                    # the tool's launches, chunk by chunk
            d, rc = ref.run(reqs[k * CHUNK:(k + 1) * CHUNK])
            assert rc == 0
            delays.append(d)
        ref.close()
        s, _, _ = P.summarize_delays(reqs, np.concatenate(delays))
        line = placed[r]
        assert line["requests"] == n and line["error_flags"] == 0 and line["core_out_of_range"] == 0
        for k, name in enumerate(("read", "write")):
            assert line[name]["count"] == int(s["cls"][k]["count"]) and line[name]["sum"] == int(s["cls"][k]["sum"]), (r, name)
            assert line[name]["mean"] == int(s["cls"][k]["sum"]) / int(s["cls"][k]["count"])
            assert line[name]["p50"] is not None
    for r in (1, 2):
        assert (placed[r]["read"]["mean"], placed[r]["write"]["mean"]) != (placed[0]["read"]["mean"], placed[0]["write"]["mean"])
