"""A seeded sweep of small random configurations: the CPU restatement
(oracle/cpu_ref.cpp) against the reference's own uncore, on the CPU.

The goldens pin chosen points of the configuration space; this draws 64 more
from one fixed seed across every axis pu::config_geometry accepts (cores,
levels, block size, nested shares, ways, bus or directory, full map or limited
pointer, shared LLC, TLB and page size, 2-D or 3-D mesh, flit widths, router,
link and inject delays, DRAM time, open or closed replay, the six stream kinds,
write shares, message sizes; tests/config_sweep.py).  Each trial runs in a
child process of its own, at most 8 at a time, because the reference can crash
where it is undefined.  A trial on which the restatement raises a
reference-undefined flag counts as "undefined" and the reference is not run;
on every other trial each delay, the return code and the completion cycles
must be equal.  The engine's six kernels run the same draws against the
restatement on the GPU (tests/test_gpu_config_sweep.py).

The share of undefined trials is bounded at 30 %: a 96-trial run of the same
axes had 13 of the 83 trials the reference survived undefined (16 %), so a
sweep that mostly stops at the flag would check nothing.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as O
import config_sweep as CS
from config_sweep import SEED, TRIALS

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.skipif(not O.ref_available(), reason="the reference's uncore is not compiled here")


def _child(path: str) -> tuple:
    r = subprocess.run([sys.executable, os.path.join(HERE, "config_sweep.py"), path], capture_output=True, text=True,
                       timeout=300)
    return r.returncode, r.stdout, r.stderr


def test_restatement_equals_reference_on_random_small_configurations(tmp_path):
    trials = []
    for i, (sim, spec, replay, redraws) in enumerate(CS.trials()):
        path = str(tmp_path / f"trial{i:02d}")
        CS.write_trial(path, sim, spec, replay)
        trials.append((path, sim, spec, replay, redraws))
    with ThreadPoolExecutor(8) as ex:
        results = list(ex.map(_child, [t[0] for t in trials]))

    signalled, differs, undefined, equal, requests = [], [], 0, 0, 0
    for i, ((path, sim, spec, replay, _), (rc, out, err)) in enumerate(zip(trials, results)):
        what = CS.what(i, sim, spec, replay)
        if rc < 0:
            signalled.append(f"{what}: the child died of signal {-rc}")
            continue
        assert rc == 0, f"{what}: the child failed\n{err}"
        res = json.loads(out.strip().splitlines()[-1])
        requests += res["requests"]
        if res["status"] == "undefined":
            undefined += 1
        elif res["status"] == "equal":
            equal += 1
        else:
            differs.append(f"{what}: {res}")
    print(f"config sweep, seed {SEED}: {TRIALS} trials, {equal} equal, {undefined} undefined, {len(differs)} differ, "
          f"{len(signalled)} died of a signal; {requests} requests; {sum(t[4] for t in trials)} share redraws")
    assert not signalled, "\n".join(signalled)
    assert not differs, "\n".join(differs)
    assert undefined <= 0.30 * TRIALS, f"{undefined} of {TRIALS} trials stopped at a reference-undefined flag"
    assert equal + undefined == TRIALS
