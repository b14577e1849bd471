"""The sweep x kernel matrix's table (sweep_matrix.py, config_sweep.py), checked
without a GPU: the build-time warm-up compiles every sweep configuration, the
draws are the same on every call, the GPU file runs every (trial, kernel) pair
with none left out, and the driver's cuts fit these short streams."""
import json
import os
import subprocess
import sys

import numpy as np

import config_sweep as CS
import kernel_matrix as KM
import sweep_matrix as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warm_up_compiles_every_sweep_configuration():
    # the tool is asked in a child process: importing it sets PRIMEUNCORE_JIT_OFFLINE
    # and the module search path for the whole process
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import jit_warm; "
            "print(json.dumps([(n, bytes(c).hex()) for n, c, extra in jit_warm.configs() if extra == '']))")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tools")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    warmed = {(n, bytes.fromhex(b)) for n, b in json.loads(r.stdout.strip().splitlines()[-1])}
    sweep = [(n, bytes(c)) for n, c in CS.sweep_configs()]
    assert [n for n, _ in sweep] == [f"sweep {i:02d}" for i in range(CS.TRIALS)]
    assert not [n for n, b in sweep if (n, b) not in warmed]
    # and they are the configurations the GPU cells create their handles on
    assert [b for _, b in sweep] == [bytes(SM.trial(i).cfg) for i in range(CS.TRIALS)]


def test_trials_are_the_same_on_every_call():
    import primesim_amd as P
    a, b = CS.trials(), CS.trials()
    assert len(a) == len(b) == CS.TRIALS == 64 and CS.SEED == 20260
    for i, ((sim0, spec0, replay0, _), (sim1, spec1, replay1, _)) in enumerate(zip(a, b)):
        assert (sim0, spec0, replay0) == (sim1, spec1, replay1), i
        assert bytes(P.config_from_dict(sim0)) == bytes(P.config_from_dict(sim1)), i
        r0, r1 = P.generate_stream(P.StreamSpec(**spec0)), P.generate_stream(P.StreamSpec(**spec1))
        assert r0.tobytes() == r1.tobytes() == SM.trial(i).reqs.tobytes(), i


def test_gpu_file_runs_every_trial_on_every_kernel():
    import test_gpu_config_sweep as T
    marks = [m for m in T.test_sweep_trial_on_kernel.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "trial,kernel"
    got = list(marks[0].args[1])
    every = [(i, k) for i in range(CS.TRIALS) for k in KM.KERNELS]
    assert got == every == SM.cells() and len(got) == len(set(got)) == CS.TRIALS * 6 == 384
    assert T.pytestmark.name == "gpu"
    assert not hasattr(SM, "EXCLUDED")
    # no exclusion is justified: every sweep mesh is far under the LDS header image's 3,400 queues
    assert max(SM.trial(i).cfg.sys.num_cores for i in range(CS.TRIALS)) <= 70


def test_flagged_trials_stay_under_the_cap():
    """From the restatement alone: the trials on which the GPU file compares a
    prefix only.  (The CPU sweep holds the same bound where the reference is built.)"""
    flagged = SM.flagged_trials()
    assert len(flagged) <= 0.30 * CS.TRIALS
    SM.check_cap()
    for i in flagged:
        e = SM.expected(i, 0)
        assert 0 <= e.limit_at < len(e.delays) and e.rc == 0


def test_cuts_fit_every_stream():
    """Every stream gets one or two host chunks that tile it, under the resident
    command size, the cut inside a message where the stream has one after the
    middle; replica 1 starts at a message start in the second half, or at 0."""
    for i in range(CS.TRIALS):
        reqs = SM.trial(i).reqs
        n = len(reqs)
        assert 1 <= n <= 4000 < KM.RESIDENT_CAP
        cuts = SM.host_cuts(reqs)
        assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:]))
        assert len(cuts) == (3 if n >= 2 else 2)
        if len(cuts) == 3:
            c = cuts[1]
            assert c >= n // 2
            inside = np.nonzero(reqs["batch_start"][n // 2:] == 0)[0]
            assert (reqs["batch_start"][c] == 0 and c == n // 2 + inside[0]) if len(inside) else c == n // 2
        h = SM.second_half_start(reqs)
        assert reqs["batch_start"][h] == 1
        later = np.nonzero(reqs["batch_start"][n // 2:])[0]
        assert h == (n // 2 + later[0] if len(later) else 0)
