"""The seeded sweep's 64 configurations through every engine kernel (sweep_matrix.py).

tests/test_config_sweep_oracle.py holds the CPU restatement equal to the
reference on these draws, on the CPU; the goldens and the golden x kernel
matrix tie the engine's kernels to chosen configurations only.  Here each
(trial, kernel) cell runs the trial's stream on that kernel, proven by
pu_last_launch_kernel after every launch, on code objects the build-time
warm-up compiled (pu_compiled_compiler), and checks every delay, completion
cycle, counter, error flag and the request count against a cold run of the
restatement, with equality and no tolerance.  On a trial the restatement
leaves at a reference-undefined flag, the engine must raise the same flags at
the same request and agree on every delay before it.  The share of such trials
is bounded when the file is collected, from the restatement alone; no cell is
left out and none skips."""
import pytest

import sweep_matrix as SM

pytestmark = pytest.mark.gpu

SM.check_cap()


@pytest.mark.parametrize("trial,kernel", SM.cells(),
                         ids=lambda v: v.replace("pu_jit_uncore_", "") if isinstance(v, str) else f"sweep{v:02d}")
def test_sweep_trial_on_kernel(trial, kernel, monkeypatch):
    SM.run_cell(trial, kernel, monkeypatch)
