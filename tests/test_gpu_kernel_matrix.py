"""Every golden configuration through every engine kernel (kernel_matrix.py).

test_gpu_golden.py runs each golden on the one kernel the default path gives
it.  Here each (golden, kernel) cell runs the golden on that kernel, proven by
pu_last_launch_kernel after every launch, and checks every delay, completion
cycle, counter, error flag, the request count and the report text against the
reference's own outputs, with equality and no tolerance.  The six cells that
cannot exist (headers that do not fit the LDS image) are the literal table
kernel_matrix.EXCLUDED; no cell skips."""
import pytest

import kernel_matrix as KM

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("golden,kernel", KM.cells(), ids=lambda v: v.replace("pu_jit_uncore_", ""))
def test_golden_on_kernel(golden, kernel, monkeypatch):
    KM.run_cell(golden, kernel, monkeypatch)
