"""mg1_wait's two paths on the GPU (pu_unit_mg1_path_run).

2^16 queue states from the three sources of tests/test_mg1_guard_rule.py (the
project's families, rho near 1 on both sides, newest - sum in -4..4) go
through the engine's guarded M/G/1 wait, one state per lane; the hook also
says which states the guard accepted (the one-division closed form) and
which ran the reference's five-division chain.  Every wait equals the
reference's, both paths occur, the states on the boundaries (exact-integer
waits, |newest - sum| <= 2) all took the chain, and the guard accepts the
ordinary states (the random family's floor of the CPU rule test).
"""
import numpy as np
import pytest

import mg1_guard as G
import oracle as O
from primesim_amd import uncore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    (n, s, q, w), where = G.sources(36_000, 14_768, 14_768, seed=23)
    assert len(n) == 1 << 16
    out = np.zeros(len(n), dtype=np.uint64)
    path = np.full(len(n), 255, dtype=np.uint8)
    rc = uncore.lib().pu_unit_mg1_path_run(n.ctypes.data, s.ctypes.data, q.ctypes.data, w.ctypes.data, len(n),
                                           out.ctypes.data, path.ctypes.data, 0)
    assert rc == 0, uncore.last_error()
    want = O.ref_mg1(n, s, q, w) if O.ref_available() else O.cpuref_mg1(n, s, q, w)
    return {"st": (n, s, q, w), "where": where, "got": out, "path": path, "want": want}


def test_waits_equal_the_reference_on_both_paths(run):
    n, s, q, w = run["st"]
    got, want, path = run["got"], run["want"], run["path"]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{len(bad)} of {len(n)} states differ; first: n={n[bad[0]]} sum={s[bad[0]]!r} "
                           f"sum_sq={q[bad[0]]!r} newest={w[bad[0]]} engine={got[bad[0]]} reference={want[bad[0]]} "
                           f"path={path[bad[0]]}")
    assert set(np.unique(path)) == {0, 1}


def test_boundary_states_take_the_chain_and_ordinary_ones_the_guard(run):
    n, s, q, w = run["st"]
    path, where = run["path"], run["where"]
    share = {f: float((path[sl] == 1).mean()) for f, sl in where.items()}
    print("accepted share:", {f: round(v, 4) for f, v in share.items()})
    assert not path[where["integer"]].any()
    close = np.abs(w.astype(np.float64) - s) <= 2.0
    assert close.sum() > 5_000 and not path[close].any()
    assert share["random"] >= 0.99, share
