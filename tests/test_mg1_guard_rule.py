"""The guard rule of mg1_wait, on the CPU (DESIGN.md §3 "Floating point").

The engine takes sum_sq / (2 (newest - sum)), or 499.5 sum_sq / sum under the
clamp, for the reference's five-division wait wherever no integer lies within
the derived error band of it and the clamp decision is beyond doubt.  Here a
numpy twin of that guard (tests/mg1_guard.py, the engine's constants) runs on
600,000 states of the project's families, 200,000 with rho within 2^-40..2^-1
of 1 on both sides and 200,000 with newest - sum in -4..4, against the
reference's chain: no accepted state may differ from it in ceil(w) or in the
clamp decision, and the guard must accept the bulk of ordinary states (one
that rejects everything is exact and useless).
"""
import numpy as np
import pytest

import mg1_guard as G
import oracle as O


@pytest.fixture(scope="module")
def run():
    (n, s, q, w), where = G.sources(600_000, 200_000, 200_000, seed=23)
    ok, c, clamp = G.guard(n, s, q, w)
    ref_c, ref_clamp = G.chain(n, s, q, w)
    return {"st": (n, s, q, w), "where": where, "ok": ok, "c": c, "clamp": clamp, "ref_c": ref_c,
            "ref_clamp": ref_clamp}


def test_twin_uses_the_engines_constants():
    k = G.engine_constants()
    assert (k["PU_MG1_GUARD_C"], k["PU_MG1_DOUBT_REL"], k["PU_MG1_DOUBT_ABS"]) == (G.GUARD_C, G.DOUBT_REL, G.DOUBT_ABS)


def test_accepted_states_equal_the_chain(run):
    ok = run["ok"]
    n, s, q, w = run["st"]
    bad = np.nonzero(ok & ((run["c"] != run["ref_c"]) | (run["clamp"] != run["ref_clamp"])))[0]
    assert len(bad) == 0, (f"{len(bad)} accepted states differ; first: n={n[bad[0]]} sum={s[bad[0]]!r} "
                           f"sum_sq={q[bad[0]]!r} newest={w[bad[0]]} guard={run['c'][bad[0]]} "
                           f"chain={run['ref_c'][bad[0]]}")
    # and the compiled restatement's chain (the oracle library) where it is built
    try:
        want = O.cpuref_mg1(n[ok], s[ok], q[ok], w[ok])
    except (OSError, RuntimeError):
        return
    assert np.array_equal(run["c"][ok].astype(np.uint64), want)


def test_guard_accepts_the_ordinary_states(run):
    ok, where = run["ok"], run["where"]
    share = {f: float(ok[sl].mean()) for f, sl in where.items()}
    print("accepted share:", {f: round(v, 4) for f, v in share.items()})
    assert share["random"] >= 0.99 and share["flat"] >= 0.98, share
    # the families on the boundaries take the chain: every exact-integer wait, every near-equal state
    assert share["integer"] == 0.0
    n, s, q, w = run["st"]
    close = np.abs(w.astype(np.float64) - s) <= 2.0
    assert close.sum() > 100_000 and not ok[close].any()
