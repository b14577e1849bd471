"""The guard of the engine's mg1_wait (engine.hip mg1_wait_fast, DESIGN.md §3
"Floating point") restated in numpy, the reference's M/G/1 chain in the same
numpy doubles, and the queue states both guard tests run on
(tests/test_mg1_guard_rule.py, tests/test_gpu_mg1_guard.py).

The twin divides with the plain IEEE f64 division; the device's quotient (one
Newton step and a residual correction) lies within QUOT_ERR = 2^-52 of it, and
the twin adds that to the device's g, so its test holds for either quotient.
"""
import os
import re

import numpy as np

from mg1_states import states

GUARD_C = 64.0            # engine.hip PU_MG1_GUARD_C
DOUBT_REL = 2.0 ** -48    # PU_MG1_DOUBT_REL
DOUBT_ABS = 2.0           # PU_MG1_DOUBT_ABS
U = 2.0 ** -53
QUOT_ERR = 2.0 ** -52   # the device quotient's distance from the correctly rounded one
FAMILIES = ("random", "flat", "overload", "edge", "integer", "small")
ENGINE_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "primesim_amd", "csrc", "engine.hip")


def engine_constants() -> dict:
    """The guard's constants as engine.hip defines them."""
    with open(ENGINE_HIP) as f:
        src = f.read()
    out = {}
    for name in ("PU_MG1_GUARD_C", "PU_MG1_DOUBT_REL", "PU_MG1_DOUBT_ABS"):
        v = re.search(r"#define %s\s+(\S+)" % name, src).group(1)
        out[name] = float.fromhex(v) if v.startswith("0x") else float(v)
    return out


def guard(n, s, q, w):
    """(accepted, ceil of the closed-form wait as f64, clamped) per state."""
    nw = w.astype(np.float64)
    clamp = s >= nw
    gap = nw - s
    den = np.where(clamp, s, gap)
    num = np.where(clamp, 499.5, 0.5) * q
    with np.errstate(all="ignore"):
        wq = num / den
        c = np.ceil(wq)
        g = np.where(clamp, GUARD_C * U * 1000.0, (GUARD_C * U) * (nw / den))
        g = g + QUOT_ERR
        ok = (wq * (1.0 + g) <= c) & (wq * (1.0 - g) > c - 1.0)
        ok &= np.abs(gap) > nw * DOUBT_REL + DOUBT_ABS
        ok &= (q < 2.0 ** 53) & (s < 2.0 ** 53) & (s >= 1.0)
        ok &= (np.trunc(s) == s) & (np.trunc(q) == q)
        ok &= s * s <= (n.astype(np.float64) * q) * (1.0 + 2.0 ** -50)
    ok &= n > 0
    return ok, c, clamp


def chain(n, s, q, w):
    """The reference's chain (queue_model_m_g_1.cpp:26-35) in its operation
    order: (ceil of its wait as f64, its clamp decision)."""
    with np.errstate(all="ignore"):
        nd = n.astype(np.float64)
        mean = s / nd
        var = q / nd - mean * mean
        mu = 1.0 / (s / nd)
        lam = nd / w.astype(np.float64)
        clamp = lam >= mu
        lam = np.where(clamp, 0.999 * mu, lam)
        inv = 1.0 / (mu * mu)
        num = 0.5 * mu
        num = num * lam
        num = num * (inv + var)
        wait = num / (mu - lam)
        return np.ceil(wait), clamp


def _moments(rng, k):
    """n, Σs, Σs² as mg1_states' random family draws them."""
    n = np.exp(rng.uniform(0, np.log(2.0 ** 36), k)).astype(np.uint64) + 1
    nf = n.astype(np.float64)
    P = rng.integers(1, 65, k).astype(np.float64)
    s = np.clip(np.round(nf * (1.0 + rng.random(k) * (P - 1.0))), nf, nf * P)
    lo = np.ceil(s * s / nf)
    q = np.floor(lo + rng.random(k) * (np.maximum(lo, s * P) - lo))
    return n, s, q


def near_one(k, seed):
    """rho = Σs / newest within 2^-40 .. 2^-1 of 1, half on either side."""
    rng = np.random.default_rng(seed)
    n, s, q = _moments(rng, k)
    eps = 2.0 ** -rng.uniform(1.0, 40.0, k) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    w = np.maximum(1.0, np.round(s / (1.0 - eps))).astype(np.uint64)
    return n, s, q, w


def near_equal(k, seed):
    """newest - Σs in -4 .. 4."""
    rng = np.random.default_rng(seed)
    n, s, q = _moments(rng, k)
    w = np.maximum(1, s.astype(np.int64) + rng.integers(-4, 5, k)).astype(np.uint64)
    return n, s, q, w


def sources(n_states, n_near_one, n_near_equal, seed=23):
    """The three sources one after the other; returns the state arrays and, per
    source and family, its slice: {"random": slice, ..., "near_one": slice, "near_equal": slice}."""
    parts = [states(n_states, seed=seed), near_one(n_near_one, seed + 1), near_equal(n_near_equal, seed + 2)]
    k = n_states // 6
    where = {f: slice(i * k, (i + 1) * k if i < 5 else n_states) for i, f in enumerate(FAMILIES)}
    where["near_one"] = slice(n_states, n_states + n_near_one)
    where["near_equal"] = slice(n_states + n_near_one, n_states + n_near_one + n_near_equal)
    n, s, q, w = (np.concatenate([p[i] for p in parts]) for i in range(4))
    return (n.astype(np.uint64), s.astype(np.float64), q.astype(np.float64), w.astype(np.uint64)), where
