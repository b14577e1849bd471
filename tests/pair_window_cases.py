"""Configurations and streams of tests/test_gpu_pair_window.py (tools/jit_warm.py
compiles the configurations ahead of the GPU run).

Each shape is the smallest that reaches a distinct path of the pair window
(engine.hip net_transmit): a probe's two legs run in one window when both fit
64 lanes (2 h <= 64) and the route is no straight line, else as two windows."""
from __future__ import annotations

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import config as CF

# name -> (preset, overrides, stream kind, requests, closed loop)
CASES = {
    # 2x2: most pairs are straight lines; fallback and pair mixed at h <= 2
    "mesh_2x2": ("C1", dict(num_cores=4), A.PU_STREAM_UNIFORM_HOTSPOT, 4000, False),
    # 4x4 and 8x8: every pair that is no straight line fits
    "mesh_4x4": ("C1", dict(num_cores=16), A.PU_STREAM_UNIFORM_HOTSPOT, 6000, False),
    "mesh_8x8": ("C1", dict(num_cores=64), A.PU_STREAM_SHARED_UNIFORM, 8000, False),
    # 20x20: h reaches 38; 0.3% of pairs exceed 32 hops (about 60 probes here)
    "mesh_20x20": ("C1", dict(num_cores=400), A.PU_STREAM_SHARED_UNIFORM, 20000, False),
    # 4x4x4: the straight-line rule in three dimensions
    "mesh_4x4x4": ("C1", dict(num_cores=64, net_type=1), A.PU_STREAM_SHARED_UNIFORM, 8000, False),
    # two levels: down recursing through children, evaluated before the forward leg
    "two_level_8x8": ("C3", dict(num_cores=64), A.PU_STREAM_UNIFORM_HOTSPOT, 8000, False),
    # closed loop: tree hops in both legs, staging and shifts
    "closed_8x8": ("C1", dict(num_cores=64), A.PU_STREAM_UNIFORM_HOTSPOT, 8000, True),
    # limited-pointer directory: broadcast probes, many pairs back to back
    "limited_8x8": ("C1", dict(num_cores=64, protocol_type=1, max_num_sharers=2), A.PU_STREAM_UNIFORM_HOTSPOT,
                    6000, False),
}
WRITE_PCT = 30   # at least 25% writes: owner probes, sharer invalidations, share probes


def sim_dict(name: str) -> dict:
    preset, over, _, _, _ = CASES[name]
    return CF.preset(preset, **over)


def stream_spec(name: str) -> P.StreamSpec:
    _, over, kind, n, _ = CASES[name]
    return P.StreamSpec(kind=kind, num_cores=over["num_cores"], seed=23, num_quanta=4, max_requests=n,
                        write_pct=WRITE_PCT)


def pair_window_configs():
    return [(f"pair-window {n}", P.config_from_dict(sim_dict(n))) for n in CASES]
