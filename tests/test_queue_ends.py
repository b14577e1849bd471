"""pu_config_queue_ends (include/primeuncore.h) against a numpy restatement of the
engine's record numbering: every link record of a configuration is a distinct mesh
edge between neighbours, every edge of the w x w (x w) grid is hit exactly once, the
bus records follow level by level, and an index outside [0, nqueues) names no queue.
Host only: the entry needs no device."""
import math
import os

import numpy as np
import pytest

import primesim_amd as P
from golden_util import GOLDEN
from primesim_amd import config as CF


def _numbering(w: int, three_d: bool) -> dict:
    """record -> (kind, a, b) by the rule of the header comment, over the whole grid."""
    w1, out = w - 1, {}
    if not three_d:
        for y in range(w):
            for x in range(w1):
                out[y * w1 + x] = (0, y * w + x, y * w + x + 1)
        for x in range(w):
            for y in range(w1):
                out[w * w1 + x * w1 + y] = (1, y * w + x, (y + 1) * w + x)
        return out
    blk, w2 = w * w * w1, w * w
    for z in range(w):
        for y in range(w):
            for x in range(w1):
                out[(z * w + y) * w1 + x] = (0, z * w2 + y * w + x, z * w2 + y * w + x + 1)
        for x in range(w):
            for y in range(w1):
                out[blk + (z * w + x) * w1 + y] = (1, z * w2 + y * w + x, z * w2 + (y + 1) * w + x)
    for y in range(w):
        for x in range(w):
            for z in range(w1):
                out[2 * blk + (y * w + x) * w1 + z] = (2, z * w2 + y * w + x, (z + 1) * w2 + y * w + x)
    return out


def _coords(node: int, w: int):
    return np.array([node % w, node // w % w, node // (w * w)])


def _cfg(kind: str, arg):
    if kind == "preset":
        return P.config_from_dict(CF.preset(*arg[:1], **arg[1]))
    return P.load_config(os.path.join(GOLDEN, f"{arg}.xml"))


CASES = [
    ("w2", "preset", ("C1", {"num_cores": 4})),
    ("w4", "preset", ("C1", {})),
    ("w32", "preset", ("C4", {})),
    ("mesh3d", "golden", "mesh3d"),
    ("nonsquare_12", "golden", "nonsquare_12"),
    ("bus_l2_shared", "golden", "bus_l2_shared"),          # a bus system: no links at all
    ("l2_shared_bus", "golden", "l2_shared_bus"),          # links, then buses
]


@pytest.mark.parametrize("name,kind,arg", CASES, ids=[c[0] for c in CASES])
def test_every_record_is_one_edge_and_every_edge_one_record(name, kind, arg):
    cfg = _cfg(kind, arg)
    y = cfg.sys
    three_d = y.network.net_type == 1
    nodes = math.ceil(y.num_cores / y.cache[y.num_levels - 1].share)
    w = math.ceil(round(nodes ** (1 / 3), 9)) if three_d else math.ceil(math.sqrt(nodes))
    want = {} if y.sys_type == 1 or w < 2 else _numbering(w, three_d)
    nlinks = len(want)
    assert nlinks == (0 if y.sys_type == 1 else (w - 1) * w * (3 * w if three_d else 2))
    if name == "w2":
        assert (w, nlinks) == (2, 4)
    if name == "w32":
        assert (w, nlinks) == (32, 1984)
    if name == "mesh3d":
        assert three_d and w == 4 and nlinks == 144
    if name == "nonsquare_12":
        assert nodes == 12 and w == 4 and nlinks == 24   # records for the full 4 x 4 grid
    if name == "bus_l2_shared":
        assert nlinks == 0

    seen = set()
    for q in range(nlinks):
        k, a, b = P.queue_ends(cfg, q)
        assert (k, a, b) == want[q], f"record {q}"
        assert 0 <= a < b < w ** (3 if three_d else 2)
        d = _coords(b, w) - _coords(a, w)
        assert d.sum() == 1 and d[k] == 1 and (d >= 0).all(), f"record {q}: {a} and {b} are not neighbours along {k}"
        seen.add((a, b))
    assert len(seen) == nlinks                             # distinct edges
    n = w ** (3 if three_d else 2)                         # every edge of the grid, by adjacency
    edges = {(v, v + s) for v in range(n) for ax, s in enumerate((1, w, w * w)[:3 if three_d else 2])
             if _coords(v, w)[ax] + 1 < w}
    assert seen == (edges if nlinks else set())

    # the buses: level by level, a cache after the other
    buses = [(l, c) for l in range(y.num_levels) if y.cache[l].share > 1
             for c in range(math.ceil(y.num_cores / y.cache[l].share))]
    for i, (l, c) in enumerate(buses):
        assert P.queue_ends(cfg, nlinks + i) == (3, l, c)
    if name in ("bus_l2_shared", "l2_shared_bus"):
        assert buses
    nq = nlinks + len(buses)
    for q in (-1, -(1 << 31), nq, nq + 1, (1 << 31) - 1):
        assert P.queue_ends(cfg, q) == (-1, -1, -1)
