"""The per-link oracle checks itself on the CPU (tests/link_oracle.py,
tests/cpp/link_visits.cpp): with the trace hook compiled in, the restatement's
delays still equal the fixture's, and its per-link counts add up to the
reference's own counters of the fixture: link visits and link flits.  Every
visited link inverts to an edge between neighbours of the mesh."""
import pytest

import primesim_amd as P
import link_oracle as LO
from golden_util import Case


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LO.load(tmp_path_factory.mktemp("link_oracle"))


@pytest.mark.parametrize("name", ["c1_stream", "nonsquare_12", "mesh3d"])
def test_traced_restatement_equals_the_fixture(oracle, name):
    c = Case(name)
    cfg = P.load_config(c.xml_path)
    t = LO.trace_case(oracle, c, cfg)
    c.check_delays(t.delays)
    assert (t.completion == c.completion).all()
    assert int(t.visits.sum()) == c.counters["link_visits"] == t.stats.net_distance
    assert int(t.flits.sum()) == c.counters["link_flits"] == t.stats.link_flits
    assert sum(v for v, _ in t.edges.values()) == c.counters["link_visits"]
    # a link carries header packets and block packets only: header_flits <= flits / visit <= plen_blk
    net = cfg.sys.network
    blk = cfg.sys.cache[cfg.sys.num_levels - 1].block_size
    plen_blk = net.header_flits + -(-blk // net.data_width)
    w = t.w
    for (a, b), (v, f) in t.edges.items():
        assert a < b and net.header_flits * v <= f <= plen_blk * v, (a, b)
        ca, cb = (a % w, a // w % w, a // (w * w)), (b % w, b // w % w, b // (w * w))
        assert sorted(y - x for x, y in zip(ca, cb)) == [0, 0, 1], f"{a} and {b} are not neighbours"
        assert b < w ** (3 if t.three_d else 2)


@pytest.mark.parametrize("w", [2, 4, 5])
def test_edge_inversion_covers_the_grid_once(w):
    """Every edge of the w x w and w x w x w grids comes from exactly one link index."""
    for three_d, dims in ((False, 2), (True, 3)):
        n = w ** dims
        want = set()
        for v in range(n):
            x, y, z = v % w, v // w % w, v // (w * w)
            for ax, (coord, step) in enumerate(((x, 1), (y, w), (z, w * w))[:dims]):
                if coord + 1 < w:
                    want.add((v, v + step))
        got = {}
        rng = range(w * 2 * w) if not three_d else range(w * w * 3 * w)
        for li in rng:
            e = LO.edge_of(li, w, three_d)
            if e in want:
                assert e not in got, (li, got.get(e))
                got[e] = li
        assert set(got) == want
