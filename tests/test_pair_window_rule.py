"""The pair window's rule (engine.hip net_transmit): under X-then-Y(-then-Z)
routing, with one record per undirected edge, the routes a -> b and b -> a
share a link exactly when the route is a straight line, that is when exactly
one of hx, hy, hz is non-zero.  Brute force over small meshes, no GPU."""
import itertools

import pytest


def route_links(a, b):
    """Undirected edges of the route from a to b: x first (at a's y, z), then y
    (at b's x, a's z), then z (at b's x, y)."""
    cur, out = list(a), set()
    for axis in range(len(a)):
        while cur[axis] != b[axis]:
            nxt = list(cur)
            nxt[axis] += 1 if b[axis] > cur[axis] else -1
            out.add(frozenset((tuple(cur), tuple(nxt))))
            cur = nxt
    return out


@pytest.mark.parametrize("dims", [(w, w) for w in range(2, 7)] + [(3, 3, 3)])
def test_routes_there_and_back_share_a_link_only_on_a_straight_line(dims):
    nodes = list(itertools.product(*[range(w) for w in dims]))
    pairs = 0
    for a, b in itertools.permutations(nodes, 2):
        there, back = route_links(a, b), route_links(b, a)
        hops = sum(abs(x - y) for x, y in zip(a, b))
        assert len(there) == len(back) == hops
        straight = sum(x != y for x, y in zip(a, b)) == 1
        assert bool(there & back) == straight, (a, b)
        if straight:
            assert there == back
        pairs += 1
    assert pairs == len(nodes) * (len(nodes) - 1)
