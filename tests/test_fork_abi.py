"""Forking a replica and its stream, on the host (pu_replica_fork, pu_stream_fork,
pu_dstream_fork; include/primeuncore.h): the entries are exported and typed, refuse
bad arguments before a device is touched, and pu_stream_fork follows the rule of
primesim_amd/csrc/stream_step.h:
  * a clone continues the source's stream byte for byte from any position (7, 100 and
    4,096 records in: the cut core is mid-quantum and mid-message);
  * a reseeded fork at position 0 is the fresh stream of the new seed (a);
  * for the kinds without per-core history (4, 5, 6) core c's k-th record after a
    reseeded fork has the address, type and gap of core c's k-th record of the fresh
    stream, its timer shifted by c's cycle at the fork (b);
  * kinds 1, 2 and 3 keep their history: streaming position and re-use ring;
  * positions and max_requests go on counting (c);
  * a destination of another shape is refused and stays what it was.
The index rules of the engine fork's kernel and the stream rule are checked by
tests/cpp/replica_fork_check.cpp under the host's sanitizers.  A range past a handle
or a device set needs a device to have one: tests/test_gpu_fork.py.

Shapes S1 to S5 are those of tests/test_gpu_dstream.py (restated)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT, run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from primesim_amd.uncore import lib

KINDS = [A.PU_STREAM_PRIVATE_STREAMING, A.PU_STREAM_SHARED_UNIFORM, A.PU_STREAM_MULTIPROGRAM,
         A.PU_STREAM_UNIFORM_HOTSPOT, A.PU_STREAM_PRODUCER_CONSUMER, A.PU_STREAM_UNIFORM]
NO_HISTORY = [A.PU_STREAM_UNIFORM_HOTSPOT, A.PU_STREAM_PRODUCER_CONSUMER, A.PU_STREAM_UNIFORM]
#            cores quantum quanta max_msg progs
SHAPES = {"S1": (48, 200, 3, 9, 2), "S2": (1, 50, 4, 3, 1), "S3": (70, 2, 40, 5, 3),
          "S4": (1030, 40, 2, 100, 4), "S5": (64, 3, 30, 2, 1)}
ADVANCE = [7, 100, 4096]
SEED, NEW_SEED = 7, 1234567


def _spec(kind, shape, seed=SEED, **kw):
    c, q, nq, mm, pr = SHAPES[shape]
    return P.StreamSpec(kind, c, seed=seed, quantum=q, num_quanta=nq, max_msg=mm, num_progs=pr, **kw)


def _take(ss, i, n=1 << 17):
    """Stream i's next up to n records (the set's other streams stay where they are)."""
    out = np.zeros(n, dtype=A.REQ_DTYPE)
    got = lib().pu_stream_next(ss._h[i], out.ctypes.data, n)
    assert got >= 0
    return out[:got]


# ------------------------------------------------------------------ exports and arguments
def test_mirror_declares_every_fork_entry():
    L = lib()
    V = C.c_void_p
    want = {
        "pu_replica_fork": (C.c_int, [V, C.c_int, C.c_int, C.c_int, C.c_int, V]),
        "pu_stream_fork": (C.c_int, [V, V, C.c_int, C.c_uint64]),
        "pu_dstream_fork": (C.c_int, [V, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), V]),
    }
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        header = f.read()
    for name, (res, args) in want.items():
        assert f"{name}(" in header, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert "#define PU_FORK_BY_COPIES 1" in header and A.PU_FORK_BY_COPIES == 1
    for cls, method in ((P.UncoreManager, "fork_replica"), (P.StreamSet, "fork"), (P.DeviceStreamSet, "fork")):
        assert callable(getattr(cls, method))


def test_replica_fork_refuses_bad_arguments_before_a_device():
    L = lib()
    for flags in (2, 3, -1, 1 << 20):
        assert L.pu_replica_fork(None, 0, 0, 1, flags, None) == -22
        assert "unknown flags" in U.last_error()
    for src, first, n in ((-1, 0, 1), (0, -1, 1), (0, 0, -1)):
        assert L.pu_replica_fork(None, src, first, n, 0, None) == -22
        assert "negative argument" in U.last_error()
    for flags in (0, A.PU_FORK_BY_COPIES):
        assert L.pu_replica_fork(None, 0, 0, 1, flags, None) == -22
        assert "no handle" in U.last_error()
    with pytest.raises(P.UncoreError):
        P.UncoreManager().fork_replica(0)


def test_stream_forks_refuse_null_and_negative_arguments():
    L = lib()
    seeds = (C.c_uint64 * 2)(1, 2)
    assert L.pu_dstream_fork(None, 0, 0, 1, seeds, None) == -22
    assert "no set" in U.last_error()
    ss = P.StreamSet([_spec(KINDS[3], "S1")])
    try:
        assert L.pu_stream_fork(None, ss._h[0], 0, 0) == -22
        assert "no stream" in U.last_error()
        assert L.pu_stream_fork(ss._h[0], None, 1, 5) == -22
        assert L.pu_stream_fork(ss._h[0], ss._h[0], 1, 5) == 0           # the source is left as it is
        np.testing.assert_array_equal(_take(ss, 0), P.generate_stream(_spec(KINDS[3], "S1")))
        with pytest.raises(P.UncoreError, match="seeds for a range"):
            ss.fork(0, seeds=[1, 2, 3])
        for bad in (dict(src=1), dict(src=-1), dict(src=0, first=0, n=2), dict(src=0, first=1, n=1), dict(src=0, n=-1)):
            with pytest.raises(P.UncoreError, match="outside the set"):
                ss.fork(**bad)
    finally:
        ss.close()


def test_index_rules_and_stream_rule_under_the_sanitizers(tmp_path):
    """Tile cover at 4,096 / 12,288 / 16,384 / 20,480 / 17 MiB + 4,096 / 2^33 + 4,096 bytes, 2,000
    random destination ranges, 2,000 forked headers."""
    assert run_cpp_check(tmp_path, "replica_fork_check.cpp").startswith("OK 6 sizes 537988864 pieces, 2000 ranges")


# ------------------------------------------------------------------ clone
@pytest.mark.parametrize("adv", ADVANCE)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_clone_continues_the_source_byte_for_byte(kind, shape, adv):
    whole = P.generate_stream(_spec(kind, shape))
    ss = P.StreamSet([_spec(kind, shape), _spec(kind, shape, seed=99)])
    try:
        head, _ = _take(ss, 0, adv), _take(ss, 1, adv)    # both streams advance; stream 1's state is stale
        k = min(adv, len(whole))
        np.testing.assert_array_equal(head, whole[:k])
        ss.fork(0, 1, 1)
        assert ss.position(1) == ss.position(0) == k
        a, b = _take(ss, 0, 5000), _take(ss, 1, 5000)     # a chunk, then the rest
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, whole[k:k + 5000])
        np.testing.assert_array_equal(_take(ss, 1), whole[k + len(a):])
        np.testing.assert_array_equal(_take(ss, 0), whole[k + len(a):])
        assert ss.position(1) == ss.position(0) == len(whole)
    finally:
        ss.close()


# ------------------------------------------------------------------ reseeded
@pytest.mark.parametrize("shape", ["S1", "S3", "S4"])
@pytest.mark.parametrize("kind", KINDS)
def test_reseeded_fork_at_position_zero_is_the_fresh_stream(kind, shape):
    """(a); and the destination's own history (here: 300 records of another seed) is gone."""
    ss = P.StreamSet([_spec(kind, shape), _spec(kind, shape, seed=99)])
    try:
        assert len(_take(ss, 1, 300)) == 300
        ss.fork(0, 1, 1, seeds=[NEW_SEED])
        assert ss.position(1) == 0
        np.testing.assert_array_equal(_take(ss, 1), P.generate_stream(_spec(kind, shape, seed=NEW_SEED)))
        np.testing.assert_array_equal(_take(ss, 0), P.generate_stream(_spec(kind, shape)))   # the source: untouched
    finally:
        ss.close()


def _forked(kind, shape, adv, **kw):
    """(prefix, the unforked source's continuation, the reseeded fork's continuation, the fresh
    stream of the new seed) for a source advanced by adv records."""
    ss = P.StreamSet([_spec(kind, shape, **kw), _spec(kind, shape, seed=99, **kw)])
    try:
        prefix, _ = _take(ss, 0, adv), _take(ss, 1, adv)
        ss.fork(0, 1, 1, seeds=[NEW_SEED])
        assert ss.position(1) == len(prefix)
        return prefix, _take(ss, 0), _take(ss, 1), P.generate_stream(_spec(kind, shape, seed=NEW_SEED, **kw))
    finally:
        ss.close()


def _check_order_and_messages(r, spec):
    """tests/test_stream.py's invariants: quantum-major then core, a message is one core's within one
    quantum and at most max_msg long."""
    q = r["timer"] // spec.quantum
    assert np.all(np.diff(q * spec.num_cores + r["core"]) >= 0)
    starts = np.nonzero(r["batch_start"])[0]
    assert starts[0] == 0
    ends = np.append(starts[1:], len(r))
    assert (ends - starts).max() <= spec.max_msg
    msg = np.cumsum(r["batch_start"]) - 1                  # message index of every record
    for field in (r["core"], q):
        assert np.array_equal(field, field[starts][msg]), "a message is one core's, within one quantum"
    # a message closes only when it is full, or its core or quantum ends
    for a, b in zip(starts[:-1], starts[1:]):
        assert b - a == spec.max_msg or r["core"][b] != r["core"][a] or q[b] != q[a]


@pytest.mark.parametrize("adv", [7, 100, 1000])
@pytest.mark.parametrize("shape", ["S1", "S3", "S4"])
@pytest.mark.parametrize("kind", NO_HISTORY)
def test_reseeded_fork_replays_the_fresh_stream_per_core(kind, shape, adv):
    """(b)"""
    spec = _spec(kind, shape)
    prefix, clone, fork, fresh = _forked(kind, shape, adv)
    assert len(prefix) == adv and len(fork) > 0
    cores = np.unique(fork["core"])
    np.testing.assert_array_equal(cores, np.unique(clone["core"]))
    for c in cores:
        f, w, u = fork[fork["core"] == c], fresh[fresh["core"] == c], clone[clone["core"] == c]
        assert len(w) >= len(f)
        w = w[:len(f)]
        np.testing.assert_array_equal(f["addr"], w["addr"])
        np.testing.assert_array_equal(f["mem_type"], w["mem_type"])
        np.testing.assert_array_equal(f["timer"] - f["timer"][0], w["timer"] - w["timer"][0])
        assert w["timer"][0] == 0 and f["timer"][0] == u["timer"][0]     # the core's cycle at the fork
        assert np.all(f["prog_id"] == u["prog_id"][0])
    _check_order_and_messages(np.concatenate([prefix, fork]), spec)
    for name in ("core", "timer", "batch_start"):             # the cursor: same core, cycle and open message
        assert fork[name][0] == clone[name][0]


def _first_per_core(r):
    cores, idx = np.unique(r["core"], return_index=True)
    return dict(zip(cores.tolist(), r[idx]))


@pytest.mark.parametrize("adv", [100, 4096])
@pytest.mark.parametrize("shape", ["S1", "S4"])
def test_reseeded_fork_keeps_the_streaming_position_of_kind_1(shape, adv):
    """A core's first streaming access after the fork is pos words into its 2-MB region, pos = its
    streaming accesses before the fork; the fresh stream's is word 0.  Table reads are the same."""
    kind = A.PU_STREAM_PRIVATE_STREAMING
    prefix, clone, fork, fresh = _forked(kind, shape, adv)
    streaming = 0x100000000
    moved = 0
    ff, ww = _first_per_core(fork), _first_per_core(fresh)
    for c, f in ff.items():
        w = ww[c]
        pos = int(np.count_nonzero((prefix["core"] == c) & (prefix["addr"] >= streaming)))
        if w["addr"] >= streaming:
            assert int(f["addr"]) - int(w["addr"]) == pos * 8 % (2 << 20)
            moved += pos > 0
        else:
            assert f["addr"] == w["addr"] and f["mem_type"] == A.PU_RD
    assert moved > 0
    _check_order_and_messages(np.concatenate([prefix, fork]), _spec(kind, shape))
    assert fork["batch_start"][0] == clone["batch_start"][0] and fork["core"][0] == clone["core"][0]


@pytest.mark.parametrize("adv", [1000, 4096])           # enough cores with a ring for some to draw a re-use
@pytest.mark.parametrize("shape", ["S1", "S4"])
def test_reseeded_fork_keeps_the_ring_of_kind_2(shape, adv):
    """A fresh stream's first access per core cannot be a re-use (its ring is empty); the fork's is,
    for some cores, and then it is one of the core's last 16 new addresses before the fork."""
    kind = A.PU_STREAM_SHARED_UNIFORM
    prefix, clone, fork, fresh = _forked(kind, shape, adv)
    ff, ww = _first_per_core(fork), _first_per_core(fresh)
    reused = 0
    for c, f in ff.items():
        mine = prefix["addr"][prefix["core"] == c]
        if f["addr"] == ww[c]["addr"]:
            continue
        # new addresses are pushed, re-uses are not: the ring is the last 16 distinct-by-push addresses
        assert len(mine) > 0 and f["addr"] in mine
        reused += 1
    assert reused > 0
    _check_order_and_messages(np.concatenate([prefix, fork]), _spec(kind, shape))
    assert fork["batch_start"][0] == clone["batch_start"][0] and fork["core"][0] == clone["core"][0]


@pytest.mark.parametrize("adv", [100, 4096])
@pytest.mark.parametrize("shape", ["S1", "S4"])
def test_reseeded_fork_keeps_the_streaming_position_of_kind_3(shape, adv):
    """Half of a core's accesses walk its slice of the program's footprint: the walk goes on from
    where the source's stood.  The walk is restated here from stream.cpp's description."""
    kind = A.PU_STREAM_MULTIPROGRAM
    spec = _spec(kind, shape)
    prefix, clone, fork, fresh = _forked(kind, shape, adv)
    base, mb = 0x80000000, 1 << 20
    per = max(spec.num_cores // spec.num_progs, 1)

    def walk(c, prog, pos):
        fp = (4, 16, 32, 64)[(prog - 1) & 3] * mb
        piece = max(fp // per, 64)
        return base + ((c % per) * piece + pos * 8 % piece) % fp

    ff, ww = _first_per_core(fork), _first_per_core(fresh)
    moved = 0
    for c, f in ff.items():
        prog, pos = int(f["prog_id"]), 0
        for a in prefix["addr"][prefix["core"] == c]:      # a uniform draw lands on the walk's next word
            pos += int(a) == walk(c, prog, pos)            # once in 2^19 or less
        if int(ww[c]["addr"]) == walk(c, prog, 0):
            assert int(f["addr"]) == walk(c, prog, pos)
            moved += pos > 0
        else:
            assert f["addr"] == ww[c]["addr"]
    assert moved > 0
    _check_order_and_messages(np.concatenate([prefix, fork]), spec)
    assert fork["batch_start"][0] == clone["batch_start"][0] and fork["core"][0] == clone["core"][0]


def test_positions_and_max_requests_go_on_counting():
    """(c): a stream capped at 3,000 requests, forked 1,000 in, has 2,000 left whatever its seed."""
    kind = A.PU_STREAM_UNIFORM_HOTSPOT
    prefix, clone, fork, fresh = _forked(kind, "S1", 1000, max_requests=3000)
    assert len(prefix) == 1000 and len(clone) == 2000 and len(fork) == 2000 and len(fresh) == 3000


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("field,value", [("kind", A.PU_STREAM_UNIFORM), ("num_cores", 49), ("quantum", 201),
                                         ("num_quanta", 4), ("max_msg", 10), ("num_progs", 3),
                                         ("max_requests", 500), ("write_pct", 40)])
def test_a_destination_of_another_shape_is_refused_and_unchanged(field, value):
    src = _spec(A.PU_STREAM_UNIFORM_HOTSPOT, "S1")
    other = dataclasses.replace(_spec(A.PU_STREAM_UNIFORM_HOTSPOT, "S1", seed=5), **{field: value})
    ss = P.StreamSet([src, other, dataclasses.replace(src, seed=6)])
    try:
        ss.next(100)
        assert lib().pu_stream_fork(ss._h[1], ss._h[0], 1, NEW_SEED) == -22
        assert "parameters differ" in U.last_error()
        with pytest.raises(P.UncoreError, match="stream 1"):
            ss.fork(0, seeds=[1, 2, 3])                      # all or nothing: stream 2 is not forked either
        assert [ss.position(i) for i in range(3)] == [100, 100, 100]
        np.testing.assert_array_equal(_take(ss, 1), P.generate_stream(other)[100:])
        np.testing.assert_array_equal(_take(ss, 2), P.generate_stream(dataclasses.replace(src, seed=6))[100:])
        np.testing.assert_array_equal(_take(ss, 0), P.generate_stream(src)[100:])
    finally:
        ss.close()
