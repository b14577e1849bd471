"""The synthetic request streams generated on the device (DeviceStreamSet,
pu_dstream_*; primesim_amd/csrc/stream_gen.hip) equal the host generator's byte
for byte, in both record formats and under any chunking, and feed run_device
without a request ever being on the host.

Shapes: the smallest at which each mechanism of the kernel can go wrong (with
seed 7 the request counts are 11,607 / 86 / 2,294 / 33,423 / 2,369 for every kind):
  S1  48 cores                fewer cores than a wave
  S2  1 core                  one core
  S3  70 cores, quantum 2     a quantum shorter than a gap: empty (quantum, core)
                              cells; cores just past one wave
  S4  1,030 cores             more cores than one group of the workgroup
  S5  64 cores, quantum 3     messages of two requests; exactly one wave of cores
Device output lands in uint8 tensors pre-filled with 0xA5, so unwritten bytes show.
"""
import functools

import numpy as np
import pytest

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U
from golden_util import Case

pytestmark = pytest.mark.gpu

KINDS = [A.PU_STREAM_PRIVATE_STREAMING, A.PU_STREAM_SHARED_UNIFORM, A.PU_STREAM_MULTIPROGRAM,
         A.PU_STREAM_UNIFORM_HOTSPOT, A.PU_STREAM_PRODUCER_CONSUMER, A.PU_STREAM_UNIFORM]
#            cores quantum quanta max_msg progs  requests
SHAPES = {"S1": (48, 200, 3, 9, 2, 11607), "S2": (1, 50, 4, 3, 1, 86), "S3": (70, 2, 40, 5, 3, 2294),
          "S4": (1030, 40, 2, 100, 4, 33423), "S5": (64, 3, 30, 2, 1, 2369)}
FILL = 0xA5


def _spec(kind, shape, seed=7, **kw):
    c, q, nq, mm, pr, _ = SHAPES[shape]
    return P.StreamSpec(kind, c, seed=seed, quantum=q, num_quanta=nq, max_msg=mm, num_progs=pr, **kw)


@functools.lru_cache(maxsize=None)
def _want_bytes(kind, shape, seed=7):
    """(pu_req bytes [n, 32], pu_req16 bytes [n, 16]) of the host stream; computed once, never changed."""
    r = P.generate_stream(_spec(kind, shape, seed))
    if seed == 7:
        assert len(r) == SHAPES[shape][5]
    b32 = r.view(np.uint8).reshape(len(r), 32).copy()
    b16 = U.pack_req16(r).view(np.uint8).reshape(len(r), 16).copy()
    b32.setflags(write=False)
    b16.setflags(write=False)
    return b32, b16


def _drive(dss, wants, chunk, fmt=A.PU_REQ_FMT_32, gap=0, stream=None, extra_calls=2):
    """Calls next_into until every stream has answered 0 (the first of the extra calls), and
    extra_calls - 1 times more, each call into its own 0xA5-filled slab, on `stream` (a
    torch stream) or on the set's own stream.  Returns the check to run afterwards; per stream:
    d_got = min(chunk, left) on every call, the records concatenate to the host stream,
    every byte the call does not own still holds 0xA5, positions() ends at the stream's length."""
    import torch
    dev = torch.device("cuda", 0)
    rec = 32 if fmt == A.PU_REQ_FMT_32 else 16
    count, stride = len(wants), chunk + gap
    longest = max(len(w) for w in wants)
    ncalls = -(-longest // chunk) + extra_calls
    out = torch.full((ncalls, count, stride, rec), FILL, dtype=torch.uint8, device=dev)
    got = torch.full((ncalls, count), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)             # the fills are done before any stream writes records
    for k in range(ncalls):
        dss.next_into(out[k].data_ptr(), chunk, stride=stride, fmt=fmt, d_got_ptr=got[k].data_ptr(),
                      stream_ptr=stream.cuda_stream if stream is not None else 0)
    return functools.partial(_check, dss, wants, chunk, out, got)


def _check(dss, wants, chunk, out, got):
    pos = dss.positions()                   # waits for the set's outstanding calls
    o, g = out.cpu().numpy(), got.cpu().numpy()
    ncalls = o.shape[0]
    for i, w in enumerate(wants):
        left = len(w)
        for k in range(ncalls):
            n = min(chunk, left)
            assert g[k, i] == n, f"stream {i} call {k}: d_got {g[k, i]}, expected {n}"
            at = len(w) - left
            np.testing.assert_array_equal(o[k, i, :n], w[at:at + n], err_msg=f"stream {i} call {k}")
            assert np.all(o[k, i, n:] == FILL), f"stream {i} call {k}: bytes past record {n} were written"
            left -= n
        assert left == 0 and g[-1, i] == 0           # the last call found the stream at its end and wrote nothing
    np.testing.assert_array_equal(pos, [len(w) for w in wants])


def _chunks():
    for shape in SHAPES:
        cs = [7, 100, 4096]
        if shape in ("S2", "S3"):
            cs.append(1)
        if shape in ("S1", "S4"):
            cs.append(40000)          # larger than the whole stream
        for c in cs:
            yield shape, c


@pytest.mark.parametrize("shape,chunk", list(_chunks()))
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_equals_one_shot(kind, shape, chunk):
    want = _want_bytes(kind, shape)[0]
    dss = P.DeviceStreamSet([_spec(kind, shape)])
    try:
        assert len(dss) == 1
        _drive(dss, [want], chunk)()
    finally:
        dss.close()


def test_mixed_set_with_a_row_gap():
    """Five streams of different shapes, kinds and seeds in one set, stride = n_each + 3."""
    mix = [("S1", KINDS[0], 11), ("S2", KINDS[1], 12), ("S3", KINDS[2], 13), ("S4", KINDS[3], 14), ("S5", KINDS[4], 15)]
    specs = [_spec(k, sh, seed) for sh, k, seed in mix]
    wants = [_want_bytes(k, sh, seed)[0] for sh, k, seed in mix]
    dss = P.DeviceStreamSet(specs)
    try:
        assert len(dss) == 5 and dss.state_bytes > 24 * sum(sp.num_cores for sp in specs)
        import torch
        _drive(dss, wants, 500, gap=3, stream=torch.cuda.Stream("cuda:0"))()
    finally:
        dss.close()


def test_max_requests_ends_the_stream():
    """tests/test_stream.py::test_resumable_stream_respects_max_requests, on the device."""
    spec = P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 1024, seed=4, num_quanta=64, max_requests=10_000)
    r = P.generate_stream(spec)
    assert len(r) == 10_000
    want = r.view(np.uint8).reshape(len(r), 32)
    dss = P.DeviceStreamSet([spec])
    try:
        _drive(dss, [want], 6000, extra_calls=1)()       # 6,000, then 4,000, then 0
    finally:
        dss.close()


@pytest.mark.parametrize("chunk", [7, 4096])
@pytest.mark.parametrize("shape", ["S1", "S3", "S4"])
@pytest.mark.parametrize("kind", [A.PU_STREAM_SHARED_UNIFORM, A.PU_STREAM_MULTIPROGRAM, A.PU_STREAM_UNIFORM_HOTSPOT])
def test_format_16_equals_the_packed_host_stream(kind, shape, chunk):
    want16 = _want_bytes(kind, shape)[1]
    dss = P.DeviceStreamSet([_spec(kind, shape)])
    try:
        _drive(dss, [want16], chunk, fmt=A.PU_REQ_FMT_16)()
    finally:
        dss.close()


def test_format_16_is_refused_for_a_stream_that_may_not_fit():
    import torch
    wide = P.StreamSpec(A.PU_STREAM_UNIFORM, 64, seed=2, quantum=100, num_quanta=1, max_msg=9, num_progs=64)
    fine = _spec(A.PU_STREAM_UNIFORM_HOTSPOT, "S1")
    w = P.generate_stream(wide)
    wants = [_want_bytes(A.PU_STREAM_UNIFORM_HOTSPOT, "S1")[0], w.view(np.uint8).reshape(len(w), 32)]
    dss = P.DeviceStreamSet([fine, wide])
    try:
        buf = torch.full((2, 64, 16), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(P.UncoreError, match=r"stream 1 does not fit pu_req16.*\(-34\)"):
            dss.next_into(buf.data_ptr(), 64, fmt=A.PU_REQ_FMT_16)
        torch.cuda.synchronize()
        assert bool((buf == FILL).all())
        np.testing.assert_array_equal(dss.positions(), [0, 0])
        _drive(dss, wants, 4096)()
    finally:
        dss.close()


def _generate_on_device(spec, n, fmt, s, chunk=4096):
    """The whole stream on the device, in chunks on torch stream s, into one tensor of n records."""
    import torch
    rec = 32 if fmt == A.PU_REQ_FMT_32 else 16
    with torch.cuda.stream(s):
        d = torch.full((n + chunk, rec), FILL, dtype=torch.uint8, device="cuda:0")
    dss = P.DeviceStreamSet([spec])
    try:
        for at in range(0, n, chunk):
            dss.next_into(d[at:].data_ptr(), chunk, fmt=fmt, stream_ptr=s.cuda_stream)
        assert dss.positions()[0] == n
    finally:
        dss.close()
    assert bool((d[n:] == FILL).all())
    return d


@pytest.mark.parametrize("name,fmt", [("c1_stream", A.PU_REQ_FMT_32), ("small_msgs", A.PU_REQ_FMT_32),
                                      ("c3_multiprog", A.PU_REQ_FMT_32), ("c4_hotspot", A.PU_REQ_FMT_32),
                                      ("c4_hotspot", A.PU_REQ_FMT_16)])
def test_goldens_straight_from_the_device(name, fmt):
    """The golden's requests never exist on the host: generated on the device, run by run_device."""
    import torch
    c = Case(name)
    spec = P.StreamSpec(**c.meta["stream"])
    n = len(c.reqs)
    s = torch.cuda.Stream("cuda:0")         # one stream orders the generator and the engine
    d_reqs = _generate_on_device(spec, n, fmt, s)
    host = c.reqs.view(np.uint8).reshape(n, 32) if fmt == A.PU_REQ_FMT_32 else \
        U.pack_req16(np.ascontiguousarray(c.reqs)).view(np.uint8).reshape(n, 16)
    np.testing.assert_array_equal(d_reqs[:n].cpu().numpy(), host)
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    try:
        if c.closed:
            um.set_replay_mode(U.PU_REPLAY_CLOSED)
        for prog, th in c.threads:
            um.allocCore(prog, th)
        d_off = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
        d_del = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        um.set_device_req_format(fmt)
        try:
            torch.cuda.synchronize()
            um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), s.cuda_stream)
            s.synchronize()
        finally:
            um.set_device_req_format(A.PU_REQ_FMT_32)
        c.check_delays(d_del.cpu().numpy())
        np.testing.assert_array_equal(um.completion(), c.completion)
        assert um.report() == c.report
    finally:
        um.close()


def test_small_ensemble_fed_from_the_device():
    """Six replicas of C2, three chunks of 2,000: DeviceStreamSet -> run_device equals StreamSet -> run_device."""
    import torch
    R, n, chunks = 6, 2000, 3
    dev = torch.device("cuda", 0)
    cfg = P.config_from_dict(CF.preset("C2"))
    specs = [P.StreamSpec(A.PU_STREAM_SHARED_UNIFORM, 64, seed=300 + r) for r in range(R)]

    def run(fill):
        um = P.UncoreManager()
        um.init(cfg, replicas=R)
        try:
            for prog, th in P.stream_threads(specs[0]):
                um.allocCore(prog, th)
            d_reqs = torch.full((R, n, 32), FILL, dtype=torch.uint8, device=dev)
            d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
            d_del = torch.full((R, n), -7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            s = torch.cuda.Stream(dev)      # one stream orders the generator and the engine
            delays = []
            for _ in range(chunks):
                fill(d_reqs, s)
                um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), s.cuda_stream)
                s.synchronize()
                delays.append(d_del.cpu().numpy().copy())
            return (np.concatenate(delays, axis=1), [um.completion(r) for r in range(R)],
                    [um.stats(r).as_dict() for r in range(R)])
        finally:
            um.close()

    dss = P.DeviceStreamSet(specs)
    hss = P.StreamSet(specs)
    try:
        dev_run = run(lambda d, s: dss.next_into(d.data_ptr(), n, stream_ptr=s.cuda_stream))

        def from_host(d, s):
            h = hss.next(n)
            assert h.shape == (R, n)
            d.copy_(torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(R, n, 32)))
            torch.cuda.synchronize(dev)
        host_run = run(from_host)
        np.testing.assert_array_equal(dss.positions(), [n * chunks] * R)
    finally:
        dss.close()
        hss.close()
    np.testing.assert_array_equal(dev_run[0], host_run[0])
    for a, b in zip(dev_run[1], host_run[1]):
        np.testing.assert_array_equal(a, b)
    assert dev_run[2] == host_run[2]
    assert all(st["requests"] == n * chunks and st["error_flags"] == 0 for st in dev_run[2])


def test_two_sets_on_two_streams():
    """The generator state is per set: interleaved calls on two sets, each on its own stream."""
    import torch
    dev = torch.device("cuda", 0)
    a = [(A.PU_STREAM_UNIFORM_HOTSPOT, "S1"), (A.PU_STREAM_SHARED_UNIFORM, "S3")]
    b = [(A.PU_STREAM_SHARED_UNIFORM, "S1"), (A.PU_STREAM_PRIVATE_STREAMING, "S5"), (A.PU_STREAM_MULTIPROGRAM, "S2")]
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    da = P.DeviceStreamSet([_spec(k, sh) for k, sh in a])
    db = P.DeviceStreamSet([_spec(k, sh) for k, sh in b])
    try:
        # both sets' calls are queued before either is checked; the sets differ in chunk and count
        torch.cuda.synchronize()
        checks = _drive_interleaved(da, [_want_bytes(k, sh)[0] for k, sh in a], 300, sa,
                                db, [_want_bytes(k, sh)[0] for k, sh in b], 170, sb)
        for check in checks:
            check()
    finally:
        da.close()
        db.close()


def _drive_interleaved(d1, w1, c1, s1, d2, w2, c2, s2):
    """_drive for two sets with their calls alternating on the host."""
    import torch
    dev = torch.device("cuda", 0)
    plans = []
    for dss, wants, chunk, s in ((d1, w1, c1, s1), (d2, w2, c2, s2)):
        ncalls = -(-max(len(w) for w in wants) // chunk) + 2
        out = torch.full((ncalls, len(wants), chunk, 32), FILL, dtype=torch.uint8, device=dev)
        got = torch.full((ncalls, len(wants)), -1, dtype=torch.int64, device=dev)
        plans.append((dss, wants, chunk, s, out, got, ncalls))
    torch.cuda.synchronize(dev)
    for k in range(max(p[6] for p in plans)):
        for dss, wants, chunk, s, out, got, ncalls in plans:
            if k < ncalls:
                dss.next_into(out[k].data_ptr(), chunk, d_got_ptr=got[k].data_ptr(), stream_ptr=s.cuda_stream)
    return [functools.partial(_check, dss, wants, chunk, out, got) for dss, wants, chunk, s, out, got, _ in plans]
