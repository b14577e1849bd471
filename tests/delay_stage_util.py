"""What the GPU tests of the three delay stages (test_gpu_dsum.py, test_gpu_dhist.py,
test_gpu_dtail.py) share: synthetic records on the device, one add of ranges, a stage
opened for a `with` block, a golden run through run_device and a stage on one torch
stream, and tools/ensemble_summary.py in a child process.  A helper module, not a
conftest: it holds no fixture and no test."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np

import primesim_amd as P
from primesim_amd import _abi as A
from primesim_amd import uncore as U
from dsum_fold import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = [A.PU_REQ_FMT_32, A.PU_REQ_FMT_16]
REC = {A.PU_REQ_FMT_32: 32, A.PU_REQ_FMT_16: 16}
# wave, workgroup-pass and trip edges of the record loads (delay_stage.h: 64, 256, 1,024)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def to_dev(reqs, delays, fmt):
    """(request records, delays) as device tensors; the copies are done when this returns."""
    import torch
    host = np.ascontiguousarray(reqs) if fmt == A.PU_REQ_FMT_32 else U.pack_req16(np.ascontiguousarray(reqs))
    b = host.view(np.uint8).reshape(len(reqs), REC[fmt]).copy()
    d_reqs = torch.from_numpy(b).to("cuda:0")
    d_del = torch.from_numpy(np.ascontiguousarray(delays, dtype=np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return d_reqs, d_del


def idx(values):
    import torch
    t = torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return t


def add(ds, dev, begins, ends, fmt, stream=None):
    """One add of ranges [begins[r], ends[r]); returns the index tensors (alive until the caller has read)."""
    b, e = idx(begins), idx(ends)
    ds.add(dev[0].data_ptr(), dev[1].data_ptr(), b.data_ptr(), e.data_ptr(), fmt=fmt,
           stream_ptr=stream.cuda_stream if stream is not None else 0)
    return b, e


@functools.lru_cache(maxsize=None)
def data(n, nc, seed):
    """synth(n, nc, seed), computed once and read-only."""
    r, d = synth(n, nc, seed)
    r.setflags(write=False)
    d.setflags(write=False)
    return r, d


@contextlib.contextmanager
def opened(stage, *args, **kwargs):
    """stage(*args, **kwargs), closed when the block ends."""
    ds = stage(*args, **kwargs)
    try:
        yield ds
    finally:
        ds.close()


def run_golden(c, d_reqs, fmt, s, open_stage, read):
    """The golden's requests (already on the device) through run_device and the stage
    open_stage() gives, both on stream s; returns read(stage), taken before the stream is
    synchronized.  The delays are checked against the golden's."""
    import torch
    n = len(c.reqs)
    um = P.UncoreManager()
    um.init(P.load_config(c.xml_path), replicas=1)
    ds = open_stage()
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
            ds.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt,
                   stream_ptr=s.cuda_stream)
            got = read(ds)
            s.synchronize()
        finally:
            um.set_device_req_format(A.PU_REQ_FMT_32)
        c.check_delays(d_del.cpu().numpy())
    finally:
        ds.close()
        um.close()
    return got


def summary_tool(*extra):
    """tools/ensemble_summary.py in a child process: C1, kind 1, 4 replicas, 2 chunks of 2,000; its JSON lines as text."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ensemble_summary.py"), "--preset", "C1", "--kind", "1",
                        "--replicas", "4", "--chunk", "2000", "--chunks", "2", *extra],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return [x for x in r.stdout.splitlines() if x.startswith("{")]
