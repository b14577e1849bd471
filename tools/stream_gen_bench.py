#!/usr/bin/env python3
"""Requests per second of the device stream generator (DeviceStreamSet,
primesim_amd/csrc/stream_gen.hip) against the host staging it can replace, at the
bench's shape: the bench's stream (kind 4, 1,024 cores, 64 quanta, seeds from
dist.replica_seed), --replicas streams, --chunk requests per stream and call.

  device   `steps` calls of next_into in each record format, timed by HIP events
           around the calls and ended by a synchronise;
  host     the same number of requests the way bench.py stages them: groups of
           256 streams, StreamSet.next_into on the job's host threads, pu_pack_req16
           for format 16, a pinned-to-device copy; a host clock around work that
           ends in a synchronise.

Before any timing the first and the last stream's device records are compared
with the host generator's (both formats, two consecutive calls); the tool exits
non-zero when they differ.  Device and host phases alternate `--rounds` times
(each after a warm-up call of its own) so the run-to-run spread shows.  Prints
one JSON line.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 4            # bench.py's
STAGE_GROUP = 256        # bench.py's: streams the host generates per staging copy
HBM_WRITE_BOUND = 8e12   # bytes per second


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=3, help="timed device calls per format and phase")
    ap.add_argument("--host-steps", type=int, default=1, help="timed host chunks per format and phase")
    ap.add_argument("--rounds", type=int, default=2, help="device/host alternations (at least 2)")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="host generator threads")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("stream_gen_bench: no GPU (the device generator has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    R, n = args.replicas, args.chunk
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, 1024, seed=replica_seed(SEED_BASE, 0, r), num_quanta=64)
             for r in range(R)]
    fmts = {"req32": (A.PU_REQ_FMT_32, 32), "req16": (A.PU_REQ_FMT_16, 16)}
    d_out = torch.empty((R, n * 32), dtype=torch.uint8, device=dev)      # both formats write here
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream

    # ---- (c) the device records are the host's, before any timing
    dss = P.DeviceStreamSet(specs)
    ends = [0, R - 1] if R > 1 else [0]
    for name, (fmt, rb) in fmts.items():
        chk = P.DeviceStreamSet([specs[i] for i in ends])
        ref = P.StreamSet([specs[i] for i in ends])
        for call in range(2):
            chk.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
            stream.synchronize()
            want = ref.next(n)
            for row in range(len(ends)):
                w = np.ascontiguousarray(want[row])
                wb = (w if rb == 32 else P.pack_req16(w)).view(np.uint8).reshape(-1)
                got = d_out.view(-1)[row * n * rb:(row + 1) * n * rb].cpu().numpy()
                if not np.array_equal(got, wb):
                    print(f"stream_gen_bench: stream {ends[row]} ({name}, call {call}): device records differ from "
                          "the host generator's", file=sys.stderr)
                    return 1
        chk.close()
        ref.close()
    # ... and in the full set: its first and last rows against the same host streams
    ref = P.StreamSet([specs[i] for i in ends])
    dss.next_into(d_out.data_ptr(), n, fmt=A.PU_REQ_FMT_32, stream_ptr=sptr)
    stream.synchronize()
    want = ref.next(n)
    for row, i in enumerate(ends):
        got = d_out[i].cpu().numpy()
        if not np.array_equal(got, np.ascontiguousarray(want[row]).view(np.uint8).reshape(-1)):
            print(f"stream_gen_bench: stream {i} of the full set differs from the host generator's", file=sys.stderr)
            return 1
    ref.close()

    # ---- (a) the device path
    def device_phase(fmt: int) -> float:
        dss.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)      # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            dss.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3

    # ---- (b) the host path it replaces (bench.py's staging: groups, two pinned buffers, a copy stream)
    G = min(R, STAGE_GROUP)
    gens = [P.StreamSet(specs[g:g + G]) for g in range(0, R, G)]
    pin32 = [torch.empty((G, n * 32), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    pin16 = [torch.empty((G, n * 16), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    host32 = [p.numpy().view(A.REQ_DTYPE) for p in pin32]
    copy_stream = torch.cuda.Stream(dev)
    packers = ThreadPoolExecutor(args.threads)
    pack = P.uncore.lib().pu_pack_req16
    in_flight = [None, None]
    turn = [0]

    def host_chunk(rb: int) -> None:
        out = d_out.view(-1)[:R * n * rb].view(R, n * rb)
        for k, gen in enumerate(gens):
            m, i = len(gen), turn[0] & 1
            turn[0] += 1
            if in_flight[i] is not None:
                in_flight[i].synchronize()
            h = host32[i][:m]
            got = gen.next_into(h, args.threads)
            assert got == n, (got, n)
            src = pin32[i]
            if rb == 16:
                src = pin16[i]
                cut = [m * j // args.threads for j in range(args.threads + 1)]
                parts = [(a, z) for a, z in zip(cut[:-1], cut[1:]) if z > a]
                rcs = packers.map(lambda az: pack(h[az[0]:az[1]].ctypes.data, (az[1] - az[0]) * n,
                                                  src[az[0]:az[1]].data_ptr()), parts)
                if any(rcs):
                    P.uncore.pack_req16(h)
            with torch.cuda.stream(copy_stream):
                out[k * G:k * G + m].copy_(src[:m], non_blocking=True)
                in_flight[i] = torch.cuda.Event()
                in_flight[i].record(copy_stream)

    def host_phase(rb: int) -> float:
        host_chunk(rb)                                                     # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.host_steps):
            host_chunk(rb)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    res = {"device": {k: [] for k in fmts}, "host": {k: [] for k in fmts}}
    for _ in range(args.rounds):
        for name, (fmt, rb) in fmts.items():
            res["device"][name].append(device_phase(fmt))
        for name, (fmt, rb) in fmts.items():
            res["host"][name].append(host_phase(rb))
    state_bytes = dss.state_bytes
    dss.close()
    for g in gens:
        g.close()
    packers.shutdown()

    dev_reqs, host_reqs = R * n * args.steps, R * n * args.host_steps
    line = {"tool": "stream_gen_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "chunk": n,
            "steps": args.steps, "host_steps": args.host_steps, "rounds": args.rounds, "host_threads": args.threads,
            "lane_mapping": "lane = core, one workgroup of 256 per stream", "state_bytes": state_bytes,
            "records_checked": "first and last stream, both formats, equal to the host generator"}
    slowest_dev, fastest_host = {}, {}
    for name, (fmt, rb) in fmts.items():
        d = [dev_reqs / t for t in res["device"][name]]
        h = [host_reqs / t for t in res["host"][name]]
        line[name] = {
            "device_requests_per_s": d, "host_requests_per_s": h,
            "device_seconds": res["device"][name], "host_seconds": res["host"][name],
            "device_bytes_written_per_s": [x * rb for x in d],
            "device_share_of_hbm_write_bound": [x * rb / HBM_WRITE_BOUND for x in d],
            "device_over_host_worst_case": min(d) / max(h),
        }
        slowest_dev[name], fastest_host[name] = min(d), max(h)
    line["device_faster_than_host_beyond_spread"] = all(slowest_dev[k] > fastest_host[k] for k in fmts)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
