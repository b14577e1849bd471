#!/usr/bin/env python3
"""Requests per second of the recorded-trace replay on the device (DeviceTraceSet,
primesim_amd/csrc/trace_place.hip) against the host staging it replaces, at the
bench's shape: one trace over 1,024 cores, --replicas replicas each under its own
placement and skew rows, --chunk requests per replica and call.

  device   `steps` calls of next_into per window, in each record format and with the
           rows staged in LDS ("lds") and gathered from global memory ("global",
           PRIMEUNCORE_TRACE_ROWS), timed by HIP events around whole calls and ended
           by a synchronise;
  host     the only other way to feed placed replicas: per replica the host twin
           (pu_trace_place) on the job's host threads, pu_pack_req16 for format 16,
           a pinned-to-device copy per group of 256 replicas; a host clock around
           work that ends in a synchronise.  --host-replicas of the replicas are
           staged (the rate is per request).

Before any timing the first and the last replica's device records are compared with
place_trace's (both formats, both instantiations, two consecutive calls); the tool
exits non-zero when they differ.  Device and host phases alternate `--rounds` times
(each after a warm-up call of its own) so the run-to-run spread shows.  The trace is
the bench's stream (kind 4, 64 quanta) cut at (steps + 1) chunks.  Prints one JSON
line.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import ctypes
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
STAGE_GROUP = 256        # bench.py's: replicas the host stages per copy
HBM_WRITE_BOUND = 8e12   # bytes per second
FORK_SHARE = 0.86        # replica_fork_kernel's share of the same bound: the mark for a pure-store kernel
ROWS_ENV = "PRIMEUNCORE_TRACE_ROWS"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--cores", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=50, help="timed device calls per window")
    ap.add_argument("--host-steps", type=int, default=1, help="timed host chunks per format and phase")
    ap.add_argument("--host-replicas", type=int, default=1024, help="replicas the host phases stage")
    ap.add_argument("--rounds", type=int, default=2, help="device/host alternations (at least 2)")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="host threads")
    ap.add_argument("--skew-max", type=int, default=1000)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("trace_place_bench: no GPU (the device replay has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    R, n, nc = args.replicas, args.chunk, args.cores
    HR = min(R, args.host_replicas)
    T = n * (args.steps + 1)
    trace = P.generate_stream(P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, nc, seed=replica_seed(SEED_BASE, 0, 0),
                                           num_quanta=64, max_requests=T))
    if len(trace) != T:
        print(f"trace_place_bench: the stream holds {len(trace)} requests, {T} are needed", file=sys.stderr)
        return 1
    place = P.random_placements(R, nc, SEED_BASE)
    skew = np.random.default_rng(SEED_BASE).integers(0, args.skew_max + 1, (R, nc)).astype(np.int32)
    skew[0] = 0
    fmts = {"req32": (A.PU_REQ_FMT_32, 32), "req16": (A.PU_REQ_FMT_16, 16)}
    variants = ("lds", "global")
    d_out = torch.empty((R, n * 32), dtype=torch.uint8, device=dev)      # both formats write here
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream
    ts = P.DeviceTraceSet(trace, nc, R, placements=place, skews=skew)
    if not ts.fits_req16():
        print(f"trace_place_bench: {P.uncore.last_error()}", file=sys.stderr)
        return 1

    # ---- the device records are the host twin's, before any timing
    ends = [0, R - 1] if R > 1 else [0]
    for var in variants:
        os.environ[ROWS_ENV] = var
        for name, (fmt, rb) in fmts.items():
            ts.seek(0)
            for call in range(2):
                ts.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
                stream.synchronize()
                for i in ends:
                    want = P.place_trace(trace[call * n:(call + 1) * n], place[i], skew[i], fmt=fmt).view(np.uint8).reshape(-1)
                    got = d_out.view(-1)[i * n * rb:(i + 1) * n * rb].cpu().numpy()
                    if not np.array_equal(got, want):
                        print(f"trace_place_bench: replica {i} ({name}, rows {var}, call {call}): device records differ "
                              "from place_trace's", file=sys.stderr)
                        return 1

    # ---- (a) the device path
    def device_phase(fmt: int, var: str) -> float:
        os.environ[ROWS_ENV] = var
        ts.seek(0)
        ts.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)        # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            ts.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        e1.record(stream)
        stream.synchronize()
        assert ts.position() == T
        return e0.elapsed_time(e1) / 1e3

    # ---- (b) the host path it replaces: the host twin per replica, groups, two pinned buffers, a copy stream
    G = min(HR, STAGE_GROUP)
    pin32 = [torch.empty((G, n * 32), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    pin16 = [torch.empty((G, n * 16), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    copy_stream = torch.cuda.Stream(dev)
    pool = ThreadPoolExecutor(args.threads)
    L = P.uncore.lib()
    PI32 = ctypes.POINTER(ctypes.c_int32)
    in_flight = [None, None]
    turn = [0]

    def host_chunk(rb: int, at: int) -> None:
        out = d_out.view(-1)[:R * n * rb].view(R, n * rb)
        src = trace[at:at + n]

        for g0 in range(0, HR, G):
            m, i = min(G, HR - g0), turn[0] & 1
            turn[0] += 1
            if in_flight[i] is not None:
                in_flight[i].synchronize()
            p32, p16 = pin32[i], pin16[i]

            def one(k: int) -> int:
                r = g0 + k
                rc = L.pu_trace_place(src.ctypes.data, n, place[r].ctypes.data_as(PI32), skew[r].ctypes.data_as(PI32), nc,
                                      A.PU_REQ_FMT_32, p32[k].data_ptr())
                if rc == 0 and rb == 16:
                    rc = L.pu_pack_req16(p32[k].data_ptr(), n, p16[k].data_ptr())
                return rc
            if any(pool.map(one, range(m))):
                raise RuntimeError(f"trace_place_bench: host staging failed: {P.uncore.last_error()}")
            with torch.cuda.stream(copy_stream):
                out[g0:g0 + m].copy_((p32 if rb == 32 else p16)[:m], non_blocking=True)
                in_flight[i] = torch.cuda.Event()
                in_flight[i].record(copy_stream)

    def host_phase(rb: int) -> float:
        host_chunk(rb, 0)                                                  # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for k in range(args.host_steps):
            host_chunk(rb, (1 + k % args.steps) * n)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    res = {"device": {v: {k: [] for k in fmts} for v in variants}, "host": {k: [] for k in fmts}}
    for _ in range(args.rounds):
        for var in variants:
            for name, (fmt, rb) in fmts.items():
                res["device"][var][name].append(device_phase(fmt, var))
        for name, (fmt, rb) in fmts.items():
            res["host"][name].append(host_phase(rb))
    os.environ.pop(ROWS_ENV, None)
    ts.seek(0)
    default_seconds = {}
    for name, (fmt, rb) in fmts.items():                                   # the shipped choice, unforced
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts.seek(0)
        ts.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        e0.record(stream)
        for _ in range(args.steps):
            ts.next_into(d_out.data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        e1.record(stream)
        stream.synchronize()
        default_seconds[name] = e0.elapsed_time(e1) / 1e3
    state_bytes = ts.state_bytes
    ts.close()
    pool.shutdown()

    dev_reqs, host_reqs = R * n * args.steps, HR * n * args.host_steps
    line = {"tool": "trace_place_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "cores": nc, "chunk": n,
            "steps": args.steps, "host_steps": args.host_steps, "host_replicas": HR, "rounds": args.rounds,
            "host_threads": args.threads, "trace_records": T, "state_bytes": state_bytes,
            "lane_mapping": "lane = record, one workgroup of 256 per tile of 1,024 records of one replica",
            "write_bound_bytes_per_s": HBM_WRITE_BOUND, "replica_fork_share_of_write_bound": FORK_SHARE,
            "default_rows_seconds": default_seconds,
            "records_checked": "first and last replica, both formats, both instantiations, equal to place_trace"}
    slowest_dev, fastest_host = {}, {}
    for name, (fmt, rb) in fmts.items():
        h = [host_reqs / t for t in res["host"][name]]
        entry = {"host_requests_per_s": h, "host_seconds": res["host"][name], "bytes_written_per_call": R * n * rb}
        for var in variants:
            d = [dev_reqs / t for t in res["device"][var][name]]
            entry[var] = {"device_requests_per_s": d, "device_seconds": res["device"][var][name],
                          "device_bytes_written_per_s": [x * rb for x in d],
                          "device_share_of_hbm_write_bound": [x * rb / HBM_WRITE_BOUND for x in d],
                          "device_over_host_worst_case": min(d) / max(h)}
            slowest_dev[(name, var)] = min(d)
        fastest_host[name] = max(h)
        line[name] = entry
    line["device_faster_than_host_beyond_spread"] = all(v > fastest_host[k[0]] for k, v in slowest_dev.items())
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
