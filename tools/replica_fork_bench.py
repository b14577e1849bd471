#!/usr/bin/env python3
"""Time per call of a replica fork (UncoreManager.fork_replica, primesim_amd/csrc/replica_fork.hip)
at the bench's replica count: replica 0, warmed by one engine chunk, copied to all the others.

Per shape (C4 and C2 at --replicas replicas, streams of the kind the preset stands for):
  engine chunk   run_device over one --chunk-record chunk on every (cold) replica: the work
                 a fork replaces, once per replica and warm-up chunk;
  fork phases    the kernel with plain stores, the kernel with non-temporal stores
                 (PRIMEUNCORE_FORK_STORES selects them) and PU_FORK_BY_COPIES: `steps` calls per
                 HIP-event window over whole calls, after a warm-up call;
  stream fork    DeviceStreamSet.fork(0, seeds) of as many streams, the same way.
The phases alternate `--rounds` times so the run-to-run spread shows.  Before any timing the
first, a middle and the last destination are compared with the source byte for byte through
their end-of-run records, per phase.  Prints one JSON line.  Needs a GPU: there is no CPU
fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 4             # bench.py's
HBM_WRITE_BOUND = 8e12    # bytes per second
SHAPES = {"C4": 4, "C2": 2}   # preset -> PU_STREAM_* kind
PHASES = {"kernel_plain": ("plain", False), "kernel_nontemporal": ("nt", False), "copies": (None, True)}


def shape(preset: str, kind: int, args) -> dict:
    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF
    from primesim_amd.dist import replica_seed

    dev = torch.device("cuda", 0)
    R, n = args.replicas, args.chunk
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream
    cfg = P.config_from_dict(CF.preset(preset))
    cores = cfg.sys.num_cores
    quanta = -(-n * 4 // (cores * cfg.thread_sync_interval)) + 1
    specs = [P.StreamSpec(kind, cores, seed=replica_seed(SEED_BASE, 0, r), quantum=cfg.thread_sync_interval,
                          num_quanta=max(64, quanta), max_msg=cfg.max_msg_size) for r in range(R)]
    d_reqs = torch.empty((R, n * 16), dtype=torch.uint8, device=dev)
    d_del = torch.zeros((R, n), dtype=torch.int32, device=dev)
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
    torch.cuda.synchronize(dev)

    def window(call, steps):
        call()                                                             # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            call()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3 / steps

    # ---- the stream fork, and the chunk the engine runs
    dss = P.DeviceStreamSet(specs)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(1000)
    try:
        dss.next_into(d_reqs.data_ptr(), n, fmt=A.PU_REQ_FMT_16, stream_ptr=sptr)
        assert int(dss.positions().min()) == n
        stream_fork = [window(lambda: dss.fork(0, seeds=seeds, stream_ptr=sptr), args.stream_steps)
                       for _ in range(args.rounds)]
        stream_state = dss.state_bytes
    finally:
        dss.close()

    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    res = {k: [] for k in PHASES}
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        um.set_device_req_format(A.PU_REQ_FMT_16)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sptr)
        e1.record(stream)
        stream.synchronize()
        engine_chunk_s = e0.elapsed_time(e1) / 1e3
        replica_bytes = um.replica_bytes

        def fork(phase):
            stores, by_copies = PHASES[phase]
            if stores:
                os.environ["PRIMEUNCORE_FORK_STORES"] = stores
            um.fork_replica(0, by_copies=by_copies, stream_ptr=sptr)

        # replicas 1 .. R-1 hold their own chunk's state: every phase has something to overwrite
        want = P.host_run_results(um, 0).tobytes()
        for phase in PHASES:
            fork(phase)
            stream.synchronize()
            for r in sorted({1, R // 2, R - 1} - {0}):
                if P.host_run_results(um, r).tobytes() != want:
                    print(f"replica_fork_bench: {preset} {phase}: replica {r} differs from the source", file=sys.stderr)
                    return {}
            if phase != list(PHASES)[-1]:                                  # stale state again for the next phase
                um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sptr)
                stream.synchronize()
                want = P.host_run_results(um, 0).tobytes()
        for _ in range(args.rounds):
            for phase in PHASES:
                res[phase].append(window(lambda: fork(phase), args.steps))
    finally:
        os.environ.pop("PRIMEUNCORE_FORK_STORES", None)
        um.close()

    written = (R - 1) * replica_bytes
    spread = {k: (max(v) - min(v)) / min(v) for k, v in res.items()}
    best = min(("kernel_plain", "kernel_nontemporal"), key=lambda k: min(res[k]))
    return {"preset": preset, "stream_kind": kind, "replicas": R, "cores": cores, "replica_bytes": replica_bytes,
            "bytes_written_per_fork": written,
            "seconds_per_fork": res, "spread_over_rounds": spread,
            "share_of_write_bound": {k: [written / HBM_WRITE_BOUND / x for x in v] for k, v in res.items()},
            "kernel_over_copies": {k: [a / b for a, b in zip(res[k], res["copies"])]
                                   for k in ("kernel_plain", "kernel_nontemporal")},
            "faster_store_policy": best,
            "destinations_checked": "1, R/2 and R-1 equal the source's end-of-run record after every phase's fork",
            "stream_fork": {"seconds_per_call": stream_fork, "state_bytes": stream_state},
            "engine_chunk": {"records_per_replica": n, "seconds_cold": engine_chunk_s,
                             "over_fastest_fork": engine_chunk_s / min(min(v) for v in res.values())}}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960, help="records of the engine chunk a fork is compared with")
    ap.add_argument("--steps", type=int, default=3, help="timed forks per window")
    ap.add_argument("--stream-steps", type=int, default=20, help="timed stream forks per window")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the phases (at least 2)")
    ap.add_argument("--presets", default="C4,C2")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch
    if not torch.cuda.is_available():
        print("replica_fork_bench: no GPU (the fork has no CPU fallback)", file=sys.stderr)
        return 2
    line = {"tool": "replica_fork_bench", "gpu": torch.cuda.get_device_name(0), "steps": args.steps,
            "stream_steps": args.stream_steps, "rounds": args.rounds, "write_bound_bytes_per_s": HBM_WRITE_BOUND,
            "shapes": []}
    for preset in args.presets.split(","):
        s = shape(preset, SHAPES[preset], args)
        if not s:
            return 1
        line["shapes"].append(s)
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
