#!/usr/bin/env python3
"""Time to learn how an ensemble's simulations ended: the device gather of the
end-of-run results (DeviceRunResults, primesim_amd/csrc/run_results.hip) against the
per-replica host path it replaces, on the bench's shape: the C4 preset, as many
replicas as the engine keeps resident, after one chunk of --chunk requests per replica
(DeviceStreamSet kind 4 -> run_device), so that the state gathered is not trivial.

  device   gather + read of every replica, without the per-queue map and with it:
           "kernel_seconds" is a HIP-event window around `steps` whole gather calls
           divided by `steps` (the kernel plus the handle's lock, the event record and
           the gaps between launches, so an upper bound of the kernel), then the wall
           time of one gather + read (launch, kernel, one copy of 448 B per replica);
           queue_totals() once per variant (two more launches and a copy), wall time;
  host     what a user has without the gather: stats(r) + completion(r) per replica,
           each a synchronise and a handful of blocking copies.  Timed on the first
           --host-replicas replicas and scaled to all of them (the cost per replica
           does not depend on the replica); the file says so.

Before any timing the first and the last replica's device records are compared with
pu_dres_host_gather; the tool exits non-zero when they differ.  Device and host phases
alternate `--rounds` times, each after a warm-up call of its own.  The bound quoted for
the kernel is the bytes its loads touch over the HBM read rate: a replica's queue
headers as whole 32-B records (piece a is 16 B of each, the lines are read whole), its
completion cycles and its EngineStats.  Prints one JSON line.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 4            # bench.py's
HBM_READ_BOUND = 8e12    # bytes per second


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", default="C4")
    ap.add_argument("--replicas", type=int, default=0, help="0: as many as the engine keeps resident")
    ap.add_argument("--chunk", type=int, default=2048, help="requests per replica run before the gathers")
    ap.add_argument("--steps", type=int, default=20, help="timed gathers per variant and phase")
    ap.add_argument("--host-replicas", type=int, default=256, help="replicas the host phase reads (scaled to all)")
    ap.add_argument("--rounds", type=int, default=2, help="device/host alternations (at least 2)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("run_results_bench: no GPU (the device gather has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    cfg = P.config_from_dict(CF.preset(args.preset))
    nc = cfg.sys.num_cores
    R = args.replicas
    if R <= 0:
        probe = P.UncoreManager()
        probe.init(cfg, replicas=1)
        R = probe.resident_replicas
        probe.close()
    n = args.chunk
    HR = min(R, args.host_replicas)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream

    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, nc, seed=replica_seed(SEED_BASE, 0, r), num_quanta=64)
             for r in range(R)]
    dss = P.DeviceStreamSet(specs)
    sets = {False: P.DeviceRunResults(um), True: P.DeviceRunResults(um, queues=True)}
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        d_reqs = torch.empty((R, n, 32), dtype=torch.uint8, device=dev)
        d_del = torch.empty((R, n), dtype=torch.int32, device=dev)
        d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
        torch.cuda.synchronize(dev)
        dss.next_into(d_reqs.data_ptr(), n, stream_ptr=sp)
        um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sp)
        stream.synchronize()
        um.synchronize()
        engine_ms = um.last_kernel_ms()

        # ---- the device records are the host gather's, before any timing
        for keep in (False, True):
            sets[keep].gather(stream_ptr=sp)
            got = sets[keep].read()
            for r in sorted({0, R - 1}):
                if got[r].tobytes() != P.host_run_results(um, r).tobytes():
                    print(f"run_results_bench: replica {r} (map {keep}): the device record differs from the host gather",
                          file=sys.stderr)
                    return 1
        requests = [int(got[0]["stats"]["requests"]), int(got[R - 1]["stats"]["requests"])]
        link_visits = int(got["link_visits"].sum())

        def device_phase(keep: bool) -> dict:
            s = sets[keep]
            s.gather(stream_ptr=sp)                                        # warm-up
            s.read()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                s.gather(stream_ptr=sp)
            e1.record(stream)
            stream.synchronize()
            kernel = e0.elapsed_time(e1) / 1e3 / args.steps
            t0 = time.perf_counter()
            s.gather(stream_ptr=sp)
            s.read()
            wall = time.perf_counter() - t0
            s.queue_totals()                                               # warm-up
            t0 = time.perf_counter()
            s.queue_totals()
            return {"kernel_seconds": kernel, "gather_read_wall_seconds": wall,
                    "queue_totals_wall_seconds": time.perf_counter() - t0}

        def host_phase() -> float:
            um.stats(0)                                                    # warm-up
            um.completion(0)
            t0 = time.perf_counter()
            for r in range(HR):
                um.stats(r)
                um.completion(r)
            return time.perf_counter() - t0

        res = {"device": {False: [], True: []}, "host": []}
        for _ in range(args.rounds):
            for keep in (False, True):
                res["device"][keep].append(device_phase(keep))
            res["host"].append(host_phase())
        state_bytes = {"without_map": sets[False].state_bytes, "with_map": sets[True].state_bytes}
        nq = sets[False].num_queues
    finally:
        for s in sets.values():
            s.close()
        dss.close()
        um.close()

    bytes_per_replica = nq * 32 + nc * 8 + 43 * 8
    bound = R * bytes_per_replica / HBM_READ_BOUND
    host_scaled = [t * R / HR for t in res["host"]]
    line = {"tool": "run_results_bench", "gpu": torch.cuda.get_device_name(0), "preset": args.preset, "replicas": R,
            "cores": nc, "queues": nq, "chunk": n, "engine_chunk_ms": engine_ms, "steps": args.steps, "rounds": args.rounds,
            "requests_first_last": requests, "link_visits_all_replicas": link_visits,
            "records_checked": "first and last replica, with and without the map, equal to pu_dres_host_gather",
            "state_bytes": state_bytes, "record_bytes": 448, "map_bytes_per_replica": nq * 16,
            "bytes_loaded_per_replica": bytes_per_replica, "hbm_read_bound_bytes_per_s": HBM_READ_BOUND,
            "bound_seconds": bound,
            "device_without_map": res["device"][False], "device_with_map": res["device"][True],
            "kernel_share_of_bound_without_map": [bound / d["kernel_seconds"] for d in res["device"][False]],
            "kernel_share_of_bound_with_map": [bound / d["kernel_seconds"] for d in res["device"][True]],
            "host_replicas_timed": HR, "host_seconds_timed": res["host"],
            "host_seconds_scaled_to_all_replicas": host_scaled,
            "host_scaling": f"timed on {HR} of {R} replicas and multiplied by {R}/{HR}",
            "host_over_device_wall_worst_case":
                min(host_scaled) / max(d["gather_read_wall_seconds"] for d in res["device"][False])}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
