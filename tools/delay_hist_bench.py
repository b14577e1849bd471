#!/usr/bin/env python3
"""Time per call of the device delay histograms (DeviceDelayHistogram,
primesim_amd/csrc/delay_hist.hip) on one chunk of the bench's shape: --replicas
replicas x --chunk records, requests from DeviceStreamSet kind 4 (the bench's stream,
seeds from dist.replica_seed) in both record formats, and delays from ONE ENGINE CHUNK
of C4 (run_device over those requests), so the values the kernel counts are spread as
the engine's are, not as a fill's.

  add        `steps` calls per HIP-event window after a warm-up call, and as many of
             DeviceDelaySummary.add without per-core tables on the same arrays in the
             same run: the yardstick, the parent commit's kernel, which reads the same
             lines;
  reading    wall time of quantiles() (eight quantiles, every replica, both classes) and
             of total(), against the host alternative: read() of every histogram and
             histogram_quantiles on the job's host threads.

Before any timing the first and the last replica's histograms are compared with the
host fold of their records (delay_histogram), in both formats; the tool exits non-zero
when they differ.  The phases alternate `--rounds` times so the
run-to-run spread shows.  Prints one JSON line.  Needs a GPU: there is no CPU fallback.
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
HBM_READ_BOUND = 8e12    # bytes per second
# the bytes of the whole lines the loads of a record touch (the request records are read in full
# lines: 16 or 32 B a record; 4 B of delay), as DESIGN.md section 6b counts them
BYTES_LINES = {"req32": 4 + 32, "req16": 4 + 16}
PPMS = [0, 1, 500000, 900000, 990000, 999000, 999999, 1000000]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=50, help="timed calls per window")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the phases (at least 2)")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="host threads of the host alternative")
    ap.add_argument("--preset", default="C4", help="the engine configuration whose delays are counted")
    ap.add_argument("--engine-record", default=os.path.join(ROOT, "profiles", "r8_bench.json"),
                    help="a bench.py result line: the engine's rate on this shape")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("delay_hist_bench: no GPU (the device histograms have no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    R, n = args.replicas, args.chunk
    fmts = {"req32": (A.PU_REQ_FMT_32, 32), "req16": (A.PU_REQ_FMT_16, 16)}
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream

    # ---- the chunk: requests of both formats from the device generator (the same seeds: the same requests)
    cfg = P.config_from_dict(CF.preset(args.preset))
    cores = cfg.sys.num_cores
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, cores, seed=replica_seed(SEED_BASE, 0, r), num_quanta=64)
             for r in range(R)]
    d_reqs = {k: torch.empty((R, n * rb), dtype=torch.uint8, device=dev) for k, (_, rb) in fmts.items()}
    d_del = torch.zeros((R, n), dtype=torch.int32, device=dev)
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
    torch.cuda.synchronize(dev)
    for k, (fmt, rb) in fmts.items():
        dss = P.DeviceStreamSet(specs)
        dss.next_into(d_reqs[k].data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        assert int(dss.positions().min()) == n
        dss.close()
    stream.synchronize()

    # ---- the delays: one engine chunk over the pu_req16 records (cold replicas), then the engine leaves
    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    try:
        for prog, th in P.stream_threads(specs[0]):
            um.allocCore(prog, th)
        um.set_device_req_format(A.PU_REQ_FMT_16)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        um.run_device(d_reqs["req16"].data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sptr)
        e1.record(stream)
        stream.synchronize()
        engine_chunk_s = e0.elapsed_time(e1) / 1e3
        flags = um.error_flags(R)
        halted = int((np.asarray(flags) != 0).sum())
    finally:
        um.close()

    # what the kernel meets: distinct counters per wave instruction (64 consecutive records), on a sample
    sample = d_del[:: max(1, R // 64)].cpu().numpy()
    words = d_reqs["req16"][:: max(1, R // 64)].cpu().numpy().view(np.uint64).reshape(len(sample), n, 2)[:, :, 1]
    cls = ((words >> np.uint64(62)) & np.uint64(1)).astype(np.int64)
    fine = np.array([P.dhist_bucket_of(int(v)) for v in np.unique(sample)])
    key = cls * A.PU_DHIST_BUCKETS + fine[np.searchsorted(np.unique(sample), sample)]
    waves = key[:, : n - n % 64].reshape(len(sample), -1, 64)
    srt = np.sort(waves, axis=2)
    distinct = 1 + (srt[:, :, 1:] != srt[:, :, :-1]).sum(axis=2)
    keys_per_wave = {"mean": float(distinct.mean()), "median": float(np.median(distinct)),
                     "share_at_most_4": float((distinct <= 4).mean()), "max": int(distinct.max()),
                     "live_counters_of_a_replica_mean": float(np.mean([len(np.unique(k)) for k in key])),
                     "sampled_replicas": len(sample)}

    sets = {"dhist": P.DeviceDelayHistogram(R), "dsum_no_tables": P.DeviceDelaySummary(R)}

    def add(what: str, k: str) -> None:
        sets[what].add(d_reqs[k].data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8,
                       fmt=fmts[k][0], stream_ptr=sptr)

    # ---- the device histograms are the host fold's, before any timing
    ends = [0, R - 1] if R > 1 else [0]
    for k, (fmt, rb) in fmts.items():
        sets["dhist"].reset()
        add("dhist", k)
        for i in ends:
            got = sets["dhist"].read(i, 1)[0]
            recs = d_reqs[k][i].cpu().numpy()
            recs = recs.view(A.REQ_DTYPE) if rb == 32 else recs.view(np.uint64).reshape(n, 2)
            want = P.delay_histogram(recs, d_del[i].cpu().numpy(), fmt=fmt)
            if not np.array_equal(got, want):
                print(f"delay_hist_bench: replica {i} ({k}): the device histogram differs from the host fold", file=sys.stderr)
                return 1

    def phase(what: str, k: str) -> float:
        add(what, k)                                                       # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            add(what, k)
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3 / args.steps

    # ---- reading: quantiles() and total() on the device against read() + histogram_quantiles on the host
    pool = ThreadPoolExecutor(args.threads)

    def device_read():
        t0 = time.perf_counter()
        count, bucket = sets["dhist"].quantiles(PPMS)
        t1 = time.perf_counter()
        tot = sets["dhist"].total()
        t2 = time.perf_counter()
        return (t1 - t0, t2 - t1), (count, bucket, tot)

    def host_read():
        t0 = time.perf_counter()
        hist = sets["dhist"].read()
        t1 = time.perf_counter()
        step = -(-R // args.threads)
        parts = list(pool.map(lambda a: P.histogram_quantiles(hist[a:a + step], PPMS), range(0, R, step)))
        count, bucket = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        tot = hist.sum(axis=0)
        t2 = time.perf_counter()
        return (t1 - t0, t2 - t1), (count, bucket, tot)

    res = {k: {what: [] for what in sets} for k in fmts}
    reading = {"quantiles_s": [], "total_s": [], "host_read_s": [], "host_quantiles_and_sum_s": []}
    for _ in range(args.rounds):
        for k in fmts:
            for what in sets:
                sets[what].reset()
                res[k][what].append(phase(what, k))
        device_read()                                                      # warm-up
        (tq, tt), dv = device_read()
        (tr, th), hv = host_read()
        if not all(np.array_equal(a, b) for a, b in zip(dv, hv)):
            print("delay_hist_bench: quantiles() / total() differ from the host functions", file=sys.stderr)
            return 1
        reading["quantiles_s"].append(tq)
        reading["total_s"].append(tt)
        reading["host_read_s"].append(tr)
        reading["host_quantiles_and_sum_s"].append(th)
    state_bytes = {what: s.state_bytes for what, s in sets.items()}
    for s in sets.values():
        s.close()
    pool.shutdown()

    engine = None
    try:
        with open(args.engine_record) as f:
            rec = json.loads(f.readline())
        engine = {"source": os.path.relpath(args.engine_record, ROOT), "accesses_per_s": rec["value"],
                  "seconds_per_chunk": R * n / rec["value"]}
    except (OSError, ValueError, KeyError):
        pass

    row_bytes = 2 * A.PU_DHIST_BUCKETS * 8
    line = {"tool": "delay_hist_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "chunk": n, "cores": cores,
            "steps": args.steps, "rounds": args.rounds, "host_threads": args.threads,
            "delays": f"one engine chunk of {args.preset} (DeviceStreamSet kind 4 -> run_device, pu_req16, cold replicas)",
            "engine_chunk_seconds_cold": engine_chunk_s, "replicas_with_error_flags": halted,
            "distinct_counters_per_wave_instruction": keys_per_wave,
            "state_bytes": state_bytes, "engine": engine,
            "histograms_checked": "first and last replica, both formats, equal to the host fold",
            "reading": reading, "reading_checked": "quantiles() and total() equal read() + histogram_quantiles / sum",
            "reading_device_over_host": [(a + b) / (c + d) for a, b, c, d in zip(*reading.values())]}
    for k in fmts:
        t = res[k]
        touched = R * n * BYTES_LINES[k] + R * 2 * row_bytes               # the lines of the loads; the row read and written
        line[k] = {
            "seconds_per_call": t,
            "dhist_over_dsum": [a / b for a, b in zip(t["dhist"], t["dsum_no_tables"])],
            "bytes_of_lines_per_record": BYTES_LINES[k], "row_bytes_read_and_written_per_replica": 2 * row_bytes,
            "share_of_hbm_read_bound": [touched / HBM_READ_BOUND / x for x in t["dhist"]],
            "share_of_engine_time": [x / engine["seconds_per_chunk"] for x in t["dhist"]] if engine else None,
        }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
