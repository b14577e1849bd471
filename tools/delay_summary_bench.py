#!/usr/bin/env python3
"""Records per second of the device delay summaries (DeviceDelaySummary,
primesim_amd/csrc/delay_sum.hip) against the host path they replace, on one chunk of
the bench's shape: --replicas replicas x --chunk records, 1,024 cores, requests from
DeviceStreamSet kind 4 (the bench's stream, seeds from dist.replica_seed), delays a
fixed pseudo-random fill (the summary's speed does not depend on their being real).

  device   `steps` calls of add per record format, with per-core tables and without,
           timed by HIP events around the calls and ended by a synchronise;
  host     what a user has without the device summaries: the delays and the request
           words the fold needs (pu_req16: b, 8 B; pu_req: its second half, 16 B)
           gathered on the device, copied to pinned host memory, and folded by numpy
           into the same per-replica and per-core figures on the job's host threads;
           a host clock around the copies and the fold.  --host-replicas bounds how
           many of the replicas the host phase takes (rates are per record).

Before any timing the first and the last replica's device summaries and per-core
tables are compared with the host fold of their records (pu_dsum_host_add), in both
formats; the tool exits non-zero when they differ.  Device and host phases alternate
`--rounds` times (each after a warm-up call of its own) so the run-to-run spread
shows.  Prints one JSON line.  Needs a GPU: there is no CPU fallback.
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
CORES = 1024
HBM_READ_BOUND = 8e12    # bytes per second
# bytes a record makes the kernel ask for (delay + the request words it loads), and the bytes of the
# whole lines those loads touch (the request records are read in full lines: 16 or 32 B a record)
BYTES_ASKED = {"req32": 4 + 16, "req16": 4 + 8}
BYTES_LINES = {"req32": 4 + 32, "req16": 4 + 16}
HOST_GROUP = 64          # replicas a host thread folds at a time
THRESHOLDS = (1 << np.arange(31, dtype=np.int64)).astype(np.int32)


def host_fold(words: np.ndarray, delays: np.ndarray, rb: int):
    """The numpy fold of a group of replicas: words [g, n] (pu_req16.b) or [g, n, 2] (the second half
    of a pu_req), delays [g, n].  Returns (count, sum, min, max, hist, core_out_of_range, core_count, core_sum)."""
    g, n = delays.shape
    if rb == 16:
        wr = ((words >> np.uint64(62)) & np.uint64(1)).astype(np.int64)
        core = ((words >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int64)
    else:
        wr = ((words[..., 1] & np.uint64(0xFF)) == np.uint64(1)).astype(np.int64)
        core = (words[..., 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64)
    d = delays.astype(np.int64)
    bucket = np.searchsorted(THRESHOLDS, delays.reshape(-1), side="right").reshape(g, n)
    row = np.arange(g, dtype=np.int64)[:, None]
    hist = np.bincount((row * 64 + wr * 32 + bucket).reshape(-1), minlength=g * 64).reshape(g, 2, 32)
    count = hist.sum(axis=2)
    sums = np.stack([np.where(wr == c, d, 0).sum(axis=1) for c in (0, 1)], axis=1)
    mins = np.stack([np.where(wr == c, delays, np.iinfo(np.int32).max).min(axis=1) for c in (0, 1)], axis=1)
    maxs = np.stack([np.where(wr == c, delays, np.iinfo(np.int32).min).max(axis=1) for c in (0, 1)], axis=1)
    ok = (core >= 0) & (core < CORES)
    oor = n - ok.sum(axis=1)
    key = (row * CORES + np.where(ok, core, 0)).reshape(-1)
    okf = ok.reshape(-1)
    core_count = np.bincount(key[okf], minlength=g * CORES).reshape(g, CORES)
    # float64 weights are exact here: a core's delays sum far below 2^53
    core_sum = np.bincount(key[okf], weights=d.reshape(-1)[okf], minlength=g * CORES).astype(np.int64).reshape(g, CORES)
    return count, sums, mins, maxs, hist, oor, core_count, core_sum


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=50, help="timed device calls per format, variant and phase")
    ap.add_argument("--host-replicas", type=int, default=1792, help="replicas the host phase copies and folds")
    ap.add_argument("--rounds", type=int, default=2, help="device/host alternations (at least 2)")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="host fold threads")
    ap.add_argument("--engine-record", default=os.path.join(ROOT, "profiles", "r8_bench.json"),
                    help="a bench.py result line: the engine's rate on this shape")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("delay_summary_bench: no GPU (the device summaries have no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    R, n = args.replicas, args.chunk
    HR = min(R, args.host_replicas)
    fmts = {"req32": (A.PU_REQ_FMT_32, 32), "req16": (A.PU_REQ_FMT_16, 16)}
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream

    # ---- the chunk: requests of both formats from the device generator, delays a fixed fill
    specs = [P.StreamSpec(A.PU_STREAM_UNIFORM_HOTSPOT, CORES, seed=replica_seed(SEED_BASE, 0, r), num_quanta=64)
             for r in range(R)]
    d_reqs = {k: torch.empty((R, n * rb), dtype=torch.uint8, device=dev) for k, (_, rb) in fmts.items()}
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    d_del = torch.randint(-1, 700, (R, n), dtype=torch.int32, device=dev, generator=gen)
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
    torch.cuda.synchronize(dev)
    for k, (fmt, rb) in fmts.items():
        dss = P.DeviceStreamSet(specs)
        dss.next_into(d_reqs[k].data_ptr(), n, fmt=fmt, stream_ptr=sptr)
        assert int(dss.positions().min()) == n
        dss.close()
    stream.synchronize()

    sets = {True: P.DeviceDelaySummary(R, num_cores=[CORES] * R), False: P.DeviceDelaySummary(R)}

    def add(k: str, tables: bool) -> None:
        sets[tables].add(d_reqs[k].data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8,
                         fmt=fmts[k][0], stream_ptr=sptr)

    # ---- the device summaries are the host fold's, before any timing
    ends = [0, R - 1] if R > 1 else [0]
    for k, (fmt, rb) in fmts.items():
        for tables in (True, False):
            sets[tables].reset()
            add(k, tables)
            for i in ends:
                got = sets[tables].read(i, 1)[0]
                recs = d_reqs[k][i].cpu().numpy()
                recs = recs.view(A.REQ_DTYPE) if rb == 32 else recs.view(np.uint64).reshape(n, 2)
                want, cnt, sm = P.summarize_delays(recs, d_del[i].cpu().numpy(), num_cores=CORES if tables else None,
                                                   fmt=fmt)
                same = got.tobytes() == want.tobytes()
                if tables:
                    c, s = sets[tables].cores(i)
                    same = same and np.array_equal(c, cnt) and np.array_equal(s, sm)
                if not same:
                    print(f"delay_summary_bench: replica {i} ({k}, tables {tables}): the device summary differs "
                          "from the host fold", file=sys.stderr)
                    return 1

    # ---- (a) the device path
    def device_phase(k: str, tables: bool) -> float:
        add(k, tables)                                                     # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            add(k, tables)
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3 / args.steps

    # ---- (b) the host path: gather the words on the device, pinned copies, the numpy fold
    pin_del = torch.empty((HR, n), dtype=torch.int32, pin_memory=True)
    pin_w = {"req16": torch.empty((HR, n), dtype=torch.int64, pin_memory=True),
             "req32": torch.empty((HR, n, 2), dtype=torch.int64, pin_memory=True)}
    pool = ThreadPoolExecutor(args.threads)

    def host_chunk(k: str):
        rb = fmts[k][1]
        words = d_reqs[k][:HR].view(torch.int64).view(HR, n, rb // 8)
        words = words[:, :, 1].contiguous() if rb == 16 else words[:, :, 2:4].contiguous()
        pin_w[k].copy_(words, non_blocking=True)
        pin_del.copy_(d_del[:HR], non_blocking=True)
        torch.cuda.synchronize(dev)
        w, d = pin_w[k].numpy().view(np.uint64), pin_del.numpy()
        groups = [(a, min(a + HOST_GROUP, HR)) for a in range(0, HR, HOST_GROUP)]
        return list(pool.map(lambda az: host_fold(w[az[0]:az[1]], d[az[0]:az[1]], rb), groups))

    def host_phase(k: str) -> float:
        host_chunk(k)                                                      # warm-up
        t0 = time.perf_counter()
        parts = host_chunk(k)
        dt = time.perf_counter() - t0
        # the host fold agrees with the device (one add since the reset) on the first replica's histogram
        got = sets[True].read(0, 1)[0]
        assert np.array_equal(parts[0][4][0], got["cls"]["hist"].astype(np.int64)), "host fold differs from the device"
        return dt

    res = {"device": {k: {True: [], False: []} for k in fmts}, "host": {k: [] for k in fmts}}
    for _ in range(args.rounds):
        for k in fmts:
            for tables in (True, False):
                sets[tables].reset()
                res["device"][k][tables].append(device_phase(k, tables))
        for k in fmts:
            sets[True].reset()
            add(k, True)
            res["host"][k].append(host_phase(k))
    state_bytes = {"with_tables": sets[True].state_bytes, "without": sets[False].state_bytes}
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

    line = {"tool": "delay_summary_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "chunk": n, "cores": CORES,
            "steps": args.steps, "rounds": args.rounds, "host_replicas": HR, "host_threads": args.threads,
            "mapping": "one workgroup of 256 per replica, lanes take consecutive records",
            "state_bytes": state_bytes, "engine": engine,
            "summaries_checked": "first and last replica, both formats, with and without tables, equal to the host fold"}
    for k in fmts:
        t_tab, t_no = res["device"][k][True], res["device"][k][False]
        rate = [R * n / t for t in t_tab]
        host_rate = [HR * n / t for t in res["host"][k]]
        line[k] = {
            "device_seconds_per_chunk": t_tab, "device_seconds_per_chunk_without_tables": t_no,
            "device_records_per_s": rate, "device_records_per_s_without_tables": [R * n / t for t in t_no],
            "host_seconds": res["host"][k], "host_records_per_s": host_rate,
            "bytes_asked_per_record": BYTES_ASKED[k], "bytes_of_lines_per_record": BYTES_LINES[k],
            "device_share_of_hbm_read_bound_asked": [x * BYTES_ASKED[k] / HBM_READ_BOUND for x in rate],
            "device_share_of_hbm_read_bound_lines": [x * BYTES_LINES[k] / HBM_READ_BOUND for x in rate],
            "tables_cost_factor": [a / b for a, b in zip(t_tab, t_no)],
            "device_over_host_worst_case": min(rate) / max(host_rate),
            "device_share_of_engine_time": [t / engine["seconds_per_chunk"] for t in t_tab] if engine else None,
        }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
