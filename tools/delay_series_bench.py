#!/usr/bin/env python3
"""Time per call of the device epoch series (DeviceDelaySeries,
primesim_amd/csrc/delay_series.hip) on one chunk of the bench's shape: --replicas
replicas x --chunk records, requests from DeviceStreamSet kind 4 (the bench's stream,
seeds from dist.replica_seed) in both record formats, and delays from ONE ENGINE CHUNK
of C4 (run_device over those requests), so the timers and delays the kernel folds are the
engine's own, not a fill's.

  add        `steps` calls per HIP-event window after a warm-up call, at E = 64 and E = 512
             epochs (t0 = 0, the shift at which the chunk's largest timer lies in the upper
             half of the epochs), and as many of DeviceDelayHistogram.add on the same arrays
             in the same run: the yardstick, the parent commit's kernel, which touches the
             same record lines.  The bar for a call is dhist's time scaled by the ratio of
             the bytes the two touch (the record lines plus the replica's row read and
             written: 2 * 64 E bytes here against 2 * 13,824 there), plus 5 %.

Before any timing the first and the last replica's cells are compared with the host fold
of their records (delay_series), in both formats and at both epoch counts; the tool exits
non-zero when they differ.  The phases alternate `--rounds` times so the run-to-run spread
shows.  Prints one JSON line.  Needs a GPU: there is no CPU fallback.
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

SEED_BASE = 4            # bench.py's
HBM_READ_BOUND = 8e12    # bytes per second
# the bytes of the whole lines the loads of a record touch (the request records are read in full
# lines: 16 or 32 B a record; 4 B of delay), as DESIGN.md section 6b counts them
BYTES_LINES = {"req32": 4 + 32, "req16": 4 + 16}
EPOCHS = (64, 512)
BAR = 1.05


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=50, help="timed calls per window")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the phases (at least 2)")
    ap.add_argument("--preset", default="C4", help="the engine configuration whose delays are folded")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("delay_series_bench: no GPU (the device epoch series have no CPU fallback)", file=sys.stderr)
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
        um.run_device(d_reqs["req16"].data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sptr)
        stream.synchronize()
        halted = int((np.asarray(um.error_flags(R)) != 0).sum())
    finally:
        um.close()

    # ---- the epochs: from 0 on, the chunk's largest timer in the upper half of the epochs
    words = d_reqs["req16"][:: max(1, R // 64)].cpu().numpy().view(np.uint64).reshape(-1, n, 2)[:, :, 1]
    timer = (words & np.uint64((1 << 40) - 1)).astype(np.int64)
    cls = ((words >> np.uint64(62)) & np.uint64(1)).astype(np.int64)
    tmax = int(timer.max())
    shift = {E: next(s for s in range(63) if (tmax >> s) < E) for E in EPOCHS}

    # what the kernel meets: distinct cells per wave instruction (64 consecutive records), on a sample
    cells_per_wave = {}
    for E in EPOCHS:
        key = cls * E + np.minimum(timer >> shift[E], E - 1)
        srt = np.sort(key[:, : n - n % 64].reshape(len(key), -1, 64), axis=2)
        distinct = 1 + (srt[:, :, 1:] != srt[:, :, :-1]).sum(axis=2)
        cells_per_wave[f"E{E}"] = {"shift": shift[E], "mean": float(distinct.mean()), "median": float(np.median(distinct)),
                                   "share_at_most_4": float((distinct <= 4).mean()), "max": int(distinct.max()),
                                   "live_cells_of_a_replica_mean": float(np.mean([len(np.unique(k)) for k in key])),
                                   "sampled_replicas": len(key)}

    sets = {f"dseries_E{E}": P.DeviceDelaySeries(R, E, t0=0, shift=shift[E]) for E in EPOCHS}
    sets["dhist"] = P.DeviceDelayHistogram(R)

    def add(what: str, k: str) -> None:
        sets[what].add(d_reqs[k].data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8,
                       fmt=fmts[k][0], stream_ptr=sptr)

    # ---- the device cells are the host fold's, before any timing
    ends = [0, R - 1] if R > 1 else [0]
    for k, (fmt, rb) in fmts.items():
        for E in EPOCHS:
            what = f"dseries_E{E}"
            sets[what].reset()
            add(what, k)
            for i in ends:
                got = sets[what].read(i, 1)[0]
                recs = d_reqs[k][i].cpu().numpy()
                recs = recs.view(A.REQ_DTYPE) if rb == 32 else recs.view(np.uint64).reshape(n, 2)
                want = P.delay_series(recs, d_del[i].cpu().numpy(), E, 0, shift[E], fmt=fmt)
                if got.tobytes() != want.tobytes():
                    print(f"delay_series_bench: replica {i} ({k}, E = {E}): the device cells differ from the host fold",
                          file=sys.stderr)
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

    res = {k: {what: [] for what in sets} for k in fmts}
    for _ in range(args.rounds):
        for k in fmts:
            for what in sets:
                sets[what].reset()
                res[k][what].append(phase(what, k))
    state_bytes = {what: s.state_bytes for what, s in sets.items()}
    for s in sets.values():
        s.close()

    hist_row = 2 * 2 * A.PU_DHIST_BUCKETS * 8                              # read and written
    line = {"tool": "delay_series_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "chunk": n, "cores": cores,
            "steps": args.steps, "rounds": args.rounds,
            "delays": f"one engine chunk of {args.preset} (DeviceStreamSet kind 4 -> run_device, pu_req16, cold replicas)",
            "replicas_with_error_flags": halted, "largest_timer": tmax, "t0": 0,
            "distinct_cells_per_wave_instruction": cells_per_wave, "state_bytes": state_bytes,
            "cells_checked": "first and last replica, both formats, E = 64 and 512, equal to the host fold",
            "bar": "dhist's seconds per call * bytes touched here / bytes touched there * 1.05"}
    for k in fmts:
        t = res[k]
        hist_bytes = R * n * BYTES_LINES[k] + R * hist_row
        line[k] = {"seconds_per_call": t, "bytes_of_lines_per_record": BYTES_LINES[k],
                   "dhist_share_of_hbm_read_bound": [hist_bytes / HBM_READ_BOUND / x for x in t["dhist"]]}
        for E in EPOCHS:
            what = f"dseries_E{E}"
            touched = R * n * BYTES_LINES[k] + R * 2 * 64 * E
            over = [a / b for a, b in zip(t[what], t["dhist"])]
            line[k][f"E{E}"] = {"row_bytes_read_and_written_per_replica": 2 * 64 * E, "bytes_ratio_to_dhist": touched / hist_bytes,
                                "dseries_over_dhist": over, "bar_ratio": BAR * touched / hist_bytes,
                                "bar_met": [x <= BAR * touched / hist_bytes for x in over],
                                "share_of_hbm_read_bound": [touched / HBM_READ_BOUND / x for x in t[what]]}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
