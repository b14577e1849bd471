#!/usr/bin/env python3
"""Time per call of the device lists of slowest requests (DeviceDelayTail,
primesim_amd/csrc/delay_tail.hip) on one chunk of the bench's shape: --replicas replicas x
--chunk records, requests from DeviceStreamSet kind 4 (the bench's stream, seeds from
dist.replica_seed) in both record formats, and delays from ONE ENGINE CHUNK of C4
(run_device over those requests), so the values the kernel compares are spread as the
engine's are, not as a fill's.

  add        `steps` calls per HIP-event window after a warm-up call, with lists of 16 and
             of 64 entries, and as many of DeviceDelayHistogram.add on the same arrays in
             the same run: the yardstick, the parent commit's kernel, which reads the same
             lines.  Two windows per list length, because a set's full lists bar most of a
             later chunk: "first chunk", every add after a reset() (the window holds both;
             a window of resets, each followed by an add of empty ranges, is timed beside it
             and taken off), and "later chunk",
             the same chunk offered again to the lists it has filled, where no record passes
             the stored lists' bar: the cost of a chunk that brings nothing new;
  ascending  the first-chunk window with delays 0, 1, 2, ... per replica, where every record
             is a candidate: the adversarial input, which the engine does not produce;
  reading    wall time of read() and of total() for the whole set, against the host
             alternative: copying requests and delays back (timed on one replica in
             sixteen and scaled).

Before any timing the first and the last replica's lists are compared with the host fold of
their records (delay_tail), in both formats and for both list lengths; the tool exits non-zero
when they differ.  The phases alternate `--rounds` times so the run-to-run spread shows.
Prints one JSON line.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import heapq
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 4            # bench.py's
KS = (16, 64)
FIELDS = ("addr", "timer", "position", "delay", "core")


def candidates_of_a_wave(delays: np.ndarray, cls: np.ndarray, k: int) -> int:
    """Insertions a wave of dtail_add_kernel makes on its records (in the order it meets them): a record
    enters while its class's list is short, afterwards when its delay exceeds the list's k-th."""
    heaps = ([], [])
    made = 0
    for d, c in zip(delays.tolist(), cls.tolist()):
        h = heaps[c]
        if len(h) < k:
            heapq.heappush(h, d)
            made += 1
        elif d > h[0]:
            heapq.heapreplace(h, d)
            made += 1
    return made


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=7168)
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=50, help="timed calls per window")
    ap.add_argument("--ascending-steps", type=int, default=5, help="timed calls per window on ascending delays")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the phases (at least 2)")
    ap.add_argument("--preset", default="C4", help="the engine configuration whose delays are listed")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    args.rounds = max(2, args.rounds)

    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF
    from primesim_amd.dist import replica_seed

    if not torch.cuda.is_available():
        print("delay_tail_bench: no GPU (the device lists have no CPU fallback)", file=sys.stderr)
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
    d_reqs = {f: torch.empty((R, n * rb), dtype=torch.uint8, device=dev) for f, (_, rb) in fmts.items()}
    d_del = torch.zeros((R, n), dtype=torch.int32, device=dev)
    d_asc = torch.arange(n, dtype=torch.int32, device=dev).repeat(R, 1).contiguous()
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n
    torch.cuda.synchronize(dev)
    for f, (fmt, rb) in fmts.items():
        dss = P.DeviceStreamSet(specs)
        dss.next_into(d_reqs[f].data_ptr(), n, fmt=fmt, stream_ptr=sptr)
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

    # what the kernel meets: the insertions of a wave, per record, on a sample of replicas
    pick = list(range(0, R, max(1, R // 8)))[:8]
    cand = {k: [] for k in KS}
    for r in pick:
        d = d_del[r].cpu().numpy()
        words = d_reqs["req16"][r].cpu().numpy().view(np.uint64).reshape(n, 2)[:, 1]
        cls = ((words >> np.uint64(62)) & np.uint64(1)).astype(np.int64)
        wave_of = (np.arange(n) % 256) // 64
        for k in KS:
            cand[k].append(sum(candidates_of_a_wave(d[wave_of == w], cls[wave_of == w], k) for w in range(4)) / n)
    candidates = {f"k{k}": {"insertions_per_record_mean": float(np.mean(v)), "max": float(np.max(v)),
                            "sampled_replicas": len(v)} for k, v in cand.items()}

    sets = {"dtail_k16": P.DeviceDelayTail(R, 16), "dtail_k64": P.DeviceDelayTail(R, 64), "dhist": P.DeviceDelayHistogram(R)}
    tails = {k: sets[f"dtail_k{k}"] for k in KS}

    def add(what: str, f: str, delays=d_del) -> None:
        sets[what].add(d_reqs[f].data_ptr(), delays.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8,
                       fmt=fmts[f][0], stream_ptr=sptr)

    # ---- the device lists are the host fold's, before any timing
    ends = [0, R - 1] if R > 1 else [0]
    for f, (fmt, rb) in fmts.items():
        for k in KS:
            what = f"dtail_k{k}"
            sets[what].reset()
            add(what, f)
            for i in ends:
                ent, cnt = sets[what].read(i, 1)
                recs = d_reqs[f][i].cpu().numpy()
                recs = recs.view(A.REQ_DTYPE) if rb == 32 else recs.view(np.uint64).reshape(n, 2)
                we, wc, _ = P.delay_tail(recs, d_del[i].cpu().numpy(), k, fmt=fmt)
                if not (np.array_equal(cnt[0], wc) and all(np.array_equal(ent[0][x], we[x]) for x in FIELDS)):
                    print(f"delay_tail_bench: replica {i} ({f}, k {k}): the device lists differ from the host fold", file=sys.stderr)
                    return 1

    def window(call, steps: int) -> float:
        call()                                                             # warm-up
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            call()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3 / steps

    def reset_on_stream(what: str) -> None:
        # reset() runs on the set's own stream, ordered after the add before it by the set's event; the
        # add after it waits for it the same way, so the window on `stream` holds both
        sets[what].reset()

    def reset_and_add(what: str, f: str, delays) -> None:
        reset_on_stream(what)
        add(what, f, delays)

    names = [f"dtail_k{k}" for k in KS]
    res = {f: {"dhist": [], **{w: {"first_chunk_with_reset": [], "later_chunk": []} for w in names}} for f in fmts}
    asc = {f: {"dhist": [], **{w: [] for w in names}} for f in fmts}
    resets = {w: [] for w in names}
    reading = {f"k{k}": {"read_s": [], "total_s": []} for k in KS}
    for _ in range(args.rounds):
        for f in fmts:
            sets["dhist"].reset()
            res[f]["dhist"].append(window(lambda: add("dhist", f), args.steps))
            for w in names:
                res[f][w]["first_chunk_with_reset"].append(window(lambda: reset_and_add(w, f, d_del), args.steps))
                res[f][w]["later_chunk"].append(window(lambda: add(w, f), args.steps))
        for w in names:
            # the add that follows a reset in the windows above, here without its work: an empty range per replica
            resets[w].append(window(lambda: (reset_on_stream(w), sets[w].add(
                d_reqs["req16"].data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr(), fmt=fmts["req16"][0],
                stream_ptr=sptr)), args.steps))
        for f in fmts:
            sets["dhist"].reset()
            asc[f]["dhist"].append(window(lambda: add("dhist", f, d_asc), args.ascending_steps))
            for w in names:
                asc[f][w].append(window(lambda: reset_and_add(w, f, d_asc), args.ascending_steps))
        for k in KS:                                                       # the lists of the ascending delays
            tails[k].read(0, 1)
            tails[k].total(0, 1)                                           # warm-up
            t0 = time.perf_counter()
            tails[k].read()
            t1 = time.perf_counter()
            tails[k].total()
            t2 = time.perf_counter()
            reading[f"k{k}"]["read_s"].append(t1 - t0)
            reading[f"k{k}"]["total_s"].append(t2 - t1)
    # the host alternative: every request and delay copied back; one replica in sixteen, scaled
    part = max(1, R // 16)
    copy_back = []
    for _ in range(args.rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        d_reqs["req16"][:part].cpu()
        d_del[:part].cpu()
        copy_back.append((time.perf_counter() - t0) * R / part)
    state_bytes = {what: s.state_bytes for what, s in sets.items()}
    for s in sets.values():
        s.close()

    line = {"tool": "delay_tail_bench", "gpu": torch.cuda.get_device_name(0), "replicas": R, "chunk": n, "cores": cores,
            "steps": args.steps, "ascending_steps": args.ascending_steps, "rounds": args.rounds,
            "delays": f"one engine chunk of {args.preset} (DeviceStreamSet kind 4 -> run_device, pu_req16, cold replicas)",
            "replicas_with_error_flags": halted, "wave_insertions": candidates, "state_bytes": state_bytes,
            "lists_checked": "first and last replica, both formats, k 16 and 64, equal to the host fold",
            "reading": reading,
            "copy_back_pu_req16_and_delays_s_scaled": copy_back, "copy_back_bytes": R * n * 20,
            "copy_back_sampled_replicas": part}
    line["reset_and_an_empty_add_seconds"] = resets
    for f in fmts:
        t, a = res[f], asc[f]
        line[f] = {"seconds_per_call": t, "ascending_seconds_per_call_with_reset": a}
        for w in names:
            first = [x - y for x, y in zip(t[w]["first_chunk_with_reset"], resets[w])]
            line[f][w] = {
                "first_chunk_less_reset": first,
                "first_chunk_over_dhist": [x / y for x, y in zip(first, t["dhist"])],
                "later_chunk_over_dhist": [x / y for x, y in zip(t[w]["later_chunk"], t["dhist"])],
                "ascending_over_dhist": [(x - z) / y for x, y, z in zip(a[w], a["dhist"], resets[w])],
            }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
