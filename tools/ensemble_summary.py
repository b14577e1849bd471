#!/usr/bin/env python3
"""An ensemble of independent simulations that never leaves the device: per chunk
DeviceStreamSet.next_into -> UncoreManager.run_device -> DeviceDelaySummary.add, all
on one torch stream.  No request and no delay is copied to the host; the only
device-to-host traffic is the summaries (568 B per replica) and the error flags.

Prints one JSON line per replica: requests, mean read and write latency, the upper
bounds of the histogram buckets that hold the median and the 99th percentile of each
class (a bucket b > 0 holds delays 2^(b-1) .. 2^b - 1; bucket 0 holds delays <= 0),
cores out of range and the engine's error flags.  Needs a GPU: there is no CPU fallback.

  python tools/ensemble_summary.py --preset C1 --kind 1 --replicas 4 --chunk 2000 --chunks 2

With --results the end-of-run results are gathered on the device too, once, after the
last chunk (DeviceRunResults.gather on the same stream; 448 B per replica more): every
replica's line gains a "results" object -- requests, the simulated end cycle, link
visits, the busiest link with its two ends, network and DRAM counters -- and one last
line lists the ensemble's ten busiest links, by visits summed over the replicas.

With --quantiles a log-linear delay histogram is kept on the device as well
(DeviceDelayHistogram.add on the same stream, after the summary's add; 13,824 B per
replica): every replica's "read" and "write" objects gain "p50", "p90", "p99" and
"p999", each {"ge": lo, "le": hi}, the bounds of the histogram bucket that holds the
quantile (exact below 64 cycles, within 3.2 % above; null for an empty class), read
from the histogram on the device, and one last line carries the same for the histogram
summed over the replicas.

With --tail K the K slowest reads and the K slowest writes of every replica are kept on the
device too (DeviceDelayTail.add on the same stream, after the summary's add and the
histogram's; 64 K + 16 B per replica): every replica's "read" and "write" objects gain
"slowest", a list of {"delay", "core", "addr", "timer", "position"}, the worst first
(position: the request's place among the replica's measured requests), and one last line
carries the K slowest of the whole ensemble with the "replica" of each.

With --series E:SHIFT[:T0] the delays are kept over simulated time on the device as well
(DeviceDelaySeries.add on the same stream, after the other stages' adds; 64 E bytes per
replica): epochs of 2^SHIFT cycles of the requests' own timers from T0 (default 0) on, the
first and the last of the E epochs catching everything before and after.  Every replica's
"read" and "write" objects gain "series": {"count": [...], "sum": [...], "max": [...],
"nonpos": [...]}, E entries each (nonpos: the delays <= 0; the mean of an epoch is sum /
count), and one last line carries the same for the cells merged over the replicas.

With --warmup-chunks K the cold start is simulated once: replica 0 alone runs K chunks of
stream 0 (the other replicas get empty ranges; nothing goes to the summaries,
histograms, lists of the slowest or series), then every other replica becomes a copy of it (UncoreManager.fork_replica)
and every other stream continues from stream 0's position with its own seed
(DeviceStreamSet.fork), all on the same stream, and the --chunks measured chunks run as
usual.  The forks share their warm-up: they are correlated until their own streams have
displaced it, and engine counters ("results", error flags) include the warm-up's.

With --msglog PATH (instead of --kind) the requests are one recorded MsgMem message log,
read once (msglog_read over the configuration's cores) and replayed on the device for every
replica (DeviceTraceSet.next_into in place of DeviceStreamSet's): --placement-seed S runs
replica r under row r of random_placements(replicas, cores, S), --skew-max K adds to every
core of replica r > 0 a start skew drawn from [0, K] (numpy's default_rng([S, r]); S = 0
without --placement-seed); replica 0 always runs the trace as recorded.  Every line carries
"placement_seed" (placement_seed(S, r); 0 is the identity) in place of "seed".  --chunks
chunks of --chunk requests must lie inside the log.  --warmup-chunks runs replica 0 alone on
the log's first chunks, forks it to the others, and all continue from the same position: the
cursor is the set's, so there is no stream to fork.

  python tools/ensemble_summary.py --preset C1 --msglog run.msglog --replicas 8 --placement-seed 5
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bucket_upper(b: int) -> int:
    """The largest delay of bucket b (0 for the bucket of the non-positive delays)."""
    return 0 if b == 0 else (1 << b) - 1


def percentile_bound(hist, pct: int):
    """Upper bound of the first bucket at which the running count reaches pct percent; None for an empty class."""
    total = int(hist.sum())
    if total == 0:
        return None
    need, run = -(-total * pct // 100), 0
    for b, h in enumerate(hist):
        run += int(h)
        if run >= need:
            return bucket_upper(b)
    return bucket_upper(len(hist) - 1)


def replica_line(r: int, seed: int, s, flags: int) -> dict:
    line = {"replica": r, "seed": seed, "requests": int(s["cls"]["count"].sum())}
    for c, name in enumerate(("read", "write")):
        k = s["cls"][c]
        n = int(k["count"])
        line[name] = {"count": n, "sum": int(k["sum"]), "mean": int(k["sum"]) / n if n else None,
                      "min": int(k["min"]) if n else None, "max": int(k["max"]) if n else None,
                      "p50_le": percentile_bound(k["hist"], 50), "p99_le": percentile_bound(k["hist"], 99)}
    line["core_out_of_range"] = int(s["core_out_of_range"])
    line["error_flags"] = flags
    return line


QUANTILES = (("p50", 500000), ("p90", 900000), ("p99", 990000), ("p999", 999000))     # name, parts per million
QUANTILE_PPM = [ppm for _, ppm in QUANTILES]


def quantile_object(buckets) -> dict:
    """One class's answering buckets of QUANTILES (histogram_quantiles / DeviceDelayHistogram.quantiles)
    as {"p50": {"ge": lo, "le": hi}, ...}; null for the -1 of an empty class."""
    import primesim_amd as P
    out = {}
    for (name, _), b in zip(QUANTILES, buckets):
        if int(b) < 0:
            out[name] = None
        else:
            lo, hi = P.dhist_bucket_bounds(int(b))
            out[name] = {"ge": lo, "le": hi}
    return out


def total_line(replicas: int, counts, buckets) -> dict:
    """The last line of --quantiles: the quantiles of the histogram summed over the replicas, per class."""
    return {"replicas": replicas,
            "quantiles": {name: {"count": int(counts[c]), **quantile_object(buckets[c])}
                          for c, name in enumerate(("read", "write"))}}


def slowest_list(entries, count, replicas=None) -> list:
    """One class's list of slowest requests (A.DTAIL_DTYPE entries, the first `count` of them), the worst first."""
    out = []
    for i in range(int(count)):
        e = entries[i]
        item = {"delay": int(e["delay"]), "core": int(e["core"]), "addr": hex(int(e["addr"])), "timer": int(e["timer"]),
                "position": int(e["position"])}
        if replicas is not None:
            item = {"replica": int(replicas[i]), **item}
        out.append(item)
    return out


def tail_total_line(replicas: int, entries, reps, counts) -> dict:
    """The last line of --tail: the slowest requests of the ensemble (DeviceDelayTail.total), per class."""
    return {"replicas": replicas,
            "slowest": {name: slowest_list(entries[c], counts[c], reps[c]) for c, name in enumerate(("read", "write"))}}


def series_object(cells) -> dict:
    """One class's epoch series (A.DSERIES_DTYPE cells, one per epoch) as the "series" object."""
    return {f: [int(v) for v in cells[f]] for f in ("count", "sum", "max", "nonpos")}


def series_total_line(replicas: int, epochs: int, shift: int, t0: int, cells) -> dict:
    """The last line of --series: the cells merged over the replicas (DeviceDelaySeries.total), per class."""
    return {"replicas": replicas,
            "series": {"epochs": epochs, "shift": shift, "t0": t0,
                       **{name: series_object(cells[c]) for c, name in enumerate(("read", "write"))}}}


def link_entry(cfg, q: int, visits: int, block_visits=None) -> dict:
    """Queue q of the configuration with its ends (pu_config_queue_ends) and its visit count."""
    import primesim_amd as P
    from primesim_amd import uncore as U
    kind, a, b = P.queue_ends(cfg, q)
    e = {"id": q, "kind": U.QUEUE_KINDS[kind] if kind >= 0 else None, "a": a, "b": b, "visits": int(visits)}
    if block_visits is not None:
        e["block_visits"] = int(block_visits)
    return e


def results_object(cfg, rec) -> dict:
    """One replica's end-of-run record (A.DRES_DTYPE) as the "results" object of its line."""
    st, done = rec["stats"], int(rec["cores_done"])
    return {"requests": int(st["requests"]), "processed": int(rec["processed"]), "halted": int(rec["halted"]),
            "cores_done": done, "end_cycle": int(rec["completion_max"]) if done else None,
            "link_visits": int(rec["link_visits"]), "link_block_visits": int(rec["link_block_visits"]),
            "links_used": int(rec["links_used"]),
            "hottest_link": link_entry(cfg, int(rec["link_max_id"]), rec["link_max_visits"])
            if int(rec["link_max_id"]) >= 0 else None,
            "bus_visits": int(rec["bus_visits"]),
            "net_accesses": int(st["net_accesses"]), "net_distance": int(st["net_distance"]),
            "net_total_delay": int(st["net_total_delay"]), "link_flits": int(st["link_flits"]),
            "dram_accesses": int(st["dram_accesses"])}


def hottest_links(cfg, n, n1, nlinks: int, top: int = 10) -> list:
    """The `top` links with the most visits (lowest id first among equals), from per-queue totals."""
    order = sorted(range(nlinks), key=lambda q: (-int(n[q]), q))[:top]
    return [link_entry(cfg, q, n[q], n1[q]) for q in order]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--preset", default="C1", help="C1 .. C5 (primesim_amd.config.preset)")
    g.add_argument("--xml", help="a config_prime XML file instead of a preset")
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--kind", type=int, default=4, help="PU_STREAM_* kind of the synthetic streams (1 .. 6)")
    src.add_argument("--msglog", help="a recorded MsgMem message log to replay instead of synthetic streams")
    ap.add_argument("--placement-seed", type=int, default=None,
                    help="with --msglog: replica r runs under row r of random_placements(replicas, cores, seed)")
    ap.add_argument("--skew-max", type=int, default=0,
                    help="with --msglog: per-core start skew of replicas 1 .., drawn from [0, skew-max]")
    ap.add_argument("--replicas", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=2000, help="requests per replica and chunk")
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--seed-base", type=int, default=1, help="replica r streams with seed seed-base + r")
    ap.add_argument("--fmt", type=int, choices=(32, 16), default=32, help="device request records: pu_req or pu_req16")
    ap.add_argument("--results", action="store_true", help="also gather the end-of-run results on the device")
    ap.add_argument("--quantiles", action="store_true",
                    help="also keep a log-linear delay histogram on the device and print p50 / p90 / p99 / p99.9")
    ap.add_argument("--tail", type=int, default=0, metavar="K",
                    help="also keep every replica's K slowest reads and writes on the device (1 .. 64)")
    ap.add_argument("--series", metavar="E:SHIFT[:T0]",
                    help="also keep the delays per epoch of 2^SHIFT cycles from T0 on the device (E of 1 .. 512 epochs)")
    ap.add_argument("--warmup-chunks", type=int, default=0,
                    help="warm replica 0 alone for this many chunks, then fork it and its stream to the others")
    args = ap.parse_args()
    if not args.msglog and (args.placement_seed is not None or args.skew_max):
        ap.error("--placement-seed and --skew-max go with --msglog")
    if not 0 <= args.tail <= 64:
        ap.error("--tail takes a list length of 1 .. 64")
    series = None
    if args.series:
        try:
            series = [int(v) for v in args.series.split(":")]
        except ValueError:
            series = []
        if len(series) == 2:
            series.append(0)
        if len(series) != 3 or not 1 <= series[0] <= 512 or not 0 <= series[1] <= 62 or not -(1 << 63) <= series[2] < 1 << 63:
            ap.error("--series takes E:SHIFT[:T0], E of 1 .. 512 epochs of 2^SHIFT cycles (SHIFT of 0 .. 62) from T0")

    import numpy as np
    import torch

    import primesim_amd as P
    from primesim_amd import _abi as A
    from primesim_amd import config as CF

    if not torch.cuda.is_available():
        print("ensemble_summary: no GPU (the device pipeline has no CPU fallback)", file=sys.stderr)
        return 2
    cfg = P.load_config(args.xml) if args.xml else P.config_from_dict(CF.preset(args.preset))
    R, n, nc = args.replicas, args.chunk, cfg.sys.num_cores
    fmt, rec = (A.PU_REQ_FMT_16, 16) if args.fmt == 16 else (A.PU_REQ_FMT_32, 32)
    quantum = cfg.thread_sync_interval
    # a core issues at least quantum / 4 requests a quantum: enough quanta for every chunk
    quanta = -(-n * (args.chunks + args.warmup_chunks) * 4 // (nc * quantum)) + 1
    specs = [P.StreamSpec(args.kind, nc, seed=args.seed_base + r, quantum=quantum, num_quanta=quanta,
                          max_msg=cfg.max_msg_size) for r in range(R)]

    dev = torch.device("cuda", 0)
    d_reqs = torch.empty((R, n, rec), dtype=torch.uint8, device=dev)
    d_del = torch.empty((R, n), dtype=torch.int32, device=dev)
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * n      # replica r owns records [r*n, (r+1)*n)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)                                     # one stream orders the three stages
    sp = stream.cuda_stream

    um = P.UncoreManager()
    um.init(cfg, replicas=R)
    if args.msglog:
        # the log's threads take their cores from the handle's scheduler as they appear (prime.cpp)
        trace = P.msglog_read(args.msglog, um)
        pseed = args.placement_seed or 0
        seeds = [P.placement_seed(pseed, r) if args.placement_seed is not None else 0 for r in range(R)]
        place = P.random_placements(R, nc, pseed) if args.placement_seed is not None else None
        skews = None
        if args.skew_max > 0:
            skews = np.zeros((R, nc), dtype=np.int32)
            for r in range(1, R):
                skews[r] = np.random.default_rng([pseed, r]).integers(0, args.skew_max + 1, nc)
        dss = P.DeviceTraceSet(trace, nc, R, placements=place, skews=skews)
    else:
        seeds = [args.seed_base + r for r in range(R)]
        dss = P.DeviceStreamSet(specs)
    dsum = P.DeviceDelaySummary(R, num_cores=[nc] * R)
    dres = P.DeviceRunResults(um) if args.results else None
    dhist = P.DeviceDelayHistogram(R) if args.quantiles else None
    dtail = P.DeviceDelayTail(R, args.tail) if args.tail else None
    dseries = P.DeviceDelaySeries(R, series[0], t0=series[2], shift=series[1]) if series else None
    records = totals = qbuckets = total = tails = tail_total = cells = cells_total = None
    nlinks = 0
    try:
        if not args.msglog:
            for prog, th in P.stream_threads(specs[0]):
                um.allocCore(prog, th)
        um.set_device_req_format(fmt)
        if args.warmup_chunks > 0:
            d_warm = d_off.clamp(max=n)                                 # replica 0: [0, n); every other: empty
            torch.cuda.synchronize(dev)                                 # made on torch's stream, read on ours
            for _ in range(args.warmup_chunks):
                dss.next_into(d_reqs.data_ptr(), n, fmt=fmt, stream_ptr=sp)
                um.run_device(d_reqs.data_ptr(), d_warm.data_ptr(), d_del.data_ptr(), sp)
            um.fork_replica(0, stream_ptr=sp)
            if not args.msglog:                                         # a trace set has one cursor: nothing to fork
                dss.fork(0, seeds=seeds, stream_ptr=sp)
        for _ in range(args.chunks):
            dss.next_into(d_reqs.data_ptr(), n, fmt=fmt, stream_ptr=sp)
            um.run_device(d_reqs.data_ptr(), d_off.data_ptr(), d_del.data_ptr(), sp)
            dsum.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt, stream_ptr=sp)
            if dhist is not None:
                dhist.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt,
                          stream_ptr=sp)
            if dtail is not None:
                dtail.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt,
                          stream_ptr=sp)
            if dseries is not None:
                dseries.add(d_reqs.data_ptr(), d_del.data_ptr(), d_off.data_ptr(), d_off.data_ptr() + 8, fmt=fmt,
                            stream_ptr=sp)
        if dres is not None:
            dres.gather(stream_ptr=sp)                                  # one launch, after the last chunk
        summaries = dsum.read()                                         # waits for the last add
        if dres is not None:
            records = dres.read()                                       # waits for the gather
            totals = dres.queue_totals()
            nlinks = dres.num_links
        if dhist is not None:
            _, qbuckets = dhist.quantiles(QUANTILE_PPM)                 # waits for the last add
            total = P.histogram_quantiles(dhist.total(), QUANTILE_PPM)
        if dtail is not None:
            tails = dtail.read()                                        # waits for the last add
            tail_total = dtail.total()
        if dseries is not None:
            cells = dseries.read()                                      # waits for the last add
            cells_total = dseries.total()
        stream.synchronize()
        served = dss.position() if args.msglog else int(dss.positions().min())
        if served != n * (args.chunks + args.warmup_chunks):
            print("ensemble_summary: a stream (or the message log) ended before its last chunk", file=sys.stderr)
            return 1
        flags = um.error_flags(R)
    finally:
        if dres is not None:
            dres.close()
        if dhist is not None:
            dhist.close()
        if dtail is not None:
            dtail.close()
        if dseries is not None:
            dseries.close()
        dsum.close()
        dss.close()
        um.close()
    for r in range(R):
        line = replica_line(r, seeds[r], summaries[r], int(flags[r]))
        if args.msglog:
            line["placement_seed"] = line.pop("seed")
        if qbuckets is not None:
            for c, name in enumerate(("read", "write")):
                line[name].update(quantile_object(qbuckets[r][c]))
        if tails is not None:
            for c, name in enumerate(("read", "write")):
                line[name]["slowest"] = slowest_list(tails[0][r][c], tails[1][r][c])
        if cells is not None:
            for c, name in enumerate(("read", "write")):
                line[name]["series"] = series_object(cells[r][c])
        if records is not None:
            line["results"] = results_object(cfg, records[r])
        print(json.dumps(line))
    if records is not None:
        print(json.dumps({"replicas": R, "hottest_links": hottest_links(cfg, totals[0], totals[1], nlinks)}))
    if total is not None:
        print(json.dumps(total_line(R, total[0], total[1])))
    if tail_total is not None:
        print(json.dumps(tail_total_line(R, *tail_total)))
    if cells_total is not None:
        print(json.dumps(series_total_line(R, series[0], series[1], series[2], cells_total)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
