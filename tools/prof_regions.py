"""Where the engine's time goes: region cycle counters of the engine kernels.

Runs bench.py's workload on the shipped kernels compiled with s_memtime
stamps (the product library with PRIMEUNCORE_JIT_EXTRA=-DPU_PROF, its own
cache entry; warm it first with the same environment: tools/jit_warm.py) and
prints, per region, the summed per-wave cycles and their share of the
per-request loop.  Regions are inclusive (NET contains NSETUP/NHOPS/NWB, NHOPS
contains NTREE, NTREE contains NWAIT, HOME contains the transmits it makes).

    python tools/prof_regions.py -- --steps 3 --warmup 1 --no-cpu
    python tools/prof_regions.py -- --replicas 1 ...   (latency mode)

(--jit is accepted and ignored: this has been the only mode since the engine
kernels became the compiled configuration's alone.)
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["LOOP", "REQ", "NET", "NSETUP", "NHOPS", "NTREE", "NWAIT", "NWB", "SETL0", "SETLN", "HOME_LD",
         "HOME", "DOWN", "windows", "tree_hops", "demand_hops", "T_LDS", "T_SEARCH", "T_DECIDE", "T_EDIT",
         "T_STORE", "T_REFILL", "NPRE", "NPOST", "MG1RUN", "mg1_lanes", "mg1_cache_hits", "MAINTAIL",
         "mg1_cache_present", "mg1_helper_stored", "mg1_helper_batches", "T_UPD", "mg1_calls",
         "mg1_chain_calls"]
COUNTS = {"windows", "tree_hops", "demand_hops", "mg1_lanes", "mg1_cache_hits", "mg1_cache_present",
          "mg1_helper_stored", "mg1_helper_batches", "mg1_calls", "mg1_chain_calls"}


def main() -> None:
    # the engine kernels with the counters compiled in
    os.environ["PRIMEUNCORE_JIT_EXTRA"] = "-DPU_PROF"
    os.environ["PU_PROF_JIT"] = "1"
    os.environ["PU_PROF_RESET_AFTER_WARMUP"] = "1"
    sys.path.insert(0, ROOT)
    args = [a for a in sys.argv[1:] if a not in ("--", "--jit")]
    import bench  # noqa: E402
    import primesim_amd.uncore as U  # noqa: E402

    sys.argv = ["bench.py", *args]
    try:
        bench.main()
    except SystemExit as e:
        # 3: the grid of the counting build was not all resident, so the rate
        # bench printed is not valid; the counters below still are
        if e.code not in (None, 0, 3):
            raise
        if e.code == 3:
            print("prof_regions: bench's residency check failed (exit 3); counters read all the same", flush=True)
    L = U.lib()
    fn = L.pu_jit_prof_read
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_int]
    buf = (C.c_ulonglong * len(NAMES))()
    if fn(buf, len(NAMES), 0) <= 0:
        raise SystemExit("no region counters read (a kernel built with -DPU_PROF must have run)")
    vals = dict(zip(NAMES, (int(x) for x in buf)))
    loop = max(vals["LOOP"], 1)
    out = {}
    for k, v in vals.items():
        out[k] = v if k in COUNTS else {"cycles": v, "frac_of_loop": round(v / loop, 4)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
