"""Small random configurations, drawn from one fixed seed: the one source of
the draws for tests/test_config_sweep_oracle.py (the CPU restatement against
the reference, on the CPU), tests/test_gpu_config_sweep.py (the engine kernels
against the restatement, on the GPU) and the build-time warm-up
(tools/jit_warm.py compiles `sweep_configs()`).  It holds the draw (in the
test's process; no GPU) and, for the CPU sweep, one trial (a child process of
its own, because the reference can crash where it is undefined):

    python tests/config_sweep.py <trial directory>

A trial directory holds config.xml, cfg.bin (the library's parse of it),
reqs.npy and trial.json (threads, replay mode).  The child loads the two
oracles only: the CPU restatement runs first and, unless it raises a
reference-undefined flag, the reference runs the same stream; every delay, the
return code and the completion cycles must be equal.  It prints one JSON line.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20260
TRIALS = 64
CORES = (1, 2, 3, 4, 8, 9, 12, 16, 27, 36, 64, 70)
PU_ENOTSUP = -95   # include/primeuncore.h


def geometry_rc(sim: dict) -> tuple:
    """pu::config_geometry's code and text (pu_config_queue_ends returns both as they are)."""
    import primesim_amd as P
    cfg = P.config_from_dict(sim)
    kind, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = P.uncore.lib().pu_config_queue_ends(C.byref(cfg), 0, C.byref(kind), C.byref(a), C.byref(b))
    return rc, (P.uncore.last_error() if rc else "")


def draw(rng: np.random.Generator) -> tuple:
    """One trial: (sim dict, StreamSpec fields, replay, share redraws)."""
    from primesim_amd import config as CF

    def pick(xs):
        return xs[int(rng.integers(len(xs)))]

    sim = CF.preset("C1")
    s = sim["system"]
    cores = pick(CORES)
    levels = int(rng.integers(1, 5))
    block = pick((16, 32, 64, 128))
    s["num_cores"] = cores
    s["num_levels"] = levels
    s["cache"] = []
    for l in range(levels):
        ways, sets = pick((1, 2, 3, 4, 8)), pick((4, 8, 16, 32))
        s["cache"].append({"level": l, "share": 1, "access_time": 1 + 3 * l, "size": sets * ways * block,
                           "block_size": block, "num_ways": ways})
    ways, sets = pick((1, 2, 3, 4, 8)), pick((8, 12, 64))
    s["directory_cache"] = {"level": 0, "share": 1, "access_time": 10, "size": sets * ways * block,
                            "block_size": block, "num_ways": ways}
    s["sys_type"] = pick((0, 1))
    protocol = pick((0, 1))
    s["max_num_sharers"] = pick((1, 2, 4))
    s["shared_llc"] = pick((0, 1))
    s["tlb_enable"] = pick((0, 1))
    s["page_size"] = pick((256, 1024, 4096))
    if pick((0, 1)):
        s["tlb_cache"] = {"level": 0, "share": 1, "access_time": 1, "size": 32, "block_size": 1, "num_ways": 4}
    s["bus_latency"] = pick((1, 2, 3))
    s["dram_access_time"] = pick((0, 50, 120))
    # header_flits >= 1: zero-flit packets are refused (tests/test_config.py)
    s["network"] = {"net_type": pick((0, 1)), "data_width": pick((1, 4, 10, 16, 64)), "header_flits": pick((1, 2, 3)),
                    "router_delay": pick((0, 1, 2, 3)), "link_delay": pick((1, 2)), "inject_delay": pick((0, 1, 4))}
    replay = pick(("open", "closed"))
    kind = int(rng.integers(1, 7))          # the six PU_STREAM_* kinds
    spec = {"kind": kind, "num_cores": cores, "seed": int(rng.integers(1, 1 << 20)), "quantum": pick((30, 100, 1000)),
            "num_quanta": pick((1, 2, 3)), "max_msg": pick((100, 7, 1)),
            "num_progs": pick((1, 2, 4)) if kind == 3 else 1, "max_requests": 4000,
            "write_pct": pick((-1, 0, 50, 100))}
    # shares multiply by 1, 2 or 4 per level; drawn again while a level's
    # children do not fill its last parent (refused: system.cpp:76, :184-188)
    redraws = 0
    while True:
        share = 1
        for l in range(1, levels):
            share *= pick((1, 2, 4))
            s["cache"][l]["share"] = share
        # limited pointer needs one LLC per core (system.cpp:623): full map elsewhere
        s["protocol_type"] = protocol if share == 1 else 0
        rc, text = geometry_rc(sim)
        if rc == 0:
            return sim, spec, replay, redraws
        assert rc == PU_ENOTSUP and "fill every parent" in text, f"the draw made a configuration refused for: {text}"
        redraws += 1


def trials() -> list:
    """The sweep's draws: what draw() gives for trial i's own generator, i in range(TRIALS)."""
    return [draw(np.random.default_rng([SEED, i])) for i in range(TRIALS)]


def sweep_configs() -> list:
    """(name, SimCfg) of every trial, in the shape of extra_configs.extra_configs()."""
    import primesim_amd as P
    return [(f"sweep {i:02d}", P.config_from_dict(sim)) for i, (sim, _, _, _) in enumerate(trials())]


def what(i: int, sim: dict, spec: dict, replay: str) -> str:
    """How a failure names trial i."""
    return f"trial {i} ({replay} replay, stream {spec}, configuration {json.dumps(sim['system'])})"


def write_trial(path: str, sim: dict, spec: dict, replay: str) -> None:
    import primesim_amd as P
    from primesim_amd import config as CF
    os.makedirs(path)
    CF.write_xml(sim, os.path.join(path, "config.xml"))
    with open(os.path.join(path, "cfg.bin"), "wb") as f:
        f.write(bytes(P.load_config(os.path.join(path, "config.xml"))))
    sp = P.StreamSpec(**spec)
    np.save(os.path.join(path, "reqs.npy"), P.generate_stream(sp).view(np.uint8))
    with open(os.path.join(path, "trial.json"), "w") as f:
        json.dump({"threads": P.stream_threads(sp), "replay": replay}, f)


def run_trial(path: str) -> dict:
    import oracle as O
    from primesim_amd import _abi as A
    with open(os.path.join(path, "cfg.bin"), "rb") as f:
        cfg = A.SimCfg.from_buffer_copy(f.read())
    reqs = np.load(os.path.join(path, "reqs.npy")).view(A.REQ_DTYPE)
    with open(os.path.join(path, "trial.json")) as f:
        t = json.load(f)
    mode = O.MODE_CLOSED if t["replay"] == "closed" else 0
    cpu = O.CpuRef(cfg)
    cpu.set_mode(mode)
    for prog, th in t["threads"]:
        cpu.alloc_core(prog, th)
    d0, rc0 = cpu.run(reqs)
    flags = int(cpu.stats().error_flags)
    if flags & ~A.PU_ERRF_NEG_DELAY:
        return {"status": "undefined", "flags": flags, "requests": len(reqs)}
    ref = O.RefUncore(os.path.join(path, "config.xml"))
    ref.set_mode(mode)
    for prog, th in t["threads"]:
        ref.alloc_core(prog, th)
    d1, rc1 = ref.run(reqs)
    bad = np.nonzero(d0 != d1)[0]
    comp = bool(np.array_equal(cpu.completion(), ref.completion()))
    if len(bad) or rc0 != rc1 or not comp:
        return {"status": "differs", "delays": int(len(bad)), "first": int(bad[0]) if len(bad) else None,
                "rc": [rc0, rc1], "completion_equal": comp, "requests": len(reqs)}
    return {"status": "equal", "requests": len(reqs), "rc": rc0}


if __name__ == "__main__":
    print(json.dumps(run_trial(sys.argv[1])), flush=True)
