"""Register, spill and LDS use of the compiled-configuration kernels of one
preset: the code objects the build-time warm-up (hipcc) produces (pu_config_jit_warm
into a scratch cache), read from its AMDGPU metadata.  No GPU.

    python tools/kernel_resources.py [C4] [--lib primesim_amd/libprimeuncore_X.so]

--static adds each kernel's static picture from its disassembly (llvm-objdump
-d): instructions and code bytes, the SGPR spill traffic (v_readlane_b32 /
v_writelane_b32), scalar no-ops of address arithmetic (a register moved onto
itself, x + 0, x + carry + 0), how often the kernel-argument tuple (the
s_load_dwordx8 at entry) is reloaded whole from its spill lanes, and the
spill lanes reloaded most often (a reloaded base pointer shows up as two
neighbouring lanes with the same count).
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size")


OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def static_counts(dis: str) -> dict:
    """Per pu_jit kernel of one disassembly: the counts --static prints."""
    out: dict = {}
    cur = None
    for ln in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:", ln)
        if m:
            cur = None
            if m.group(2).startswith("pu_jit"):
                cur = out[m.group(2)] = {"insts": 0, "bytes": 0, "v_readlane": 0, "v_writelane": 0, "self_moves": 0,
                                         "add_0": 0, "addc_0": 0, "arg_tuple_reloads": 0, "_first": int(m.group(1), 16),
                                         "_tuple": None, "_lane_of": {}, "_lanes": {}, "_run": set()}
            continue
        if cur is None:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):((?: [0-9A-Fa-f]{8})+)", ln)
        if not m:
            continue
        op, args = m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
        cur["insts"] += 1
        cur["bytes"] = int(m.group(3), 16) + 4 * len(m.group(4).split()) - cur["_first"]
        if op == "s_mov_b32" and len(args) == 2 and args[0] == args[1]:
            cur["self_moves"] += 1
        if op == "s_add_u32" and args[-1] == "0":
            cur["add_0"] += 1
        if op == "s_addc_u32" and args[-1] == "0":
            cur["addc_0"] += 1
        if op == "s_load_dwordx8" and cur["_tuple"] is None:      # the argument block: s[a:a+7]
            t = re.match(r"s\[(\d+):(\d+)\]", args[0])
            if t:
                cur["_tuple"] = {f"s{r}" for r in range(int(t.group(1)), int(t.group(2)) + 1)}
        if op == "v_writelane_b32":
            cur["v_writelane"] += 1
            if cur["_tuple"] and args[1] in cur["_tuple"] and len(cur["_lane_of"]) < 8:
                cur["_lane_of"][(args[0], args[2])] = args[1]     # the tuple's first spill: its eight lanes
        if op == "v_readlane_b32":
            cur["v_readlane"] += 1
            key = (args[1], args[2])
            cur["_lanes"][key] = cur["_lanes"].get(key, 0) + 1
            if key in cur["_lane_of"]:      # (a reload's eight readlanes are interleaved with other instructions)
                cur["_run"].add(key)
                if len(cur["_run"]) == 8:
                    cur["arg_tuple_reloads"] += 1
                    cur["_run"] = set()
    for k in out.values():
        top = sorted(k["_lanes"].items(), key=lambda kv: -kv[1])[:6]
        k["most_reloaded_spill_lanes"] = [f"{v}[{l}] x{n}" for (v, l), n in top]
        for x in [x for x in k if x.startswith("_")]:
            del k[x]
    return out


def resources(preset: str, lib: str | None = None, static: dict | None = None) -> dict:
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, PRIMEUNCORE_JIT_CACHE=d, PRIMEUNCORE_JIT_OFFLINE="1")   # hipcc, as shipped
        if lib:
            env["PRIMEUNCORE_LIB"] = os.path.abspath(lib)
        code = ("import ctypes as C, sys; sys.path.insert(0, %r); import primesim_amd as P; "
                "from primesim_amd import config as CF, uncore; cfg = P.config_from_dict(CF.preset(%r)); "
                "rc = uncore.lib().pu_config_jit_warm(C.byref(cfg)); sys.exit(0 if rc >= 0 else 1)") % (ROOT, preset)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-3000:])
        # two code objects per configuration (jit.cpp: throughput and latency kernels)
        notes = "".join(subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", hsaco],
                                       capture_output=True, text=True).stdout
                        for hsaco in sorted(glob.glob(os.path.join(d, "*.hsaco"))))
        if static is not None:
            for hsaco in sorted(glob.glob(os.path.join(d, "*.hsaco"))):
                static.update(static_counts(subprocess.run([OBJDUMP, "-d", hsaco], capture_output=True,
                                                           text=True).stdout))
    # one map per kernel, keys in alphabetical order (.agpr_count first, .name
    # in the middle): a kernel's entry starts at its .agpr_count line
    out: dict = {}
    entry: dict = {}
    for ln in notes.splitlines():
        s = ln.strip().lstrip("- ")
        if s.startswith(".agpr_count:"):
            entry = {}
        m = re.match(r"\.name:\s+(\S+)", s)
        if m and m.group(1).startswith("pu_jit"):
            out[m.group(1)] = entry
            continue
        m = re.match(r"(\.[a-z_]+):\s+(\d+)$", s)
        if m and m.group(1) in KEYS:
            entry[m.group(1)] = int(m.group(2))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="C4")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--static", action="store_true", help="also the static instruction picture of each kernel")
    a = ap.parse_args()
    static: dict | None = {} if a.static else None
    for k, v in sorted(resources(a.preset, a.lib, static).items()):
        print(k, v)
    for k, v in sorted((static or {}).items()):
        print(k, "static", v)


if __name__ == "__main__":
    main()
