"""The engine's source set (primesim_amd/csrc/Makefile JIT_SRCS; jit.cpp), without a GPU:
the sources embedded in the library for the per-configuration compile are closed under
#include and leave the API header out, pu_jit_source_tag() is the hash of exactly those
files, and include/primeuncore_records.h, the one header the host and the engine share,
stands on its own and declares no function."""
import os
import re
import shutil
import subprocess

import pytest

import test_abi
from abi_helpers import ROOT
from primesim_amd.uncore import lib

CSRC = os.path.join(ROOT, "primesim_amd", "csrc")
RECORDS = os.path.join(ROOT, "include", "primeuncore_records.h")
MAIN = "engine.hip"          # jit.cpp kMainSrc
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+(\S+)', re.M)
N_DECLARED = 119             # the entries primeuncore.h declared when the records header was split off


def jit_sources():
    """[(name, path)] of the embedded sources, in order: the Makefile's one list, each file
    under its own name."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        lists = re.findall(r"^JIT_SRCS\s*:?=\s*(.+)$", f.read(), flags=re.M)
    assert len(lists) == 1, lists
    return [(os.path.basename(s), os.path.normpath(os.path.join(CSRC, s))) for s in lists[0].split()]


@pytest.fixture(scope="module")
def sources():
    out = []
    for name, path in jit_sources():
        with open(path, "rb") as f:
            out.append((name, path, f.read()))
    return out


def test_the_makefile_embeds_its_one_list():
    """What the build hands to tools/embed_src.py (the recipe as make expands it) is
    JIT_SRCS, name=path for each, and that list is the rule's prerequisites too."""
    r = subprocess.run(["make", "-C", CSRC, "-n", "-B", "--no-print-directory", "../../build/obj/jit_src.cpp"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    cmds = [ln.split() for ln in r.stdout.splitlines() if "embed_src.py" in ln]
    assert len(cmds) == 1, r.stdout
    pairs = cmds[0][cmds[0].index("../../build/obj/jit_src.cpp") + 1:]
    want = jit_sources()
    assert [p.split("=", 1)[0] for p in pairs] == [n for n, _ in want]
    assert [os.path.normpath(os.path.join(CSRC, p.split("=", 1)[1])) for p in pairs] == [p for _, p in want]
    assert want[0][0] == MAIN and len({n for n, _ in want}) == len(want)
    with open(os.path.join(CSRC, "jit.cpp")) as f:
        assert f'kMainSrc = "{MAIN}"' in f.read()


def test_the_set_is_closed_and_leaves_the_api_header_out(sources):
    names = {n for n, _, _ in sources}
    paths = {p for _, p, _ in sources}
    with open(os.path.join(CSRC, "jit.cpp")) as f:
        geo = re.findall(r'-DPU_JIT_GEO=\\"([^"\\]+)\\"', f.read())
    assert len(geo) == 1, geo
    included = set()
    for name, path, text in sources:
        for inc in INCLUDE.findall(text.decode()):
            if inc.startswith("<"):
                continue                     # the toolchain's own (hipRTC: jit.cpp's stand-ins)
            if not inc.startswith('"'):
                assert inc == "PU_JIT_GEO", (name, inc)      # the configuration, written by geo_emit.h
                continue
            inc = inc.strip('"')
            if "/" in inc:                   # the library's own build: a path from the including file
                target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
                assert target in paths, (name, inc)
                included.add(os.path.basename(target))
            else:                            # the per-configuration compile: a flat name
                assert inc in names or inc == geo[0], (name, inc)
                included.add(inc)
    assert included >= names - {MAIN}, names - {MAIN} - included
    assert "primeuncore.h" not in names
    for name, _, text in sources:
        if name in (MAIN, "geometry.h"):
            assert not re.search(r'#[ \t]*include[ \t]+"([^"]*/)?primeuncore\.h"', text.decode()), name


def fnv1a(data: bytes, h: int) -> int:
    for c in data:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_tag_is_the_hash_of_exactly_those_files(sources):
    """jit.cpp: FNV-1a 64 from the offset basis over the seed string, then each source's
    name and text in the list's order; the tag is the upper 32 bits."""
    h = fnv1a(b"primeuncore-jit-src", 1469598103934665603)
    for name, _, text in sources:
        h = fnv1a(text, fnv1a(name.encode(), h))
    assert lib().pu_jit_source_tag().decode() == f"{h >> 32:08x}"


def _compiler(*candidates):
    for c in candidates:
        p = shutil.which(c) or (c if os.path.isabs(c) and os.access(c, os.X_OK) else None)
        if p:
            return p
    raise AssertionError(f"none of {candidates} found")


@pytest.mark.parametrize("lang,std,candidates", [
    ("c", "-std=c11", ("gcc", "cc", "clang", "/opt/rocm/lib/llvm/bin/clang")),
    ("c++", "-std=c++17", ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")),
])
def test_the_records_header_compiles_on_its_own(lang, std, candidates):
    r = subprocess.run([_compiler(*candidates), "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", RECORDS],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_the_records_header_declares_no_function():
    """test_abi.py's own symbol search finds nothing in the records header and, in
    primeuncore.h, every entry whose arguments are the records that moved."""
    with open(RECORDS) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(test_abi.__file__) as f:       # the regex below is that file's, to the letter
        assert r'''re.findall(r"^[A-Za-z_][\w \*]*?\b(pu_\w+)\s*\(", text, flags=re.M)''' in f.read()
    assert re.findall(r"^[A-Za-z_][\w \*]*?\b(pu_\w+)\s*\(", text, flags=re.M) == []
    assert "extern" not in text
    syms = test_abi.declared_symbols()
    assert len(syms) >= N_DECLARED
    assert {"pu_pack_req16", "pu_set_device_req_format", "pu_access_batch", "pu_run_device", "pu_error_flags",
            "pu_jit_source_tag"} <= set(syms)
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        first = INCLUDE.search(f.read())
    assert first and first.group(1) == '"primeuncore_records.h"'
