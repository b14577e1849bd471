"""What the C-ABI tests share (test_abi.py, test_dstream_abi.py, test_dsum_abi.py,
test_req16_layout.py): the repository root, whether a GPU is present, and the
recipe for a stand-alone C++ check under tests/cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_present() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def run_cpp_check(tmp_path, source: str, *, includes=()) -> str:
    """Builds tests/cpp/<source> as a stand-alone program with the host's address
    and undefined-behaviour sanitizers, runs it and returns what it printed."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / os.path.splitext(source)[0]
    # the sanitizer runtimes linked into the program itself: it then runs whatever else the loader brings in
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", *static, *[f"-I{d}" for d in includes], "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", source)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout
