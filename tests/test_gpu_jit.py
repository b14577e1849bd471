"""The engine kernels are the configuration compiled into the kernel (jit.cpp:
hipcc's code objects from the build-time warm-up, hipRTC on a cache miss at
run time).  Every handle runs them for every launch (latency launches: at most
one replica per CU, headers in LDS; throughput launches: short batches, many
replicas) and reports so; there is no other engine to fall back to, so a
compile that fails fails pu_create with the compiler's log.
"""
import pytest

import primesim_amd as P
from primesim_amd import uncore
from golden_util import Case
from test_gpu_golden import test_engine_reproduces_reference

pytestmark = pytest.mark.gpu


def _reports_compiled_configuration(name):
    um = P.UncoreManager()
    um.init(P.load_config(Case(name).xml_path), replicas=1)
    try:
        assert uncore.lib().pu_compiled_config(um._handle()) == 2
    finally:
        um.close()


def test_handle_reports_its_variant():
    _reports_compiled_configuration("c1_hot")


# The test below dates from when the library held a second set of engine
# kernels that read the geometry at run time, selected by environment
# variables that are gone with them.  Its cases are retired in steps (its
# companion, test_ahead_of_time_kernels_match_reference, went when
# test_gpu_kernel_matrix.py began to run every golden on every kernel, each
# cell also checking that the handle reports the compiled configuration);
# these five go with the next change to this file.  Until then each checks
# that a handle on its kind of configuration (one level, multi-program, bus
# system, TLB, closed loop) reports the compiled configuration, and re-runs
# its golden.
@pytest.mark.parametrize("name", ["c1_hot", "c3_multiprog", "bus_c2", "tlb_c3", "c4_closed"])
def test_ahead_of_time_throughput_launches_match_reference(name):
    _reports_compiled_configuration(name)
    test_engine_reproduces_reference(name)


def test_failed_compile_fails_the_handle(tmp_path, monkeypatch):
    """A cache miss whose compile fails (an empty cache directory, an option
    that makes the engine source an error) fails pu_create: the error carries
    the compiler's diagnostic, nothing is cached and no kernel is launched
    (there is no handle).  With the environment restored a new handle on the
    same configuration is the compiled configuration again and reproduces the
    reference."""
    cfg = P.load_config(Case("c1_hot").xml_path)
    with monkeypatch.context() as m:
        m.setenv("PRIMEUNCORE_JIT_CACHE", str(tmp_path))
        m.setenv("PRIMEUNCORE_JIT_EXTRA", "-Werror=macro-redefined -DPU_JIT_PART=7")
        um = P.UncoreManager()
        with pytest.raises(uncore.UncoreError, match="'PU_JIT_PART' macro redefined"):
            um.init(cfg, replicas=1)
        assert um._h is None
    assert list(tmp_path.glob("*.hsaco")) == []
    um = P.UncoreManager()
    um.init(cfg, replicas=1)
    try:
        assert uncore.lib().pu_compiled_config(um._handle()) == 2
    finally:
        um.close()
    test_engine_reproduces_reference("c1_hot")


def test_handle_reports_its_compiler(tmp_path, monkeypatch):
    """The in-tree cache holds hipcc's code objects (build-time warm-up): a
    handle over it reports compiler 2.  A cache miss at run time (an empty
    cache directory) is compiled by hipRTC in-process, never by starting a
    compiler from a process that has used the GPU: compiler 1, and the same
    delays as the reference."""
    cfg = P.load_config(Case("c1_hot").xml_path)
    um = P.UncoreManager()
    um.init(cfg, replicas=1)
    try:
        assert uncore.lib().pu_compiled_compiler(um._handle()) == 2
    finally:
        um.close()
    monkeypatch.setenv("PRIMEUNCORE_JIT_CACHE", str(tmp_path))
    um = P.UncoreManager()
    um.init(cfg, replicas=1)
    try:
        assert uncore.lib().pu_compiled_compiler(um._handle()) == 1
    finally:
        um.close()
    assert len(list(tmp_path.glob("*.hsaco"))) == 2        # both parts, hipRTC's keys
    test_engine_reproduces_reference("c1_hot")              # on hipRTC's code objects (the env still points there)
