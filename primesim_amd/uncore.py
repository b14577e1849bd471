"""Python host mirror of the reference's uncore interface, over the C ABI.

`UncoreManager` follows reference src/uncore_manager.h:51-68 (init, allocCore,
deallocCore, getCoreId, uncore_access, report) with the same argument meaning
and error behaviour (uncore_access returns -1 for core_id >= num_cores,
system.cpp:147-150).  It adds the batch paths the engine is built for:
`access_batch` (host arrays, one replica) and `run_device` (device-resident
requests for every replica, the benchmark path).

The HIP library is mandatory: importing works everywhere (stream generation
and config parsing are host code), but creating an engine without a GPU or
without the built library raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# PRIMEUNCORE_LIB selects another build of the same library (the region-profiling
# build, tools/prof_regions.py); there is no fallback when it is missing.
LIB_PATH = os.environ.get("PRIMEUNCORE_LIB") or os.path.join(_HERE, "libprimeuncore.so")
_lib: Optional[C.CDLL] = None


class UncoreError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libprimeuncore.so (build it with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UncoreError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 under the
    # same SONAME (libamdhip64.so.7) but NEEDs it as "libamdhip64.so", so if this
    # library loaded /opt/rocm's copy first, torch would load a second runtime
    # and find no GPU.  Loading torch first makes both share torch's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    sig = {
        "pu_config_load_xml": (C.c_int, [C.c_char_p, P(A.SimCfg)]),
        "pu_config_parse_xml": (C.c_int, [C.c_char_p, C.c_size_t, P(A.SimCfg)]),
        "pu_config_write_xml": (C.c_int, [P(A.SimCfg), C.c_char_p, C.c_size_t, P(C.c_size_t)]),
        "pu_create": (C.c_void_p, [P(A.SimCfg), C.c_int, C.c_int]),
        "pu_config_geo_source": (C.c_long, [P(A.SimCfg), C.c_char_p, C.c_size_t]),
        "pu_config_jit_warm": (C.c_int, [P(A.SimCfg)]),
        "pu_compiled_config": (C.c_int, [C.c_void_p]),
        "pu_compiled_compiler": (C.c_int, [C.c_void_p]),
        "pu_last_launch_kernel": (C.c_char_p, [C.c_void_p]),
        "pu_jit_source_tag": (C.c_char_p, []),
        "pu_jit_prof_read": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int, C.c_int]),
        "pu_destroy": (None, [C.c_void_p]),
        "pu_reset": (C.c_int, [C.c_void_p]),
        "pu_num_replicas": (C.c_int, [C.c_void_p]),
        "pu_replica_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_limit_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_replica_pool_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_resident_replicas": (C.c_int, [C.c_void_p]),
        "pu_alloc_core": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
        "pu_dealloc_core": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
        "pu_get_core_id": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
        "pu_access": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_uint64), C.c_int64]),
        "pu_access_status": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_uint64), C.c_int64,
                                       P(C.c_int32)]),
        "pu_access_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
        "pu_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pu_run_device_sliced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_void_p]),
        "pu_pool_slots": (C.c_int, [C.c_void_p]),
        "pu_pool_words": (C.c_long, [C.c_int]),
        "pu_run_device_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_uint64, C.c_void_p]),
        "pu_synchronize": (C.c_int, [C.c_void_p]),
        "pu_set_device_req_format": (C.c_int, [C.c_void_p, C.c_int]),
        "pu_pack_req16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
        "pu_core_completion": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "pu_stats_get": (C.c_int, [C.c_void_p, C.c_int, P(A.Stats)]),
        "pu_report": (C.c_long, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
        "pu_last_kernel_ms": (C.c_double, [C.c_void_p]),
        "pu_set_resident": (C.c_int, [C.c_void_p, C.c_int]),
        "pu_resident_info": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_size_t]),
        "pu_last_error": (C.c_char_p, []),
        "pu_version": (C.c_char_p, []),
        "pu_set_replay_mode": (C.c_int, [C.c_void_p, C.c_int]),
        "pu_sim_start_time": (None, [C.c_void_p]),
        "pu_sim_finish_time": (None, [C.c_void_p]),
        "pu_error_flags": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_stream_count": (C.c_int64, [P(A.StreamParams)]),
        "pu_stream_generate": (C.c_int64, [P(A.StreamParams), C.c_void_p, C.c_size_t]),
        "pu_stream_thread_of": (C.c_int, [P(A.StreamParams), C.c_int, P(C.c_int), P(C.c_int)]),
        "pu_stream_open": (C.c_void_p, [P(A.StreamParams)]),
        "pu_stream_close": (None, [C.c_void_p]),
        "pu_stream_next": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_stream_position": (C.c_int64, [C.c_void_p]),
        "pu_stream_next_many": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]),
        "pu_msglog_open": (C.c_void_p, [C.c_char_p, C.c_int]),
        "pu_msglog_next": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_msglog_messages": (C.c_int64, [C.c_void_p]),
        "pu_msglog_create": (C.c_void_p, [C.c_char_p]),
        "pu_msglog_append": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
        "pu_msglog_close": (C.c_int, [C.c_void_p]),
        "pu_msglog_from_requests": (C.c_int, [C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int]),
        "pu_stream_fits_req16": (C.c_int, [P(A.StreamParams)]),
        "pu_dstream_open": (C.c_void_p, [P(A.StreamParams), C.c_int, C.c_int]),
        "pu_dstream_close": (None, [C.c_void_p]),
        "pu_dstream_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                      C.c_void_p]),
        "pu_dstream_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "pu_dstream_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_replica_fork": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        "pu_stream_fork": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64]),
        "pu_dstream_fork": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_uint64), C.c_void_p]),
        "pu_dtrace_open": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), C.c_int]),
        "pu_dtrace_close": (None, [C.c_void_p]),
        "pu_dtrace_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                     C.c_void_p]),
        "pu_dtrace_seek": (C.c_int, [C.c_void_p, C.c_int64]),
        "pu_dtrace_position": (C.c_int64, [C.c_void_p]),
        "pu_dtrace_fits_req16": (C.c_int, [C.c_void_p]),
        "pu_dtrace_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_trace_place": (C.c_int, [C.c_void_p, C.c_size_t, P(C.c_int32), P(C.c_int32), C.c_int, C.c_int, C.c_void_p]),
        "pu_placement_shuffle": (C.c_int, [P(C.c_int32), C.c_int, C.c_uint64]),
        "pu_dsum_open": (C.c_void_p, [C.c_int, P(C.c_int32), C.c_int]),
        "pu_dsum_close": (None, [C.c_void_p]),
        "pu_dsum_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pu_dsum_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DsumReplica)]),
        "pu_dsum_read_cores": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint64), P(C.c_int64), C.c_size_t]),
        "pu_dsum_reset": (C.c_int, [C.c_void_p]),
        "pu_dsum_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_dsum_host_init": (None, [P(A.DsumReplica)]),
        "pu_dsum_host_add": (C.c_int, [P(A.DsumReplica), P(C.c_uint64), P(C.c_int64), C.c_int, C.c_void_p, C.c_int,
                                       P(C.c_int32), C.c_size_t]),
        "pu_dhist_open": (C.c_void_p, [C.c_int, C.c_int]),
        "pu_dhist_close": (None, [C.c_void_p]),
        "pu_dhist_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pu_dhist_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(C.c_uint64)]),
        "pu_dhist_quantiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(C.c_uint32), C.c_int, P(A.DhistQuantile)]),
        "pu_dhist_read_total": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(C.c_uint64)]),
        "pu_dhist_reset": (C.c_int, [C.c_void_p]),
        "pu_dhist_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_dhist_host_add": (C.c_int, [P(C.c_uint64), C.c_void_p, C.c_int, P(C.c_int32), C.c_size_t]),
        "pu_dhist_host_quantiles": (C.c_int, [P(C.c_uint64), P(C.c_uint32), C.c_int, P(C.c_uint64), P(C.c_int32)]),
        "pu_dhist_bucket_of": (C.c_int, [C.c_int32]),
        "pu_dhist_bucket_bounds": (C.c_int, [C.c_int, P(C.c_int32), P(C.c_int32)]),
        "pu_dtail_open": (C.c_void_p, [C.c_int, C.c_int, C.c_int]),
        "pu_dtail_close": (None, [C.c_void_p]),
        "pu_dtail_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pu_dtail_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DtailEntry), P(C.c_uint32)]),
        "pu_dtail_read_total": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DtailEntry), P(C.c_int32), P(C.c_uint32)]),
        "pu_dtail_reset": (C.c_int, [C.c_void_p]),
        "pu_dtail_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_dtail_k": (C.c_int, [C.c_void_p]),
        "pu_dtail_host_add": (C.c_int, [P(A.DtailEntry), P(C.c_uint32), P(C.c_uint64), C.c_int, C.c_void_p, C.c_int,
                                        P(C.c_int32), C.c_size_t]),
        "pu_dres_open": (C.c_void_p, [C.c_void_p, C.c_int]),
        "pu_dres_close": (None, [C.c_void_p]),
        "pu_dres_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "pu_dres_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DresReplica)]),
        "pu_dres_read_queues": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint64), P(C.c_uint64), C.c_size_t]),
        "pu_dres_read_queue_totals": (C.c_int, [C.c_void_p, P(C.c_uint64), P(C.c_uint64), C.c_size_t]),
        "pu_dres_nqueues": (C.c_int, [C.c_void_p]),
        "pu_dres_state_bytes": (C.c_uint64, [C.c_void_p]),
        "pu_num_links": (C.c_int, [C.c_void_p]),
        "pu_num_queues": (C.c_int, [C.c_void_p]),
        "pu_dres_host_gather": (C.c_int, [C.c_void_p, C.c_int, P(A.DresReplica), P(C.c_uint64), P(C.c_uint64),
                                          C.c_size_t]),
        "pu_config_queue_ends": (C.c_int, [P(A.SimCfg), C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]),
        "pu_trace_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]),
        "pu_alloc_core_replica": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "pu_dealloc_core_replica": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "pu_get_core_id_replica": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "pu_server_create": (C.c_void_p, [C.c_void_p, P(A.ServerOpts)]),
        "pu_server_create_exec": (C.c_void_p, [A.EXEC_FN, C.c_void_p, C.c_int, P(A.ServerOpts)]),
        "pu_server_run": (C.c_int, [C.c_void_p]),
        "pu_server_round": (C.c_int, [C.c_void_p, C.c_int]),
        "pu_server_stop": (None, [C.c_void_p]),
        "pu_server_get_stats": (C.c_int, [C.c_void_p, P(A.ServerStats)]),
        "pu_server_destroy": (None, [C.c_void_p]),
        "pu_client_connect": (C.c_void_p, [C.c_char_p, C.c_int, C.c_int]),
        "pu_client_send": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
        "pu_client_recv": (C.c_int, [C.c_void_p, C.c_int, P(C.c_int32)]),
        "pu_client_close": (None, [C.c_void_p]),
        "pu_unit_mg1_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_int]),
        "pu_unit_queue_run": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        P(C.c_uint64), C.c_int]),
        "pu_unit_network_run": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          P(A.Stats), C.c_int]),
    }
    for name, (res, args) in sig.items():
        if name == "pu_jit_prof_read" and not hasattr(L, name):
            continue   # diagnostics only: libraries of older commits (same-box A/B variants) lack it
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return lib().pu_last_error().decode()


class _Owner:
    """Owns one native handle, `_h` (set once the library has created it):
    `_handle()` gives it or raises `_no_handle`, `close()` hands it to the
    library's entry `_close` and is run again, harmlessly, on collection."""
    _h: Optional[int] = None
    _close = ""
    _no_handle = ""

    def _handle(self) -> int:
        if not self._h:
            raise UncoreError(self._no_handle)
        return self._h

    def close(self) -> None:
        if self._h:
            getattr(lib(), self._close)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _state_bytes(entry: str, doc: str) -> property:
    return property(lambda self: int(getattr(lib(), entry)(self._handle())), doc=doc)


class _DelayStage(_Owner):
    """What the three delay stages share: `_n` replicas, and the entries `<_entry>_add`,
    `<_entry>_reset` and the readers, called on the handle by `_call`."""
    _entry = ""
    _n = 0

    def _call(self, name: str, *args) -> None:
        rc = getattr(lib(), f"{self._entry}_{name}")(self._handle(), *args)
        if rc != 0:
            raise UncoreError(f"{self._entry}_{name}: {last_error()} ({rc})")

    def _count(self, first: int, n: Optional[int]) -> int:
        """n of a reader's (first, n): by default the replicas from first on."""
        return self._n - first if n is None else n

    def __len__(self) -> int:
        return self._n

    def add(self, d_reqs_ptr: int, d_delay_ptr: int, d_begin_ptr: int, d_end_ptr: int, fmt: int = A.PU_REQ_FMT_32,
            stream_ptr: int = 0) -> None:
        """Asynchronous on stream_ptr (a hipStream_t as an integer); 0 is the set's own
        stream, which is not ordered with torch's streams.  d_begin / d_end: device uint64,
        one entry per replica, in records (d_off and d_off + 1 after run_device)."""
        self._call("add", d_reqs_ptr or None, fmt, d_delay_ptr or None, d_begin_ptr or None, d_end_ptr or None,
                   stream_ptr or None)

    def reset(self) -> None:
        self._call("reset")


# PU_E* codes (include/primeuncore.h).  pu_access returns them in-band (a
# wrapped delay may collide with one); the mirror uses pu_access_status.
PU_ERRORS = (-5, -12, -19, -22, -34, -71, -95)
PU_REPLAY_OPEN, PU_REPLAY_CLOSED = 0, 1
PU_REQ_FMT_32, PU_REQ_FMT_16 = 0, 1


def library_source_hash() -> str:
    """The source hash pu_version() was built with (tools/src_hash.py)."""
    v = lib().pu_version().decode()
    return v.rsplit(" src ", 1)[1] if " src " in v else ""


# ---------------------------------------------------------------- config
def load_config(path: str) -> A.SimCfg:
    """XmlParser::parse equivalent (reference xml_parser.cpp:684)."""
    cfg = A.SimCfg()
    rc = lib().pu_config_load_xml(path.encode(), C.byref(cfg))
    if rc != 0:
        raise UncoreError(f"config {path}: {last_error()}")
    return cfg


def parse_config(text: str) -> A.SimCfg:
    cfg = A.SimCfg()
    b = text.encode()
    rc = lib().pu_config_parse_xml(b, len(b), C.byref(cfg))
    if rc != 0:
        raise UncoreError(f"config: {last_error()}")
    return cfg


def config_from_dict(sim: dict) -> A.SimCfg:
    from .config import to_xml
    return parse_config(to_xml(sim))


# ---------------------------------------------------------------- streams
@dataclass
class StreamSpec:
    kind: int
    num_cores: int
    seed: int = 1
    quantum: int = 1000
    num_quanta: int = 1
    max_msg: int = 100
    num_progs: int = 1
    max_requests: int = 0
    write_pct: int = -1

    def params(self) -> A.StreamParams:
        return A.StreamParams(self.kind, self.num_cores, self.seed, self.quantum, self.num_quanta,
                              self.max_msg, self.num_progs, self.max_requests, self.write_pct, 0)


def pack_req16(reqs: np.ndarray) -> np.ndarray:
    """REQ_DTYPE records -> 16-B pu_req16 records (uint64 pairs, primeuncore.h);
    raises UncoreError naming the first record that does not fit."""
    assert reqs.dtype == A.REQ_DTYPE and reqs.flags.c_contiguous
    out = np.empty(reqs.shape + (2,), dtype=np.uint64)
    if lib().pu_pack_req16(reqs.ctypes.data, reqs.size, out.ctypes.data) != 0:
        raise UncoreError(last_error())
    return out


def generate_stream(spec: StreamSpec) -> np.ndarray:
    """Deterministic synthetic request stream in canonical order (REQ_DTYPE)."""
    p = spec.params()
    n = lib().pu_stream_count(C.byref(p))
    if n < 0:
        raise UncoreError(f"stream: {last_error()} ({n})")
    out = np.zeros(n, dtype=A.REQ_DTYPE)
    if n:
        got = lib().pu_stream_generate(C.byref(p), out.ctypes.data, n)
        if got != n:
            raise UncoreError(f"stream generation returned {got}, expected {n}")
    return out


def _fork_range(count: int, src: int, first: int, n: Optional[int], seeds):
    """(first, n, seeds) of a fork over `count` members: n = None is "to the end"; seeds,
    where given, one uint64 per member of the range."""
    n = count - first if n is None else n
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (max(n, 0),):
            raise UncoreError(f"fork: {seeds.shape} seeds for a range of {n}")
    return first, n, seeds


class StreamSet:
    """Resumable generators for several streams (pu_stream_open/next_many):
    `next(n)` returns the next n requests of every stream as an [count, n]
    array; the chunks concatenate to exactly generate_stream's output."""

    def __init__(self, specs: list[StreamSpec]):
        self._h = []
        self._specs = list(specs)
        for sp in specs:
            p = sp.params()
            h = lib().pu_stream_open(C.byref(p))
            if not h:
                self.close()
                raise UncoreError(f"stream: {last_error()}")
            self._h.append(h)
        self._arr = (C.c_void_p * len(self._h))(*self._h)

    def __len__(self) -> int:
        return len(self._h)

    def next_into(self, out: np.ndarray, threads: int = 0) -> int:
        """Fill out[i, :] with stream i's next out.shape[1] requests; returns the
        smallest number produced (short only at the end of a stream)."""
        assert out.dtype == A.REQ_DTYPE and out.ndim == 2 and out.shape[0] == len(self._h)
        assert out.flags.c_contiguous
        got = lib().pu_stream_next_many(self._arr, len(self._h), out.ctypes.data, out.shape[1], out.shape[1],
                                        threads)
        if got < 0:
            raise UncoreError(f"stream: {last_error()}")
        return int(got)

    def next(self, n: int, threads: int = 0) -> np.ndarray:
        out = np.zeros((len(self._h), n), dtype=A.REQ_DTYPE)
        got = self.next_into(out, threads)
        return out[:, :got]

    def position(self, i: int = 0) -> int:
        return int(lib().pu_stream_position(self._h[i]))

    def fork(self, src: int, first: int = 0, n: Optional[int] = None, seeds=None) -> None:
        """Streams [first, first + n) continue from stream src's position (pu_stream_fork):
        exact clones without seeds, else stream first + i draws as a stream of seeds[i]
        does.  src inside the range is left as it is.  A stream whose parameters differ
        from src's in more than the seed is refused, before any stream is changed."""
        first, n, seeds = _fork_range(len(self._h), src, first, n, seeds)
        if not (0 <= src < len(self._h) and 0 <= first and 0 <= n and first + n <= len(self._h)):
            raise UncoreError(f"pu_stream_fork: source {src} or range [{first}, {first + n}) outside the set")
        shape = dataclasses.replace(self._specs[src], seed=0)
        for d in range(first, first + n):   # all or nothing: pu_stream_fork itself refuses stream by stream
            if dataclasses.replace(self._specs[d], seed=0) != shape:
                raise UncoreError(f"pu_stream_fork: the parameters of stream {d} differ from those of stream {src} "
                                  "in more than the seed")
        for i in range(n):
            d = first + i
            if d == src:
                continue
            seed = int(seeds[i]) if seeds is not None else 0
            rc = lib().pu_stream_fork(self._h[d], self._h[src], int(seeds is not None), seed)
            if rc != 0:
                raise UncoreError(f"pu_stream_fork: stream {d}: {last_error()} ({rc})")
            self._specs[d] = dataclasses.replace(self._specs[d], seed=seed if seeds is not None
                                                 else self._specs[src].seed)

    def close(self) -> None:
        for h in self._h:
            lib().pu_stream_close(h)
        self._h = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_fits_req16(spec: StreamSpec) -> bool:
    """True when every record of the stream fits pu_req16, decided from the
    parameters alone (pu_stream_fits_req16): never True for a stream that
    pack_req16 would refuse."""
    p = spec.params()
    rc = lib().pu_stream_fits_req16(C.byref(p))
    if rc not in (0, -34):
        raise UncoreError(f"stream: {last_error()}")
    return rc == 0


class DeviceStreamSet(_Owner):
    """StreamSet on the device (pu_dstream_*): the generator state of every
    stream lives in device memory and `next_into` writes each stream's next
    chunk into device memory, ready for run_device / run_device_sliced /
    run_device_pool, byte for byte what StreamSet produces.  Pointers are plain
    integers (tensor.data_ptr()).  Needs a GPU: there is no host fallback."""
    _close, _no_handle = "pu_dstream_close", "DeviceStreamSet is closed"

    def __init__(self, specs: list[StreamSpec], device: int = 0):
        self._n = len(specs)
        arr = (A.StreamParams * max(1, len(specs)))(*[sp.params() for sp in specs])
        h = lib().pu_dstream_open(arr, len(specs), device)
        if not h:
            raise UncoreError(f"pu_dstream_open: {last_error()}")
        self._h = h

    def __len__(self) -> int:
        return self._n

    state_bytes = _state_bytes("pu_dstream_state_bytes", "Device memory the set's generator state takes.")

    def next_into(self, d_out_ptr: int, n_each: int, stride: Optional[int] = None, fmt: int = A.PU_REQ_FMT_32,
                  d_got_ptr: int = 0, stream_ptr: int = 0) -> None:
        """Stream i's next up to n_each requests into records [i*stride, i*stride + got_i)
        of d_out (pu_req, or pu_req16 with fmt = PU_REQ_FMT_16); got_i goes to
        d_got[i] (device uint64) when given.  Asynchronous on stream_ptr (a hipStream_t as an
        integer, e.g. torch.cuda.Stream().cuda_stream); 0 is the set's own stream, which is
        not ordered with torch's default stream: positions() waits for it."""
        rc = lib().pu_dstream_next(self._handle(), d_out_ptr or None, n_each, n_each if stride is None else stride,
                                   fmt, d_got_ptr or None, stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"pu_dstream_next: {last_error()} ({rc})")

    def fork(self, src: int, first: int = 0, n: Optional[int] = None, seeds=None, stream_ptr: int = 0) -> None:
        """StreamSet.fork on the device (pu_dstream_fork), asynchronous on stream_ptr like
        next_into: streams [first, first + n) continue from stream src's position, as exact
        clones without seeds, else stream first + i with the draws of a stream of seeds[i]."""
        first, n, seeds = _fork_range(self._n, src, first, n, seeds)
        rc = lib().pu_dstream_fork(self._handle(), src, first, n, None if seeds is None else _as(seeds, C.c_uint64),
                                   stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"pu_dstream_fork: {last_error()} ({rc})")

    def positions(self) -> np.ndarray:
        """Requests produced so far per stream (waits for the set's outstanding calls)."""
        out = np.zeros(self._n, dtype=np.int64)
        if lib().pu_dstream_positions(self._handle(), out.ctypes.data, self._n) != 0:
            raise UncoreError(f"pu_dstream_positions: {last_error()}")
        return out


# ---------------------------------------------------------------- recorded traces
def _as(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _rows(a, shape: tuple, what: str) -> Optional[np.ndarray]:
    """A placement or skew table as the contiguous int32 array of `shape` the library takes (None stays None)."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.shape != shape or a.dtype.kind not in "iu" or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
        raise UncoreError(f"{what}: an integer array of shape {shape} in int32 range, not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.int32)


def place_trace(reqs: np.ndarray, placement=None, skew=None, num_cores: Optional[int] = None,
                fmt: int = A.PU_REQ_FMT_32) -> np.ndarray:
    """A recorded trace under one replica's rows (pu_trace_place; the rule is in
    include/primeuncore.h): core' = placement[core], timer' = timer + skew[core], everything
    else unchanged.  Returns REQ_DTYPE records, or with fmt = PU_REQ_FMT_16 the [n, 2] uint64
    array pack_req16 gives for them.  num_cores defaults to the rows' length, or without rows
    to the trace's largest core + 1.  Needs no device."""
    assert reqs.dtype == A.REQ_DTYPE and reqs.ndim == 1
    reqs = np.ascontiguousarray(reqs)
    if num_cores is None:
        given = placement if placement is not None else skew
        num_cores = len(given) if given is not None else (int(reqs["core"].max()) + 1 if len(reqs) else 1)
    place = _rows(placement, (num_cores,), "place_trace: placement")
    sk = _rows(skew, (num_cores,), "place_trace: skew")
    out = np.zeros((len(reqs), 2), dtype=np.uint64) if fmt == A.PU_REQ_FMT_16 else np.zeros(len(reqs), dtype=A.REQ_DTYPE)
    rc = lib().pu_trace_place(reqs.ctypes.data, len(reqs), None if place is None else _as(place, C.c_int32),
                              None if sk is None else _as(sk, C.c_int32), num_cores, fmt, out.ctypes.data)
    if rc != 0:
        raise UncoreError(f"pu_trace_place: {last_error()} ({rc})")
    return out


_MASK64 = (1 << 64) - 1


def placement_seed(seed: int, r: int) -> int:
    """The pu_placement_shuffle seed of row r of random_placements(.., seed): 0 (the identity) for
    r = 0; otherwise the splitmix64 output function of (seed + r * 0x9E3779B97F4A7C15) mod 2^64,
    with 1 in place of a 0 (which would be the identity again)."""
    if r == 0:
        return 0
    z = (seed + r * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return (z ^ (z >> 31)) or 1


def random_placements(count: int, num_cores: int, seed: int) -> np.ndarray:
    """int32[count][num_cores]: row r is pu_placement_shuffle of placement_seed(seed, r), so row 0
    is the identity and every row is a permutation; deterministic.  Needs no device."""
    out = np.zeros((count, num_cores), dtype=np.int32)
    for r in range(count):
        rc = lib().pu_placement_shuffle(_as(out[r], C.c_int32), num_cores, placement_seed(seed, r))
        if rc != 0:
            raise UncoreError(f"pu_placement_shuffle: {last_error()} ({rc})")
    return out


class DeviceTraceSet(_Owner):
    """One recorded trace replayed across `count` replicas on the device (pu_dtrace_*): the
    trace lives in device memory once and `next_into` writes its next chunk into every
    replica's window under that replica's placement and skew rows ([count][num_cores], or
    None), byte for byte what place_trace gives.  One cursor for the whole set.  `next_into`
    has DeviceStreamSet's signature, so a driver can hold either.  Pointers are plain integers
    (tensor.data_ptr()).  Needs a GPU: place_trace is the host path."""
    _close, _no_handle = "pu_dtrace_close", "DeviceTraceSet is closed"

    def __init__(self, reqs: np.ndarray, num_cores: int, count: int, placements=None, skews=None, device: int = 0):
        assert reqs.dtype == A.REQ_DTYPE and reqs.ndim == 1
        reqs = np.ascontiguousarray(reqs)
        self._n, self._len = count, len(reqs)
        shape = (max(count, 0), max(num_cores, 0))
        place = _rows(placements, shape, "DeviceTraceSet: placements")
        sk = _rows(skews, shape, "DeviceTraceSet: skews")
        h = lib().pu_dtrace_open(reqs.ctypes.data if len(reqs) else None, len(reqs), num_cores, count,
                                 None if place is None else _as(place, C.c_int32),
                                 None if sk is None else _as(sk, C.c_int32), device)
        if not h:
            raise UncoreError(f"pu_dtrace_open: {last_error()}")
        self._h = h

    def __len__(self) -> int:
        return self._n

    @property
    def trace_len(self) -> int:
        """Records of the trace."""
        return self._len

    state_bytes = _state_bytes("pu_dtrace_state_bytes", "Device memory the set holds: the trace once, and the rows.")

    def next_into(self, d_out_ptr: int, n_each: int, stride: Optional[int] = None, fmt: int = A.PU_REQ_FMT_32,
                  d_got_ptr: int = 0, stream_ptr: int = 0) -> None:
        """The next got = min(n_each, what the trace has left) records, placed for replica i, into
        records [i*stride, i*stride + got) of d_out (pu_req, or pu_req16 with fmt =
        PU_REQ_FMT_16); got goes to d_got[i] (device uint64) when given.  Asynchronous on
        stream_ptr (a hipStream_t as an integer); 0 is the set's own stream, which is not
        ordered with torch's default stream: position() waits for it."""
        rc = lib().pu_dtrace_next(self._handle(), d_out_ptr or None, n_each, n_each if stride is None else stride,
                                  fmt, d_got_ptr or None, stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"pu_dtrace_next: {last_error()} ({rc})")

    def seek(self, position: int) -> None:
        """Move the set's cursor (0 .. trace_len); seek(0) replays the trace.  Waits for the set's outstanding calls."""
        rc = lib().pu_dtrace_seek(self._handle(), position)
        if rc != 0:
            raise UncoreError(f"pu_dtrace_seek: {last_error()} ({rc})")

    def position(self) -> int:
        """Records of the trace served so far (waits for the set's outstanding calls)."""
        p = int(lib().pu_dtrace_position(self._handle()))
        if p < 0:
            raise UncoreError(f"pu_dtrace_position: {last_error()} ({p})")
        return p

    def fits_req16(self) -> bool:
        """True when next_into serves PU_REQ_FMT_16 (decided at open; last_error() has the reason when not)."""
        return lib().pu_dtrace_fits_req16(self._handle()) == 0


# ---------------------------------------------------------------- delay summaries


def summarize_delays(reqs: np.ndarray, delays: np.ndarray, num_cores: Optional[int] = None,
                     fmt: int = A.PU_REQ_FMT_32):
    """The host fold of (request, delay) pairs (pu_dsum_host_add; the rule is in
    include/primeuncore.h): returns (summary, core_count, core_sum), where summary is
    one A.DSUM_DTYPE record and the per-core arrays (num_cores entries) are None
    without num_cores.  reqs: REQ_DTYPE records, or with fmt = PU_REQ_FMT_16 the
    [n, 2] uint64 array of pack_req16.  Needs no device."""
    n = len(delays)
    if fmt == A.PU_REQ_FMT_16:
        assert reqs.dtype == np.uint64 and reqs.shape == (n, 2)
    else:
        assert reqs.dtype == A.REQ_DTYPE and reqs.shape == (n,)
    reqs = np.ascontiguousarray(reqs)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    out = np.zeros(1, dtype=A.DSUM_DTYPE)
    lib().pu_dsum_host_init(_as(out, A.DsumReplica))
    cnt = sm = None
    if num_cores is not None:
        # (at least one entry, so that the library sees tables and refuses a num_cores below 1)
        cnt, sm = np.zeros(max(num_cores, 1), dtype=np.uint64), np.zeros(max(num_cores, 1), dtype=np.int64)
    rc = lib().pu_dsum_host_add(_as(out, A.DsumReplica), None if cnt is None else _as(cnt, C.c_uint64),
                                None if sm is None else _as(sm, C.c_int64), 0 if num_cores is None else num_cores,
                                reqs.ctypes.data, fmt, _as(delays, C.c_int32), n)
    if rc != 0:
        raise UncoreError(f"pu_dsum_host_add: {last_error()} ({rc})")
    return out[0], cnt, sm


class DeviceDelaySummary(_DelayStage):
    """Per-replica delay summaries kept on the device (pu_dsum_*): `add` folds every
    replica's records [begin[r], end[r]) of device request and delay arrays into its
    running summary, bit for bit what summarize_delays gives.  num_cores (one entry per
    replica) adds per-core (count, sum) tables.  Pointers are plain integers
    (tensor.data_ptr()).  Needs a GPU: there is no host fallback."""
    _entry, _close, _no_handle = "pu_dsum", "pu_dsum_close", "DeviceDelaySummary is closed"

    def __init__(self, count: int, num_cores=None, device: int = 0):
        self._n = count
        self._nc = None
        arr = None
        if num_cores is not None:
            self._nc = [int(c) for c in num_cores]
            if len(self._nc) != count:
                raise UncoreError(f"DeviceDelaySummary: {len(self._nc)} num_cores entries for {count} replicas")
            arr = (C.c_int32 * max(1, count))(*self._nc)
        h = lib().pu_dsum_open(count, arr, device)
        if not h:
            raise UncoreError(f"pu_dsum_open: {last_error()}")
        self._h = h

    state_bytes = _state_bytes("pu_dsum_state_bytes", "Device memory the set holds.")

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Summaries of replicas [first, first + n) as A.DSUM_DTYPE records (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros(max(n, 0), dtype=A.DSUM_DTYPE)
        self._call("read", first, n, _as(out, A.DsumReplica))
        return out

    def cores(self, replica: int) -> tuple[np.ndarray, np.ndarray]:
        """(count, sum) per core of one replica; raises for a set opened without num_cores."""
        nc = self._nc[replica] if self._nc is not None and 0 <= replica < self._n else 0
        cnt, sm = np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.int64)
        self._call("read_cores", replica, _as(cnt, C.c_uint64), _as(sm, C.c_int64), nc)
        return cnt, sm


# ---------------------------------------------------------------- delay histograms
def _ppm_array(ppm) -> np.ndarray:
    """Quantiles in parts per million as the uint32 array the library takes (it checks count and range)."""
    a = np.atleast_1d(np.asarray(ppm, dtype=np.int64))
    if a.ndim != 1 or (a < 0).any() or (a > 0xFFFFFFFF).any():
        raise UncoreError("quantiles: ppm is a list of integers in [0, 1000000]")
    return np.ascontiguousarray(a, dtype=np.uint32)


def dhist_bucket_of(d: int) -> int:
    """The log-linear bucket of a delay (pu_dhist_bucket_of; the rule is in include/primeuncore.h)."""
    return int(lib().pu_dhist_bucket_of(int(d)))


def dhist_bucket_bounds(k: int) -> tuple[int, int]:
    """(lo, hi), both inclusive, of the delays bucket k holds (pu_dhist_bucket_bounds)."""
    lo, hi = C.c_int32(), C.c_int32()
    rc = lib().pu_dhist_bucket_bounds(int(k), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise UncoreError(f"pu_dhist_bucket_bounds: {last_error()} ({rc})")
    return lo.value, hi.value


def delay_histogram(reqs: np.ndarray, delays: np.ndarray, fmt: int = A.PU_REQ_FMT_32) -> np.ndarray:
    """The host fold of (request, delay) pairs into a [2, PU_DHIST_BUCKETS] uint64 log-linear
    histogram, reads and writes apart (pu_dhist_host_add).  reqs as for summarize_delays.
    Needs no device."""
    n = len(delays)
    if fmt == A.PU_REQ_FMT_16:
        assert reqs.dtype == np.uint64 and reqs.shape == (n, 2)
    else:
        assert reqs.dtype == A.REQ_DTYPE and reqs.shape == (n,)
    reqs = np.ascontiguousarray(reqs)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    out = np.zeros((2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
    rc = lib().pu_dhist_host_add(_as(out, C.c_uint64), reqs.ctypes.data, fmt, _as(delays, C.c_int32), n)
    if rc != 0:
        raise UncoreError(f"pu_dhist_host_add: {last_error()} ({rc})")
    return out


def histogram_quantiles(hist: np.ndarray, ppm) -> tuple[np.ndarray, np.ndarray]:
    """(count, bucket) of log-linear histograms [..., PU_DHIST_BUCKETS]: per histogram its count
    (uint64 [...]) and the bucket of every quantile of ppm (int32 [..., len(ppm)]; -1 for an
    empty histogram), by the nearest-rank rule (pu_dhist_host_quantiles).  Needs no device."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.ndim < 1 or h.shape[-1] != A.PU_DHIST_BUCKETS:
        raise UncoreError(f"histogram_quantiles: the last axis holds {A.PU_DHIST_BUCKETS} buckets")
    q = _ppm_array(ppm)
    flat = h.reshape(-1, A.PU_DHIST_BUCKETS)
    count = np.zeros(len(flat), dtype=np.uint64)
    bucket = np.full((len(flat), max(len(q), 1)), -1, dtype=np.int32)
    for i in range(len(flat)):
        rc = lib().pu_dhist_host_quantiles(_as(flat[i], C.c_uint64), _as(q, C.c_uint32), len(q),
                                           _as(count[i:], C.c_uint64), _as(bucket[i], C.c_int32))
        if rc != 0:
            raise UncoreError(f"pu_dhist_host_quantiles: {last_error()} ({rc})")
    return count.reshape(h.shape[:-1]), bucket.reshape(h.shape[:-1] + (bucket.shape[1],))


class DeviceDelayHistogram(_DelayStage):
    """Per-replica log-linear delay histograms kept on the device (pu_dhist_*): `add` counts
    every replica's records [begin[r], end[r]) of device request and delay arrays into its
    [2, PU_DHIST_BUCKETS] histogram, bit for bit what delay_histogram gives; `quantiles`
    and `total` are formed on the device.  Pointers are plain integers (tensor.data_ptr()).
    Needs a GPU: there is no host fallback."""
    _entry, _close, _no_handle = "pu_dhist", "pu_dhist_close", "DeviceDelayHistogram is closed"

    def __init__(self, count: int, device: int = 0):
        self._n = count
        h = lib().pu_dhist_open(count, device)
        if not h:
            raise UncoreError(f"pu_dhist_open: {last_error()}")
        self._h = h

    state_bytes = _state_bytes("pu_dhist_state_bytes", "Device memory the set holds.")

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Histograms of replicas [first, first + n): uint64 [n, 2, PU_DHIST_BUCKETS] (waits for the set's calls)."""
        n = self._count(first, n)
        out = np.zeros((max(n, 0), 2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
        self._call("read", first, n, _as(out, C.c_uint64))
        return out

    def quantiles(self, ppm, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray]:
        """(count, bucket) of replicas [first, first + n), formed on the device: count uint64 [n, 2],
        bucket int32 [n, 2, len(ppm)] (-1 for an empty class); ppm: up to PU_DHIST_MAX_Q quantiles
        in parts per million.  dhist_bucket_bounds gives the delays a bucket holds."""
        n = self._count(first, n)
        q = _ppm_array(ppm)
        out = np.zeros((max(n, 0), 2), dtype=A.DHIST_Q_DTYPE)
        self._call("quantiles", first, n, _as(q, C.c_uint32), len(q), _as(out, A.DhistQuantile))
        return out["count"].copy(), out["bucket"][:, :, :len(q)].copy()

    def total(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The histogram summed over replicas [first, first + n): uint64 [2, PU_DHIST_BUCKETS].
        Histograms add elementwise, so ranks sum what this returns."""
        out = np.zeros((2, A.PU_DHIST_BUCKETS), dtype=np.uint64)
        self._call("read_total", first, self._count(first, n), _as(out, C.c_uint64))
        return out


# ---------------------------------------------------------------- slowest requests
def delay_tail(reqs: np.ndarray, delays: np.ndarray, k: int, fmt: int = A.PU_REQ_FMT_32, acc=None):
    """The host fold of (request, delay) pairs into one replica's lists of slowest requests
    (pu_dtail_host_add; the rule is in include/primeuncore.h): returns (entries, counts, seen),
    entries A.DTAIL_DTYPE [2, k] (reads and writes apart, best first, zero past the count),
    counts uint32 [2] and seen, the records added so far.  acc, a triple an earlier call
    returned for the same k, is continued (and left unchanged).  reqs as for
    summarize_delays.  Needs no device."""
    n = len(delays)
    if fmt == A.PU_REQ_FMT_16:
        assert reqs.dtype == np.uint64 and reqs.shape == (n, 2)
    else:
        assert reqs.dtype == A.REQ_DTYPE and reqs.shape == (n,)
    reqs = np.ascontiguousarray(reqs)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    k = int(k)
    if acc is None:
        entries, counts, seen = np.zeros((2, max(k, 1)), dtype=A.DTAIL_DTYPE), np.zeros(2, dtype=np.uint32), C.c_uint64(0)
    else:
        entries, counts, seen = acc[0].copy(), acc[1].copy(), C.c_uint64(int(acc[2]))
        if entries.shape != (2, k) or entries.dtype != A.DTAIL_DTYPE or counts.shape != (2,) or counts.dtype != np.uint32:
            raise UncoreError(f"delay_tail: acc is not the result of a call with k = {k}")
    rc = lib().pu_dtail_host_add(_as(entries, A.DtailEntry), _as(counts, C.c_uint32), C.byref(seen), k,
                                 reqs.ctypes.data, fmt, _as(delays, C.c_int32), n)
    if rc != 0:
        raise UncoreError(f"pu_dtail_host_add: {last_error()} ({rc})")
    return entries, counts, int(seen.value)


class DeviceDelayTail(_DelayStage):
    """Per-replica lists of the k slowest reads and the k slowest writes kept on the device
    (pu_dtail_*): `add` offers every replica's records [begin[r], end[r]) of device request and
    delay arrays to its lists, bit for bit what delay_tail gives; `total` is the best k of the
    ensemble, formed on the device.  Pointers are plain integers (tensor.data_ptr()).
    Needs a GPU: there is no host fallback."""
    _entry, _close, _no_handle = "pu_dtail", "pu_dtail_close", "DeviceDelayTail is closed"

    def __init__(self, count: int, k: int = 16, device: int = 0):
        self._n, self._k = count, k
        h = lib().pu_dtail_open(count, k, device)
        if not h:
            raise UncoreError(f"pu_dtail_open: {last_error()}")
        self._h = h

    @property
    def k(self) -> int:
        """Entries a list holds at most."""
        return int(lib().pu_dtail_k(self._handle()))

    state_bytes = _state_bytes("pu_dtail_state_bytes", "Device memory the set holds.")

    def read(self, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray]:
        """(entries, counts) of replicas [first, first + n): A.DTAIL_DTYPE [n, 2, k], best first and zero
        past the count, and uint32 [n, 2] (waits for the set's calls)."""
        n = self._count(first, n)
        entries = np.zeros((max(n, 0), 2, self._k), dtype=A.DTAIL_DTYPE)
        counts = np.zeros((max(n, 0), 2), dtype=np.uint32)
        self._call("read", first, n, _as(entries, A.DtailEntry), _as(counts, C.c_uint32))
        return entries, counts

    def total(self, first: int = 0, n: Optional[int] = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(entries, replicas, counts) of the best k over replicas [first, first + n), per class:
        A.DTAIL_DTYPE [2, k], int32 [2, k] (-1 past the count) and uint32 [2]; by delay descending,
        then replica, then position.  Lists of different ranks merge by the same order on the host."""
        entries = np.zeros((2, self._k), dtype=A.DTAIL_DTYPE)
        replicas = np.full((2, self._k), -1, dtype=np.int32)
        counts = np.zeros(2, dtype=np.uint32)
        self._call("read_total", first, self._count(first, n), _as(entries, A.DtailEntry), _as(replicas, C.c_int32),
                   _as(counts, C.c_uint32))
        return entries, replicas, counts


QUEUE_KINDS = ("x", "y", "z", "bus")     # pu_config_queue_ends: kind 0 .. 3


def queue_ends(cfg: A.SimCfg, q: int) -> tuple[int, int, int]:
    """(kind, a, b) of queue q of a configuration (pu_config_queue_ends; no device):
    kind 0 / 1 / 2 a link along x / y / z between nodes a < b, 3 the bus of cache b of
    level a, -1 (with a = b = -1) where q names no queue."""
    kind, a, b = C.c_int(), C.c_int(), C.c_int()
    rc = lib().pu_config_queue_ends(C.byref(cfg), q, C.byref(kind), C.byref(a), C.byref(b))
    if rc != 0:
        raise UncoreError(f"pu_config_queue_ends: {last_error()} ({rc})")
    return kind.value, a.value, b.value


def host_run_results(um: "UncoreManager", replica: int = 0, queues: bool = False):
    """One replica's end-of-run record by plain copies (pu_dres_host_gather), as an
    A.DRES_DTYPE record; with queues also the n and n1 of every queue."""
    out = np.zeros(1, dtype=A.DRES_DTYPE)
    nq = int(lib().pu_num_queues(um._handle())) if queues else 0
    n = np.zeros(nq, dtype=np.uint64) if queues else None
    n1 = np.zeros(nq, dtype=np.uint64) if queues else None
    rc = lib().pu_dres_host_gather(um._handle(), replica, _as(out, A.DresReplica),
                                   None if n is None else _as(n, C.c_uint64),
                                   None if n1 is None else _as(n1, C.c_uint64), nq)
    if rc != 0:
        raise UncoreError(f"pu_dres_host_gather: {last_error()} ({rc})")
    return (out[0], n, n1) if queues else out[0]


class DeviceRunResults(_Owner):
    """The end-of-run results of an UncoreManager's replicas gathered on the device
    (pu_dres_*): `gather` snapshots every replica of a range in one launch -- the
    counters of stats(), the fold of completion(), the run state and the visit counts
    of the links and buses -- and `read` brings the records (A.DRES_DTYPE) to the host
    in one copy.  queues=True keeps the per-queue map (16 B per queue and replica).
    Close it before the UncoreManager.  Needs a GPU: host_run_results is the host path."""
    _close, _no_handle = "pu_dres_close", "DeviceRunResults is closed"

    def __init__(self, um: "UncoreManager", queues: bool = False):
        self._um = um                      # the set reads the manager's replicas: keep it alive
        self._n = int(lib().pu_num_replicas(um._handle()))
        h = lib().pu_dres_open(um._handle(), A.PU_DRES_QUEUES if queues else 0)
        if not h:
            raise UncoreError(f"pu_dres_open: {last_error()}")
        self._h = h
        self._nq = int(lib().pu_dres_nqueues(h))

    def __len__(self) -> int:
        return self._n

    @property
    def num_queues(self) -> int:
        """Queues per replica: the links first, then the buses."""
        return self._nq

    @property
    def num_links(self) -> int:
        return int(lib().pu_num_links(self._um._handle()))

    state_bytes = _state_bytes("pu_dres_state_bytes", "Device memory the set holds.")

    def gather(self, first: int = 0, n: Optional[int] = None, stream_ptr: int = 0) -> None:
        """Asynchronous on stream_ptr (a hipStream_t as an integer; 0 is the set's own
        stream).  The caller orders it after the run it wants to see: the run's stream,
        or synchronize() first."""
        n = self._n - first if n is None else n
        self._um._handle()                 # the set reads the manager's replicas: it must still be open
        rc = lib().pu_dres_gather(self._handle(), first, n, stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"pu_dres_gather: {last_error()} ({rc})")

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records of replicas [first, first + n) as of their last gather (waits for the set's calls)."""
        n = self._n - first if n is None else n
        out = np.zeros(max(n, 0), dtype=A.DRES_DTYPE)
        rc = lib().pu_dres_read(self._handle(), first, n, _as(out, A.DresReplica))
        if rc != 0:
            raise UncoreError(f"pu_dres_read: {last_error()} ({rc})")
        return out

    def queues(self, replica: int) -> tuple[np.ndarray, np.ndarray]:
        """(n, n1) per queue of one replica; raises for a set opened without queues=True."""
        n, n1 = np.zeros(self._nq, dtype=np.uint64), np.zeros(self._nq, dtype=np.uint64)
        rc = lib().pu_dres_read_queues(self._handle(), replica, _as(n, C.c_uint64), _as(n1, C.c_uint64), self._nq)
        if rc != 0:
            raise UncoreError(f"pu_dres_read_queues: {last_error()} ({rc})")
        return n, n1

    def queue_totals(self) -> tuple[np.ndarray, np.ndarray]:
        """(n, n1) per queue summed over the replicas of the last gather.  A set opened with
        queues=True sums its map: a snapshot, like the records.  A set without it sums the queue
        headers as they are at this call, so after another run the two kinds of set answer
        differently for the same gather: read the totals before the next run, or keep the map."""
        self._um._handle()                 # without the map the totals are read from the manager's replicas
        n, n1 = np.zeros(self._nq, dtype=np.uint64), np.zeros(self._nq, dtype=np.uint64)
        rc = lib().pu_dres_read_queue_totals(self._handle(), _as(n, C.c_uint64), _as(n1, C.c_uint64), self._nq)
        if rc != 0:
            raise UncoreError(f"pu_dres_read_queue_totals: {last_error()} ({rc})")
        return n, n1


# ---------------------------------------------------------------- MsgMem logs
MSGMEM_DTYPE = np.dtype([("mem_type", np.uint8), ("_pad", np.uint8, 3), ("mem_size", np.int32),
                         ("addr_dmem", np.uint64), ("timer", np.int64)])   # reference common.h:49-59
assert MSGMEM_DTYPE.itemsize == 24
MSG_MEM_REQUESTS, MSG_PROCESS_STARTING, MSG_PROCESS_FINISHING = 0, -3, -1
MSG_BARRIER, MSG_NEW_THREAD, MSG_THREAD_FINISHING, MSG_PROGRAM_EXITING = -2, -4, -8, -5


def msglog_from_stream(path: str, reqs: np.ndarray, spec: "StreamSpec") -> None:
    """Write a synthetic stream as the MsgMem message log its cores would have sent."""
    threads = stream_threads(spec)
    tp = np.array([t[0] for t in threads], np.int32)
    ti = np.array([t[1] for t in threads], np.int32)
    ct = np.arange(spec.num_cores, dtype=np.int32)
    reqs = np.ascontiguousarray(reqs, dtype=A.REQ_DTYPE)
    rc = lib().pu_msglog_from_requests(path.encode(), reqs.ctypes.data, len(reqs), tp.ctypes.data, ti.ctypes.data,
                                       len(threads), ct.ctypes.data, spec.num_cores)
    if rc != 0:
        raise UncoreError(f"msglog: {last_error()}")


class MsgLogWriter:
    """Capture side: append messages exactly as prime.cpp:53 receives them."""

    def __init__(self, path: str):
        self._h = lib().pu_msglog_create(path.encode())
        if not self._h:
            raise UncoreError(f"msglog: {last_error()}")

    def append(self, source: int, records: np.ndarray) -> None:
        records = np.ascontiguousarray(records, dtype=MSGMEM_DTYPE)
        if lib().pu_msglog_append(self._h, source, records.ctypes.data, len(records)) != 0:
            raise UncoreError(f"msglog: {last_error()}")

    def close(self) -> None:
        if self._h:
            lib().pu_msglog_close(self._h)
            self._h = None


def msglog_read(path: str, um: "UncoreManager | None" = None, num_cores: int = 0,
                chunk: int = 1 << 16) -> np.ndarray:
    """Replay a MsgMem log into requests (prime.cpp:55-137 semantics), resolving
    core ids through um's ThreadSched (or the log's own over num_cores cores)."""
    L = lib().pu_msglog_open(path.encode(), num_cores)
    if not L:
        raise UncoreError(f"msglog: {last_error()}")
    parts = []
    try:
        h = um._handle() if um is not None else None
        while True:
            buf = np.zeros(chunk, dtype=A.REQ_DTYPE)
            n = lib().pu_msglog_next(L, h, buf.ctypes.data, chunk)
            if n < 0:
                raise UncoreError(f"msglog: {last_error()}")
            if n == 0:
                break
            parts.append(buf[:n])
    finally:
        lib().pu_msglog_close(L)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=A.REQ_DTYPE)


def stream_threads(spec: StreamSpec) -> list[tuple[int, int]]:
    """(prog_id, thread_id) of every core, in allocation order."""
    p = spec.params()
    res = []
    for c in range(spec.num_cores):
        pr, th = C.c_int(), C.c_int()
        if lib().pu_stream_thread_of(C.byref(p), c, C.byref(pr), C.byref(th)) != 0:
            raise UncoreError(last_error())
        res.append((pr.value, th.value))
    return res


# ---------------------------------------------------------------- engine
@dataclass
class InsMem:
    """reference src/cache.h:92-99 (the fields System::access reads)."""
    mem_type: int
    prog_id: int
    addr_dmem: int
    thread_id: int = 0
    rec_thread_id: int = 0


class UncoreManager(_Owner):
    """reference UncoreManager (uncore_manager.h:51-68) backed by the HIP engine."""
    _close, _no_handle = "pu_destroy", "UncoreManager not initialised"

    def __init__(self) -> None:
        self.cfg: Optional[A.SimCfg] = None
        self.replicas = 0

    # UncoreManager::init (uncore_manager.cpp:46-50)
    def init(self, cfg: A.SimCfg, replicas: int = 1, device: int = 0) -> None:
        h = lib().pu_create(C.byref(cfg), replicas, device)
        if not h:
            raise UncoreError(f"pu_create: {last_error()}")
        self._h = h
        self.cfg = cfg
        self.replicas = replicas

    def reset(self) -> None:
        if lib().pu_reset(self._handle()) != 0:
            raise UncoreError(last_error())

    @property
    def replica_bytes(self) -> int:
        return int(lib().pu_replica_bytes(self._handle()))

    @property
    def replica_pool_bytes(self) -> int:
        """The sharer-bitmap pool's share of replica_bytes."""
        return int(lib().pu_replica_pool_bytes(self._handle()))

    @property
    def resident_replicas(self) -> int:
        """Replicas the engine kernel holds resident on the device at once."""
        n = lib().pu_resident_replicas(self._handle())
        if n <= 0:
            raise UncoreError(last_error())
        return int(n)

    def allocCore(self, prog_id: int, thread_id: int) -> int:
        return lib().pu_alloc_core(self._handle(), prog_id, thread_id)

    def deallocCore(self, prog_id: int, thread_id: int) -> int:
        return lib().pu_dealloc_core(self._handle(), prog_id, thread_id)

    def getCoreId(self, prog_id: int, thread_id: int) -> int:
        return lib().pu_get_core_id(self._handle(), prog_id, thread_id)

    # UncoreManager::uncore_access (uncore_manager.cpp:82-85)
    def uncore_access(self, core_id: int, ins_mem: InsMem, timer: int) -> int:
        addr = C.c_uint64(ins_mem.addr_dmem)
        d = C.c_int32(0)
        rc = lib().pu_access_status(self._handle(), core_id, ins_mem.prog_id, ins_mem.mem_type, C.byref(addr), timer,
                                    C.byref(d))
        if rc != 0:                       # status out of band: every int delay is a delay
            raise UncoreError(f"uncore_access: {last_error()}")
        ins_mem.addr_dmem = addr.value
        return d.value

    def access_batch(self, reqs: np.ndarray, replica: int = 0) -> np.ndarray:
        """prime.cpp:120-137 for a run of messages; returns per-request delays."""
        reqs = np.ascontiguousarray(reqs, dtype=A.REQ_DTYPE)
        out = np.zeros(len(reqs), dtype=np.int32)
        rc = lib().pu_access_batch(self._handle(), replica, reqs.ctypes.data, len(reqs), out.ctypes.data)
        if rc != 0:
            raise UncoreError(f"access_batch: {last_error()}")
        return out

    # UncoreManager::getSimStartTime / getSimFinishTime (uncore_manager.cpp:52-60)
    def getSimStartTime(self) -> None:
        lib().pu_sim_start_time(self._handle())

    def getSimFinishTime(self) -> None:
        lib().pu_sim_finish_time(self._handle())

    def set_replay_mode(self, mode: int) -> None:
        """PU_REPLAY_OPEN (recorded timers) or PU_REPLAY_CLOSED (timer_i += the
        core's earlier batch delays, core_manager.cpp:265)."""
        if lib().pu_set_replay_mode(self._handle(), mode) != 0:
            raise UncoreError(last_error())

    def set_device_req_format(self, fmt: int) -> None:
        """PU_REQ_FMT_32 (pu_req) or PU_REQ_FMT_16 (pu_req16, pack_req16): the
        record format run_device / run_device_sliced / run_device_pool read."""
        if lib().pu_set_device_req_format(self._handle(), fmt) != 0:
            raise UncoreError(last_error())

    def error_flags(self, n: Optional[int] = None) -> np.ndarray:
        """PU_ERRF_* bits of replicas [0, n)."""
        n = self.replicas if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        if lib().pu_error_flags(self._handle(), out.ctypes.data, n) != 0:
            raise UncoreError(last_error())
        return out

    def limit_positions(self, n: Optional[int] = None) -> np.ndarray:
        """Per replica: index of the first request of the last launch that raised
        a PU_ERRF_LIMITS bit (2^64-1: none)."""
        n = self.replicas if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        if lib().pu_limit_positions(self._handle(), out.ctypes.data, n) != 0:
            raise UncoreError(last_error())
        return out

    def run_device(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, stream_ptr: int = 0) -> None:
        """All replicas at once on device-resident buffers (asynchronous)."""
        rc = lib().pu_run_device(self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"run_device: {last_error()}")

    def run_device_sliced(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, d_pos_ptr: int, budget_us: int,
                          stream_ptr: int = 0) -> None:
        """Time-sliced run: replica r continues from d_pos[r] for at most budget_us
        of wall time (stopping only between requests) and advances d_pos[r]."""
        rc = lib().pu_run_device_sliced(self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, d_pos_ptr, budget_us,
                                        stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"run_device_sliced: {last_error()}")

    def pool_slots(self) -> int:
        """Most wavefronts of a replica-pool launch: min(replicas, resident replicas)."""
        n = lib().pu_pool_slots(self._handle())
        if n < 0:
            raise UncoreError(f"pool_slots: {last_error()}")
        return int(n)

    @staticmethod
    def pool_words(slots: int) -> int:
        """uint32 words of the scheduling array a pool of `slots` wavefronts needs (all 0 to start)."""
        n = lib().pu_pool_words(slots)
        if n < 0:
            raise UncoreError(f"pool_words: {last_error()}")
        return int(n)

    def run_device_pool(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, d_pos_ptr: int, d_sched_ptr: int,
                        slots: int, budget_us: int, stream_ptr: int = 0) -> None:
        """Time-sliced run of more replicas than run at once: each of `slots`
        wavefronts continues its replica and, once that replica's range is done
        (or it halted), takes the next unstarted one (pu_run_device_pool)."""
        rc = lib().pu_run_device_pool(self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, d_pos_ptr, d_sched_ptr,
                                      slots, budget_us, stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"run_device_pool: {last_error()}")

    def fork_replica(self, src: int, first: int = 0, n: Optional[int] = None, by_copies: bool = False,
                     stream_ptr: int = 0) -> None:
        """Replicas [first, first + n) (n = None: to the last) become bit-for-bit copies of
        replica src (pu_replica_fork), asynchronously on stream_ptr like run_device; src
        inside the range is left as it is.  Their statistics, reports and completion cycles
        are then the source's, warm-up included.  by_copies: one device-to-device copy per
        destination instead of the kernel."""
        n = self.replicas - first if n is None else n
        rc = lib().pu_replica_fork(self._handle(), src, first, n, A.PU_FORK_BY_COPIES if by_copies else 0,
                                   stream_ptr or None)
        if rc != 0:
            raise UncoreError(f"pu_replica_fork: {last_error()} ({rc})")

    def synchronize(self) -> None:
        if lib().pu_synchronize(self._handle()) != 0:
            raise UncoreError(last_error())

    def last_kernel_ms(self) -> float:
        return float(lib().pu_last_kernel_ms(self._handle()))

    def last_launch_kernel(self) -> str:
        """Symbol name of the engine kernel the handle launched last
        (pu_last_launch_kernel), "" before any launch."""
        return lib().pu_last_launch_kernel(self._handle()).decode()

    def set_resident(self, mode: int) -> int:
        """Resident mode for uncore_access / short batches (pu_set_resident):
        1 on, 0 off, -1 query; returns the previous mode."""
        rc = lib().pu_set_resident(self._handle(), mode)
        if rc < 0:
            raise UncoreError(last_error())
        return rc

    def resident_info(self) -> dict:
        """The resident kernel (pu_resident_info): running, commands served,
        kernels launched, eligible, and per command the mean kernel-side phases
        (request copy, message loop, close, mailbox) and host-side call time in µs."""
        out = (C.c_uint64 * 10)()
        if lib().pu_resident_info(self._handle(), out, 10) < 0:
            raise UncoreError(last_error())
        n = max(1, int(out[1]))
        nfull = max(1, int(out[1]) - int(out[9]))
        sums_us = {"request_copy": out[4] / 100, "message_loop": out[5] / 100, "close": out[6] / 100,
                   "mailbox": out[7] / 100, "host_call": out[8] / 1000}
        return {"running": bool(out[0]), "commands": int(out[1]), "launches": int(out[2]), "eligible": bool(out[3]),
                "fast_answers": int(out[9]), "sums_us": sums_us,
                "mean_us": {k: v / (n if k == "host_call" else nfull) for k, v in sums_us.items()}}

    def stats(self, replica: int = 0) -> A.Stats:
        s = A.Stats()
        if lib().pu_stats_get(self._handle(), replica, C.byref(s)) != 0:
            raise UncoreError(last_error())
        return s

    def completion(self, replica: int = 0) -> np.ndarray:
        n = self.cfg.sys.num_cores
        out = np.zeros(n, dtype=np.int64)
        if lib().pu_core_completion(self._handle(), replica, out.ctypes.data, n) != 0:
            raise UncoreError(last_error())
        return out

    # UncoreManager::report (uncore_manager.cpp:87-98)
    def report(self, replica: int = 0, include_time: bool = False) -> str:
        n = lib().pu_report(self._handle(), replica, int(include_time), None, 0)
        if n < 0:
            raise UncoreError(last_error())
        buf = C.create_string_buffer(n + 1)
        lib().pu_report(self._handle(), replica, int(include_time), buf, n + 1)
        return buf.value.decode()


# ---------------------------------------------------------------- unit hooks
def unit_queue(min_proc: int, t: np.ndarray, p: np.ndarray, device: int = 0) -> tuple[np.ndarray, int]:
    """The history-tree queue model alone on the GPU."""
    t = np.ascontiguousarray(t, dtype=np.uint64)
    p = np.ascontiguousarray(p, dtype=np.uint64)
    out = np.zeros(len(t), dtype=np.uint64)
    calls = C.c_uint64(0)
    rc = lib().pu_unit_queue_run(min_proc, t.ctypes.data, p.ctypes.data, len(t), out.ctypes.data, C.byref(calls),
                                 device)
    if rc != 0:
        raise UncoreError(f"unit_queue: {last_error()}")
    return out, int(calls.value)


def unit_network(nodes: int, net_type: int, data_width: int, header_flits: int, router_delay: int,
                 link_delay: int, inject_delay: int, src, dst, ln, timer, device: int = 0):
    """Network::transmit sequence alone on the GPU."""
    src = np.ascontiguousarray(src, dtype=np.int32)
    dst = np.ascontiguousarray(dst, dtype=np.int32)
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    timer = np.ascontiguousarray(timer, dtype=np.uint64)
    out = np.zeros(len(src), dtype=np.uint64)
    st = A.Stats()
    rc = lib().pu_unit_network_run(nodes, net_type, data_width, header_flits, router_delay, link_delay,
                                   inject_delay, src.ctypes.data, dst.ctypes.data, ln.ctypes.data,
                                   timer.ctypes.data, len(src), out.ctypes.data, C.byref(st), device)
    if rc != 0:
        raise UncoreError(f"unit_network: {last_error()}")
    return out, st
