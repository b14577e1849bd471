"""libprimeuncore.so and the rules for calling it.

`SIGNATURES` is the ctypes declaration of every entry of include/primeuncore.h and
`lib()` loads the library and applies it.  The ABI has three return conventions and
there is one helper for each: `call` (0 or a PU_E* code), `opened` (a handle or
NULL) and `counted` (a count or a negative code).  All three raise `UncoreError` in
one form, "<entry>: <the library's text> (<code>)".  A raw `lib().pu_x(...)` returns
what the entry returns.  `_Owner` and `_DeviceSet` are the bases of the classes that
hold a native handle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# PRIMEUNCORE_LIB selects another build of the same library (the region-profiling
# build, tools/prof_regions.py); there is no fallback when it is missing.
LIB_PATH = os.environ.get("PRIMEUNCORE_LIB") or os.path.join(_HERE, "libprimeuncore.so")
_lib: Optional[C.CDLL] = None

# PU_E* codes (include/primeuncore.h).  pu_access returns them in-band (a
# wrapped delay may collide with one); the mirror uses pu_access_status.
PU_ERRORS = (-5, -12, -19, -22, -34, -71, -95)

P = C.POINTER
# name -> (restype, argtypes); an entry left undeclared would return int, which truncates a handle or a char*
SIGNATURES = {
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
    "pu_dseries_open": (C.c_void_p, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]),
    "pu_dseries_close": (None, [C.c_void_p]),
    "pu_dseries_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pu_dseries_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DseriesCell)]),
    "pu_dseries_read_total": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(A.DseriesCell)]),
    "pu_dseries_reset": (C.c_int, [C.c_void_p]),
    "pu_dseries_state_bytes": (C.c_uint64, [C.c_void_p]),
    "pu_dseries_epochs": (C.c_int, [C.c_void_p]),
    "pu_dseries_host_add": (C.c_int, [P(A.DseriesCell), C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, P(C.c_int32),
                                      C.c_size_t]),
    "pu_dseries_epoch_of": (C.c_int, [C.c_int64, C.c_int, C.c_int64, C.c_int]),
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
    "pu_unit_mg1_path_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_int]),
    "pu_unit_queue_run": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                    P(C.c_uint64), C.c_int]),
    "pu_unit_network_run": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                      P(A.Stats), C.c_int]),
}
del P
# diagnostics and test hooks only: libraries of older commits (same-box A/B variants) lack them
OPTIONAL = ("pu_jit_prof_read", "pu_unit_mg1_path_run")


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
    for name, (res, args) in SIGNATURES.items():
        if name in OPTIONAL and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return lib().pu_last_error().decode()


def library_source_hash() -> str:
    """The source hash pu_version() was built with (tools/src_hash.py)."""
    v = lib().pu_version().decode()
    return v.rsplit(" src ", 1)[1] if " src " in v else ""


def call(name: str, *args, context: str = "") -> None:
    """An entry that returns 0 or a PU_E* code.  context goes in front of the message where the
    caller knows what the library does not (a path, which member of a set)."""
    rc = getattr(_lib or lib(), name)(*args)
    if rc != 0:
        raise UncoreError(f"{context}{name}: {last_error()} ({rc})")


def opened(name: str, *args, context: str = "") -> int:
    """An entry that returns a handle, or NULL with the reason in last_error()."""
    h = getattr(_lib or lib(), name)(*args)
    if not h:
        raise UncoreError(f"{context}{name}: {last_error()}")
    return h


def counted(name: str, *args, context: str = "") -> int:
    """An entry that returns a count, or a negative PU_E* code."""
    n = getattr(_lib or lib(), name)(*args)
    if n < 0:
        raise UncoreError(f"{context}{name}: {last_error()} ({n})")
    return int(n)


def _as(a: Optional[np.ndarray], ctype):
    """A contiguous array as a POINTER(ctype) argument (None stays None: the entry's "not given")."""
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _to_end(count: int, first: int, n: Optional[int]) -> int:
    """n of a (first, n) range over `count` members: by default the members from first on."""
    return count - first if n is None else n


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


class _DeviceSet(_Owner):
    """A set of `_n` replicas' state on the device behind the entries `<_prefix>_*`:
    `_open` creates it, `_call` runs `<_prefix>_<suffix>` on the handle."""
    _prefix = ""
    _n = 0
    _close = property(lambda self: f"{self._prefix}_close")
    _no_handle = property(lambda self: f"{type(self).__name__} is closed")

    def _open(self, *args) -> None:
        self._h = opened(f"{self._prefix}_open", *args)

    def _call(self, suffix: str, *args) -> None:
        call(f"{self._prefix}_{suffix}", self._handle(), *args)

    def _count(self, first: int, n: Optional[int]) -> int:
        """n of a reader's (first, n): by default the replicas from first on."""
        return _to_end(self._n, first, n)

    def __len__(self) -> int:
        return self._n

    @property
    def state_bytes(self) -> int:
        """Device memory the set holds."""
        return int(getattr(lib(), f"{self._prefix}_state_bytes")(self._handle()))
