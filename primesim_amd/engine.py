"""The engine: configurations (pu_config_*), `UncoreManager` over one engine handle
(pu_create .. pu_destroy) and the unit hooks that run one model alone on the GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi as A
from ._native import _Owner, _to_end, call, counted, lib, opened


# ---------------------------------------------------------------- config
def load_config(path: str) -> A.SimCfg:
    """XmlParser::parse equivalent (reference xml_parser.cpp:684)."""
    cfg = A.SimCfg()
    call("pu_config_load_xml", path.encode(), C.byref(cfg), context=f"config {path}: ")
    return cfg


def parse_config(text: str) -> A.SimCfg:
    cfg = A.SimCfg()
    b = text.encode()
    call("pu_config_parse_xml", b, len(b), C.byref(cfg))
    return cfg


def config_from_dict(sim: dict) -> A.SimCfg:
    from .config import to_xml
    return parse_config(to_xml(sim))


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
        self._h = opened("pu_create", C.byref(cfg), replicas, device)
        self.cfg = cfg
        self.replicas = replicas

    def reset(self) -> None:
        call("pu_reset", self._handle())

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
        return counted("pu_resident_replicas", self._handle())

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
        # status out of band: every int delay is a delay
        call("pu_access_status", self._handle(), core_id, ins_mem.prog_id, ins_mem.mem_type, C.byref(addr), timer,
             C.byref(d))
        ins_mem.addr_dmem = addr.value
        return d.value

    def access_batch(self, reqs: np.ndarray, replica: int = 0) -> np.ndarray:
        """prime.cpp:120-137 for a run of messages; returns per-request delays."""
        reqs = np.ascontiguousarray(reqs, dtype=A.REQ_DTYPE)
        out = np.zeros(len(reqs), dtype=np.int32)
        call("pu_access_batch", self._handle(), replica, reqs.ctypes.data, len(reqs), out.ctypes.data)
        return out

    # UncoreManager::getSimStartTime / getSimFinishTime (uncore_manager.cpp:52-60)
    def getSimStartTime(self) -> None:
        lib().pu_sim_start_time(self._handle())

    def getSimFinishTime(self) -> None:
        lib().pu_sim_finish_time(self._handle())

    def set_replay_mode(self, mode: int) -> None:
        """PU_REPLAY_OPEN (recorded timers) or PU_REPLAY_CLOSED (timer_i += the
        core's earlier batch delays, core_manager.cpp:265)."""
        call("pu_set_replay_mode", self._handle(), mode)

    def set_device_req_format(self, fmt: int) -> None:
        """PU_REQ_FMT_32 (pu_req) or PU_REQ_FMT_16 (pu_req16, pack_req16): the
        record format run_device / run_device_sliced / run_device_pool read."""
        call("pu_set_device_req_format", self._handle(), fmt)

    def error_flags(self, n: Optional[int] = None) -> np.ndarray:
        """PU_ERRF_* bits of replicas [0, n)."""
        n = self.replicas if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        call("pu_error_flags", self._handle(), out.ctypes.data, n)
        return out

    def limit_positions(self, n: Optional[int] = None) -> np.ndarray:
        """Per replica: index of the first request of the last launch that raised
        a PU_ERRF_LIMITS bit (2^64-1: none)."""
        n = self.replicas if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        call("pu_limit_positions", self._handle(), out.ctypes.data, n)
        return out

    def run_device(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, stream_ptr: int = 0) -> None:
        """All replicas at once on device-resident buffers (asynchronous)."""
        call("pu_run_device", self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, stream_ptr or None)

    def run_device_sliced(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, d_pos_ptr: int, budget_us: int,
                          stream_ptr: int = 0) -> None:
        """Time-sliced run: replica r continues from d_pos[r] for at most budget_us
        of wall time (stopping only between requests) and advances d_pos[r]."""
        call("pu_run_device_sliced", self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, d_pos_ptr, budget_us,
             stream_ptr or None)

    def pool_slots(self) -> int:
        """Most wavefronts of a replica-pool launch: min(replicas, resident replicas)."""
        return counted("pu_pool_slots", self._handle())

    @staticmethod
    def pool_words(slots: int) -> int:
        """uint32 words of the scheduling array a pool of `slots` wavefronts needs (all 0 to start)."""
        return counted("pu_pool_words", slots)

    def run_device_pool(self, d_reqs_ptr: int, d_off_ptr: int, d_delay_ptr: int, d_pos_ptr: int, d_sched_ptr: int,
                        slots: int, budget_us: int, stream_ptr: int = 0) -> None:
        """Time-sliced run of more replicas than run at once: each of `slots`
        wavefronts continues its replica and, once that replica's range is done
        (or it halted), takes the next unstarted one (pu_run_device_pool)."""
        call("pu_run_device_pool", self._handle(), d_reqs_ptr, d_off_ptr, d_delay_ptr, d_pos_ptr, d_sched_ptr,
             slots, budget_us, stream_ptr or None)

    def fork_replica(self, src: int, first: int = 0, n: Optional[int] = None, by_copies: bool = False,
                     stream_ptr: int = 0) -> None:
        """Replicas [first, first + n) (n = None: to the last) become bit-for-bit copies of
        replica src (pu_replica_fork), asynchronously on stream_ptr like run_device; src
        inside the range is left as it is.  Their statistics, reports and completion cycles
        are then the source's, warm-up included.  by_copies: one device-to-device copy per
        destination instead of the kernel."""
        call("pu_replica_fork", self._handle(), src, first, _to_end(self.replicas, first, n),
             A.PU_FORK_BY_COPIES if by_copies else 0, stream_ptr or None)

    def synchronize(self) -> None:
        call("pu_synchronize", self._handle())

    def last_kernel_ms(self) -> float:
        return float(lib().pu_last_kernel_ms(self._handle()))

    def last_launch_kernel(self) -> str:
        """Symbol name of the engine kernel the handle launched last
        (pu_last_launch_kernel), "" before any launch."""
        return lib().pu_last_launch_kernel(self._handle()).decode()

    def set_resident(self, mode: int) -> int:
        """Resident mode for uncore_access / short batches (pu_set_resident):
        1 on, 0 off, -1 query; returns the previous mode."""
        return counted("pu_set_resident", self._handle(), mode)

    def resident_info(self) -> dict:
        """The resident kernel (pu_resident_info): running, commands served,
        kernels launched, eligible, and per command the mean kernel-side phases
        (request copy, message loop, close, mailbox) and host-side call time in µs."""
        out = (C.c_uint64 * 10)()
        counted("pu_resident_info", self._handle(), out, 10)
        n = max(1, int(out[1]))
        nfull = max(1, int(out[1]) - int(out[9]))
        sums_us = {"request_copy": out[4] / 100, "message_loop": out[5] / 100, "close": out[6] / 100,
                   "mailbox": out[7] / 100, "host_call": out[8] / 1000}
        return {"running": bool(out[0]), "commands": int(out[1]), "launches": int(out[2]), "eligible": bool(out[3]),
                "fast_answers": int(out[9]), "sums_us": sums_us,
                "mean_us": {k: v / (n if k == "host_call" else nfull) for k, v in sums_us.items()}}

    def stats(self, replica: int = 0) -> A.Stats:
        s = A.Stats()
        call("pu_stats_get", self._handle(), replica, C.byref(s))
        return s

    def completion(self, replica: int = 0) -> np.ndarray:
        n = self.cfg.sys.num_cores
        out = np.zeros(n, dtype=np.int64)
        call("pu_core_completion", self._handle(), replica, out.ctypes.data, n)
        return out

    # UncoreManager::report (uncore_manager.cpp:87-98)
    def report(self, replica: int = 0, include_time: bool = False) -> str:
        n = counted("pu_report", self._handle(), replica, int(include_time), None, 0)
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
    call("pu_unit_queue_run", min_proc, t.ctypes.data, p.ctypes.data, len(t), out.ctypes.data, C.byref(calls), device)
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
    call("pu_unit_network_run", nodes, net_type, data_width, header_flits, router_delay, link_delay,
         inject_delay, src.ctypes.data, dst.ctypes.data, ln.ctypes.data, timer.ctypes.data, len(src),
         out.ctypes.data, C.byref(st), device)
    return out, st
