"""ctypes mirror of include/primeuncore.h (structs, constants).

Shared by the product binding (the signature table in primesim_amd._native and the
modules that call it) and the test harness.  Each record layout is stated once, as a
ctypes.Structure; the numpy dtype of a record is made from its Structure.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

PU_MAX_LEVELS = 4

PU_RD, PU_WR, PU_WB = 0, 1, 2

PU_STREAM_PRIVATE_STREAMING = 1
PU_STREAM_SHARED_UNIFORM = 2
PU_STREAM_MULTIPROGRAM = 3
PU_STREAM_UNIFORM_HOTSPOT = 4
PU_STREAM_PRODUCER_CONSUMER = 5
PU_STREAM_UNIFORM = 6

PU_REQ_FMT_32, PU_REQ_FMT_16 = 0, 1      # device request records: pu_req, pu_req16
PU_REPLAY_OPEN, PU_REPLAY_CLOSED = 0, 1  # pu_set_replay_mode

PU_DSUM_BUCKETS = 32                     # delay summaries (pu_dsum_*)
PU_DHIST_SUB_BITS, PU_DHIST_BUCKETS, PU_DHIST_MAX_Q = 5, 864, 8     # log-linear delay histograms (pu_dhist_*)
PU_DTAIL_MAX_K = 64                      # the longest list of slowest requests (pu_dtail_*)
PU_DSERIES_MAX_EPOCHS = 512              # the most epochs of an epoch series (pu_dseries_*)

PU_ERRF_CORE_RANGE = 1 << 0
PU_ERRF_WB_MISS = 1 << 1
PU_ERRF_EMPTY_SHARER = 1 << 2
PU_ERRF_QUEUE = 1 << 3
PU_ERRF_NEG_DELAY = 1 << 4
PU_ERRF_POOL = 1 << 5
PU_ERRF_PAGES = 1 << 6
PU_ERRF_PROG = 1 << 7
PU_ERRF_LIMITS = PU_ERRF_WB_MISS | PU_ERRF_EMPTY_SHARER | PU_ERRF_QUEUE | PU_ERRF_POOL | PU_ERRF_PAGES | PU_ERRF_PROG


class CacheCfg(C.Structure):
    _fields_ = [
        ("level", C.c_int32), ("share", C.c_int32), ("access_time", C.c_int32), ("_pad", C.c_int32),
        ("size", C.c_uint64), ("block_size", C.c_uint64), ("num_ways", C.c_uint64),
    ]


class NetCfg(C.Structure):
    _fields_ = [
        ("data_width", C.c_int32), ("header_flits", C.c_int32), ("net_type", C.c_int32), ("_pad", C.c_int32),
        ("router_delay", C.c_uint64), ("link_delay", C.c_uint64), ("inject_delay", C.c_uint64),
    ]


class DramCfg(C.Structure):              # pu_dram_cfg (opt-in bank model)
    _fields_ = [
        ("banks", C.c_int32), ("t_rcd", C.c_int32), ("t_rp", C.c_int32), ("t_burst", C.c_int32),
        ("row_bytes", C.c_uint64),
    ]


class SysCfg(C.Structure):
    _fields_ = [
        ("sys_type", C.c_int32), ("protocol_type", C.c_int32), ("max_num_sharers", C.c_int32),
        ("page_size", C.c_int32), ("tlb_enable", C.c_int32), ("shared_llc", C.c_int32),
        ("verbose_report", C.c_int32), ("dram_access_time", C.c_int32), ("cpi_nonmem", C.c_double),
        ("num_levels", C.c_int32), ("num_cores", C.c_int32), ("freq", C.c_double),
        ("bus_latency", C.c_int32), ("page_miss_delay", C.c_int32),
        ("network", NetCfg), ("directory_cache", CacheCfg), ("tlb_cache", CacheCfg),
        ("cache", CacheCfg * PU_MAX_LEVELS), ("dram", DramCfg),
    ]


class SimCfg(C.Structure):
    _fields_ = [
        ("max_msg_size", C.c_int32), ("num_recv_threads", C.c_int32), ("thread_sync_interval", C.c_int32),
        ("proc_sync_interval", C.c_int32), ("syscall_cost", C.c_int32), ("_pad", C.c_int32),
        ("sys", SysCfg),
    ]


class LevelStats(C.Structure):
    _fields_ = [("ins", C.c_uint64), ("miss", C.c_uint64), ("evict", C.c_uint64), ("wb", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [
        ("net_accesses", C.c_uint64), ("net_distance", C.c_uint64), ("net_total_delay", C.c_uint64),
        ("net_router_delay", C.c_uint64), ("net_link_delay", C.c_uint64), ("net_inject_delay", C.c_uint64),
        ("dram_accesses", C.c_uint64), ("total_bus_contention", C.c_uint64), ("total_num_broadcast", C.c_int64),
        ("num_levels", C.c_int32), ("_pad", C.c_int32),
        ("level", LevelStats * PU_MAX_LEVELS), ("directory", LevelStats), ("tlb", LevelStats),
        ("link_flits", C.c_uint64), ("mg1_calls", C.c_uint64), ("lockdown_calls", C.c_uint64),
        ("bus_accesses", C.c_uint64), ("requests", C.c_uint64), ("error_flags", C.c_uint64),
        ("dram_row_hits", C.c_uint64), ("dram_row_empty", C.c_uint64), ("dram_row_conflicts", C.c_uint64),
        ("dram_bank_wait", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {}
        for name, _ in self._fields_:
            if name.startswith("_"):
                continue
            v = getattr(self, name)
            if name == "level":
                for i in range(self.num_levels):
                    for f in ("ins", "miss", "evict", "wb"):
                        d[f"L{i}_{f}"] = getattr(v[i], f)
            elif isinstance(v, LevelStats):
                for f in ("ins", "miss", "evict", "wb"):
                    d[f"{name}_{f}"] = getattr(v, f)
            else:
                d[name] = v
        return d


class StreamParams(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("num_cores", C.c_int32), ("seed", C.c_uint64), ("quantum", C.c_int32),
        ("num_quanta", C.c_int32), ("max_msg", C.c_int32), ("num_progs", C.c_int32),
        ("max_requests", C.c_int64), ("write_pct", C.c_int32), ("_pad", C.c_int32),
    ]


class DsumClass(C.Structure):           # pu_dsum_class
    _fields_ = [
        ("count", C.c_uint64), ("sum", C.c_int64), ("min", C.c_int32), ("max", C.c_int32),
        ("hist", C.c_uint64 * PU_DSUM_BUCKETS),
    ]


class DsumReplica(C.Structure):         # pu_dsum_replica
    _fields_ = [("cls", DsumClass * 2), ("core_out_of_range", C.c_uint64)]


class DhistQuantile(C.Structure):       # pu_dhist_quantile
    _fields_ = [("count", C.c_uint64), ("bucket", C.c_int32 * PU_DHIST_MAX_Q)]


class DtailEntry(C.Structure):          # pu_dtail_entry
    _fields_ = [("addr", C.c_uint64), ("timer", C.c_int64), ("position", C.c_uint64), ("delay", C.c_int32),
                ("core", C.c_int32)]


class DseriesCell(C.Structure):         # pu_dseries_cell
    _fields_ = [("count", C.c_uint64), ("sum", C.c_int64), ("nonpos", C.c_uint64), ("max", C.c_int32),
                ("_pad", C.c_int32)]


class DresReplica(C.Structure):         # pu_dres_replica
    _fields_ = [
        ("stats", Stats), ("processed", C.c_uint64), ("halted", C.c_int32), ("cores_done", C.c_int32),
        ("completion_max", C.c_int64), ("completion_min", C.c_int64), ("completion_sum", C.c_int64),
        ("link_visits", C.c_uint64), ("link_block_visits", C.c_uint64), ("link_max_visits", C.c_uint64),
        ("link_max_id", C.c_int32), ("links_used", C.c_int32),
        ("bus_visits", C.c_uint64), ("bus_max_visits", C.c_uint64),
        ("bus_max_id", C.c_int32), ("buses_used", C.c_int32),
    ]


class ServerOpts(C.Structure):          # pu_server_opts
    _fields_ = [
        ("socket_path", C.c_char_p), ("report_prefix", C.c_char_p), ("num_sessions", C.c_int32),
        ("num_recv_threads", C.c_int32), ("max_msg_size", C.c_int32), ("verbose", C.c_int32),
    ]


class ServerStats(C.Structure):         # pu_server_stats
    _fields_ = [
        ("rounds", C.c_uint64), ("launches", C.c_uint64), ("messages", C.c_uint64), ("requests", C.c_uint64),
        ("sessions_ended", C.c_int32), ("sessions_halted", C.c_int32),
        ("sessions_failed", C.c_int32), ("_pad", C.c_int32),
    ]


# pu_exec_fn(ctx, session, reqs, n, delays)
EXEC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)


# pu_req as a numpy structured dtype (32 bytes, matches the C struct layout)
REQ_DTYPE = np.dtype([
    ("addr", "<u8"), ("timer", "<i8"), ("core", "<i4"), ("prog_id", "<i4"),
    ("mem_type", "u1"), ("batch_start", "u1"), ("tag", "<u2"), ("_pad1", "<i4"),
])
assert REQ_DTYPE.itemsize == 32
# The records the readers return, as numpy structured dtypes: each is its Structure's layout
DSUM_CLASS_DTYPE, DSUM_DTYPE = np.dtype(DsumClass), np.dtype(DsumReplica)
DHIST_Q_DTYPE = np.dtype(DhistQuantile)
DTAIL_DTYPE = np.dtype(DtailEntry)
DSERIES_DTYPE = np.dtype(DseriesCell)
LEVEL_STATS_DTYPE, STATS_DTYPE, DRES_DTYPE = np.dtype(LevelStats), np.dtype(Stats), np.dtype(DresReplica)
# the sizes pin the layouts to include/primeuncore.h
assert C.sizeof(LevelStats) == 32 and C.sizeof(DtailEntry) == 32 and C.sizeof(DhistQuantile) == 40
assert C.sizeof(DseriesCell) == 32
assert C.sizeof(Stats) == 352 and C.sizeof(DresReplica) == 448 and C.sizeof(DsumReplica) == 568
PU_DRES_QUEUES = 1                       # pu_dres_open: keep the per-queue map
PU_FORK_BY_COPIES = 1                    # pu_replica_fork: one device-to-device copy per destination
assert C.sizeof(SimCfg) == 24 + C.sizeof(SysCfg)


def ptr(a: np.ndarray, ctype=C.c_void_p):
    """Raw pointer to a contiguous numpy array."""
    assert a.flags["C_CONTIGUOUS"]
    return C.cast(a.ctypes.data, ctype)
