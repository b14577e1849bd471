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

This module is the one name the mirror is used under.  The code is in `_native` (the
library, its signature table and the rules for calling it), `engine`, `streams`,
`traces`, `delays`, `results` and `msglog`.
"""
from ._abi import PU_REPLAY_CLOSED, PU_REPLAY_OPEN, PU_REQ_FMT_16, PU_REQ_FMT_32  # noqa: F401
from ._native import LIB_PATH, PU_ERRORS, UncoreError, last_error, lib, library_source_hash  # noqa: F401
from .delays import (DeviceDelayHistogram, DeviceDelaySeries, DeviceDelaySummary, DeviceDelayTail,  # noqa: F401
                     delay_histogram, delay_series, delay_tail, dhist_bucket_bounds, dhist_bucket_of, dseries_epoch_of,
                     histogram_quantiles, summarize_delays)
from .engine import (InsMem, UncoreManager, config_from_dict, load_config, parse_config, unit_network,  # noqa: F401
                     unit_queue)
from .msglog import (MSG_BARRIER, MSG_MEM_REQUESTS, MSG_NEW_THREAD, MSG_PROCESS_FINISHING,  # noqa: F401
                     MSG_PROCESS_STARTING, MSG_PROGRAM_EXITING, MSG_THREAD_FINISHING, MSGMEM_DTYPE, MsgLogWriter,
                     msglog_from_stream, msglog_read)
from .results import QUEUE_KINDS, DeviceRunResults, host_run_results, queue_ends  # noqa: F401
from .streams import (DeviceStreamSet, StreamSet, StreamSpec, generate_stream, pack_req16,  # noqa: F401
                      stream_fits_req16, stream_threads)
from .traces import DeviceTraceSet, place_trace, placement_seed, random_placements  # noqa: F401
