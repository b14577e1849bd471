"""primesim_amd — MI355X-native uncore timing engine for PriME's memory-system hot path.

The product is the HIP engine in libprimeuncore.so (C ABI: include/primeuncore.h);
this package is its Python host mirror, the config_prime schema (`config`) and the
ctypes ABI definitions (`_abi`: the record layouts and constants).  `_native` loads
the library, holds the ctypes signature table and the one rule for turning an entry's
return value into `UncoreError`; the mirror itself is by concern in `engine`
(`UncoreManager`, the config loaders), `streams`, `traces`, `delays`, `results` and
`msglog`, with `server` on top.  `uncore` re-exports all of it under one name.
"""
from . import _abi, config  # noqa: F401
from .uncore import (DeviceDelayHistogram, DeviceDelaySummary, DeviceDelayTail, DeviceRunResults, DeviceStreamSet, DeviceTraceSet, InsMem, StreamSet, StreamSpec, UncoreError, UncoreManager, config_from_dict,  # noqa: F401
                     generate_stream, load_config, msglog_from_stream, msglog_read, parse_config,
                     pack_req16, stream_fits_req16, stream_threads, summarize_delays, MsgLogWriter,
                     host_run_results, queue_ends, delay_histogram, histogram_quantiles, dhist_bucket_of,
                     dhist_bucket_bounds, delay_tail, place_trace, placement_seed, random_placements)
# bound as attributes, not listed: __all__ is pinned by tests/test_python_mirror.py
from .uncore import DeviceDelaySeries, delay_series, dseries_epoch_of  # noqa: F401

__all__ = ["DeviceDelayHistogram", "DeviceDelaySummary", "DeviceDelayTail", "DeviceRunResults", "DeviceStreamSet", "DeviceTraceSet", "InsMem", "StreamSet", "StreamSpec", "UncoreError", "UncoreManager", "config_from_dict", "generate_stream",
           "load_config", "msglog_from_stream", "msglog_read", "MsgLogWriter", "pack_req16", "parse_config",
           "stream_fits_req16", "stream_threads", "summarize_delays", "host_run_results", "queue_ends",
           "delay_histogram", "histogram_quantiles", "dhist_bucket_of", "dhist_bucket_bounds", "place_trace",
           "placement_seed", "random_placements", "delay_tail"]
