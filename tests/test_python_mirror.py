"""The Python mirror's own rules: the ctypes signature table declares exactly what
include/primeuncore.h declares, primesim_amd.uncore exports every name its users take from
it, every wrapper raises in one form while a raw call returns the entry's code, and the six
device sets share one base."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import primesim_amd as P
from abi_helpers import ROOT
from primesim_amd import _abi as A
from primesim_amd import config as CF
from primesim_amd import uncore as U
from primesim_amd._native import SIGNATURES


def declared_entries() -> dict:
    """name -> number of parameters of every pu_* function include/primeuncore.h declares."""
    with open(os.path.join(ROOT, "include", "primeuncore.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"^[A-Za-z_][\w \*]*?\b(pu_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = m.group(2).strip()
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_signature_table_declares_the_header():
    """An entry the table lacks would return int (a truncated handle or char*); one it has too many
    of, or with the wrong number of arguments, is a declaration the header does not make."""
    want = declared_entries()
    assert len(want) >= 137
    assert set(SIGNATURES) == set(want), sorted(set(SIGNATURES) ^ set(want))
    wrong = {n: (len(SIGNATURES[n][1]), want[n]) for n in want if len(SIGNATURES[n][1]) != want[n]}
    assert not wrong, wrong


PACKAGE_ALL = [
    "DeviceDelayHistogram", "DeviceDelaySummary", "DeviceDelayTail", "DeviceRunResults", "DeviceStreamSet",
    "DeviceTraceSet", "InsMem", "StreamSet", "StreamSpec", "UncoreError", "UncoreManager", "config_from_dict",
    "generate_stream", "load_config", "msglog_from_stream", "msglog_read", "MsgLogWriter", "pack_req16",
    "parse_config", "stream_fits_req16", "stream_threads", "summarize_delays", "host_run_results", "queue_ends",
    "delay_histogram", "histogram_quantiles", "dhist_bucket_of", "dhist_bucket_bounds", "place_trace",
    "placement_seed", "random_placements", "delay_tail"]
FACADE_ONLY = [
    "lib", "last_error", "LIB_PATH", "library_source_hash", "PU_ERRORS", "PU_REPLAY_OPEN", "PU_REPLAY_CLOSED",
    "PU_REQ_FMT_32", "PU_REQ_FMT_16", "QUEUE_KINDS", "MSGMEM_DTYPE", "MSG_MEM_REQUESTS", "MSG_PROCESS_STARTING",
    "MSG_PROCESS_FINISHING", "MSG_BARRIER", "MSG_NEW_THREAD", "MSG_THREAD_FINISHING", "MSG_PROGRAM_EXITING",
    "unit_queue", "unit_network"]


def test_facade_is_whole():
    assert set(P.__all__) == set(PACKAGE_ALL) and len(P.__all__) == len(PACKAGE_ALL)
    missing = [n for n in PACKAGE_ALL + FACADE_ONLY if not hasattr(U, n)]
    assert not missing, missing
    assert all(getattr(P, n) is getattr(U, n) for n in PACKAGE_ALL)
    assert (U.PU_REQ_FMT_32, U.PU_REQ_FMT_16) == (A.PU_REQ_FMT_32, A.PU_REQ_FMT_16) == (0, 1)
    assert (U.PU_REPLAY_OPEN, U.PU_REPLAY_CLOSED) == (A.PU_REPLAY_OPEN, A.PU_REPLAY_CLOSED) == (0, 1)


def _unpackable():
    reqs = np.zeros(3, dtype=A.REQ_DTYPE)
    reqs[2]["tag"] = 1                     # pu_req16 has no room for a tag
    return P.pack_req16(reqs)


@pytest.mark.parametrize("wrapper,form", [
    (lambda: P.dhist_bucket_bounds(-1), r"^pu_dhist_bucket_bounds: .+ \(-\d+\)$"),                       # call
    (_unpackable, r"^pu_pack_req16: request \d+ does not fit.* \(-34\)$"),                               # call
    (lambda: P.DeviceDelayHistogram(0), r"^pu_dhist_open: .*no replicas"),                               # opened
    (lambda: P.generate_stream(P.StreamSpec(kind=99, num_cores=16)), r"^pu_stream_count: .+ \(-\d+\)$"),  # counted
], ids=["call", "call-pack", "opened", "counted"])
def test_one_error_form(wrapper, form):
    """Every wrapper raises "<entry>: <the library's text> (<code>)"; the rule is in the helpers, not
    in the library object, so a raw call goes on returning the code."""
    with pytest.raises(P.UncoreError, match=form):
        wrapper()
    lo, hi = C.c_int32(), C.c_int32()
    assert U.lib().pu_dhist_bucket_bounds(-1, C.byref(lo), C.byref(hi)) < 0


def _open_set(kind):
    """(set, the manager it reads or None, a call of the set) at the smallest shape it opens with."""
    specs = [P.StreamSpec(kind=A.PU_STREAM_UNIFORM, num_cores=2, seed=s, max_requests=4) for s in (1, 2)]
    if kind == "DeviceStreamSet":
        s = P.DeviceStreamSet(specs)
        return s, None, s.positions
    if kind == "DeviceTraceSet":
        trace = P.generate_stream(specs[0])
        assert len(trace) == 4
        s = P.DeviceTraceSet(trace, 2, 2)
        return s, None, s.position
    if kind == "DeviceRunResults":
        um = P.UncoreManager()
        um.init(P.config_from_dict(CF.preset("C1")), replicas=2)
        s = P.DeviceRunResults(um)
        return s, um, s.gather
    s = {"DeviceDelaySummary": lambda: P.DeviceDelaySummary(2), "DeviceDelayHistogram": lambda: P.DeviceDelayHistogram(2),
         "DeviceDelayTail": lambda: P.DeviceDelayTail(2, k=1)}[kind]()
    return s, None, s.read


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["DeviceStreamSet", "DeviceTraceSet", "DeviceDelaySummary", "DeviceDelayHistogram",
                                  "DeviceDelayTail", "DeviceRunResults"])
def test_device_sets_share_one_base(kind):
    s, um, use = _open_set(kind)
    try:
        assert type(s).__name__ == kind
        assert len(s) == 2
        assert s.state_bytes > 0
        s.close()
        s.close()
        with pytest.raises(P.UncoreError, match=f"{kind} is closed"):
            use()
    finally:
        s.close()
        if um is not None:
            um.close()
