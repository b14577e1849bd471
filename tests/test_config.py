"""config_prime XML schema loader vs the reference's XmlParser (xml_parser.cpp)."""
import ctypes as C
import hashlib
import json
import os

import pytest

import primesim_amd as P
from abi_helpers import run_cpp_check
from primesim_amd import _abi as A
from primesim_amd import config as CF
from golden_util import GOLDEN, case_names


def _as_dict(cfg):
    """The XmlSim fields (pu_sys_cfg.dram, the opt-in bank model, has no XmlSys counterpart)."""
    def conv(o):
        if isinstance(o, (A.CacheCfg, A.NetCfg, A.SysCfg, A.SimCfg)):
            return {k: conv(getattr(o, k)) for k, _ in o._fields_ if not k.startswith("_") and k != "dram"}
        if hasattr(o, "__len__") and not isinstance(o, (str, bytes)):
            return [conv(x) for x in o]
        return o
    return conv(cfg)


def _strip_unused_levels(d):
    n = d["sys"]["num_levels"]
    d["sys"]["cache"] = d["sys"]["cache"][:n]
    return d


def test_schema_fixtures_match_reference_parser():
    with open(os.path.join(GOLDEN, "configs.json")) as f:
        fx = json.load(f)
    for name, v in fx.items():
        got = _strip_unused_levels(_as_dict(P.parse_config(v["xml"])))
        want = _strip_unused_levels(v["xmlsim"])
        assert got == want, name


@pytest.mark.parametrize("name", case_names())
def test_golden_case_configs(name):
    with open(os.path.join(GOLDEN, f"{name}.json")) as f:
        want = _strip_unused_levels(json.load(f)["xmlsim"])
    got = _strip_unused_levels(_as_dict(P.load_config(os.path.join(GOLDEN, f"{name}.xml"))))
    assert got == want


def test_config_prime_default_values():
    cfg = P.config_from_dict(CF.default_config())
    assert cfg.max_msg_size == 100 and cfg.thread_sync_interval == 1000 and cfg.num_recv_threads == 1
    assert cfg.sys.num_levels == 3 and cfg.sys.num_cores == 64 and cfg.sys.tlb_enable == 1
    assert cfg.sys.cache[2].share == 64 and cfg.sys.directory_cache.size == 31457280
    assert cfg.sys.network.link_delay == 1 and cfg.sys.freq == 2.5


def test_optional_fields_default_to_zero():
    sim = CF.preset("C1")
    del sim["system"]["max_num_sharers"]
    del sim["system"]["network"]["inject_delay"]
    cfg = P.config_from_dict(sim)
    assert cfg.sys.max_num_sharers == 0 and cfg.sys.network.inject_delay == 0


@pytest.mark.parametrize("mutate", [
    lambda s: s.pop("max_msg_size"),                               # simulator count 4 != 5
    lambda s: s["system"].pop("freq"),                             # system count 12 != 13
    lambda s: s["system"]["network"].pop("data_width"),            # network count 3 != 4
    lambda s: s["system"]["directory_cache"].pop("num_ways"),      # directory 5 != 6
    lambda s: s["system"].pop("tlb_cache"),                        # //tlb_cache missing
    lambda s: s["system"]["cache"].pop(),                          # //cache count != num_levels
])
def test_schema_errors_are_reported(mutate):
    sim = CF.default_config()
    mutate(sim)
    with pytest.raises(P.UncoreError):
        P.config_from_dict(sim)


def test_malformed_xml():
    with pytest.raises(P.UncoreError):
        P.parse_config("<simulator><max_msg_size>1</simulator>")


def test_numeric_parse_semantics():
    """`stringstream >> dec >> v`: leading blanks skipped, numeric prefix taken."""
    xml = CF.to_xml(CF.preset("C1")).replace("<num_cores>16</num_cores>", "<num_cores>\n   16abc </num_cores>")
    assert P.parse_config(xml).sys.num_cores == 16


def test_write_xml_round_trip():
    import ctypes as C
    cfg = P.config_from_dict(CF.preset("C3"))
    n = C.c_size_t(0)
    buf = C.create_string_buffer(1 << 16)
    assert P.uncore.lib().pu_config_write_xml(C.byref(cfg), buf, len(buf), C.byref(n)) == 0
    again = P.parse_config(buf.value.decode())
    assert _as_dict(again) == _as_dict(cfg)


def _geo_source_sha(cfg) -> str:
    n = P.uncore.lib().pu_config_geo_source(C.byref(cfg), None, 0)
    assert n > 0, P.uncore.last_error()
    buf = C.create_string_buffer(n + 1)
    assert P.uncore.lib().pu_config_geo_source(C.byref(cfg), buf, n + 1) == n
    return hashlib.sha256(buf.value).hexdigest()


def test_geometry_of_every_known_configuration_is_the_recorded_one(monkeypatch):
    """tests/golden/geo_source.json holds, for every XML under tests/golden and the
    presets C1-C5, the sha256 of pu_config_geo_source's text as the commit under
    "_from" produced it.  Every offset, count and flag of a Geo is in that text, so
    the validation and the replica layout (geometry.cpp) are pinned field by field."""
    for k in ("PRIMEUNCORE_POOL_ENTRIES", "PRIMEUNCORE_PAGE_ENTRIES"):   # both size a part of the layout
        monkeypatch.delenv(k, raising=False)
    with open(os.path.join(GOLDEN, "geo_source.json")) as f:
        want = json.load(f)
    assert len(want.pop("_from")) == 40
    xmls = sorted(os.path.splitext(n)[0] for n in os.listdir(GOLDEN) if n.endswith(".xml"))
    presets = ["C1", "C2", "C3", "C4", "C5"]
    assert sorted(want) == sorted(xmls + [f"preset:{p}" for p in presets])
    got = {name: _geo_source_sha(P.load_config(os.path.join(GOLDEN, f"{name}.xml"))) for name in xmls}
    got.update({f"preset:{p}": _geo_source_sha(P.config_from_dict(CF.preset(p))) for p in presets})
    assert {k: v for k, v in got.items() if v != want[k]} == {}


PU_ENOTSUP = -95   # include/primeuncore.h


def _geometry_rc(sim) -> tuple:
    """pu::config_geometry's code and text for a configuration (pu_config_queue_ends returns both as they are)."""
    cfg = P.config_from_dict(sim)
    kind, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = P.uncore.lib().pu_config_queue_ends(C.byref(cfg), 0, C.byref(kind), C.byref(a), C.byref(b))
    return rc, (P.uncore.last_error() if rc else "")


def _shared_l2(cores: int, share: int) -> dict:
    sim = CF.preset("C1")
    s = sim["system"]
    s["num_cores"] = cores
    s["num_levels"] = 2
    s["cache"] = [
        {"level": 0, "share": 1, "access_time": 1, "size": 8192, "block_size": 64, "num_ways": 4},
        {"level": 1, "share": share, "access_time": 6, "size": 65536, "block_size": 64, "num_ways": 8},
    ]
    return sim


@pytest.mark.parametrize("cores,share,ok", [(9, 2, False), (2, 8, False), (10, 4, False), (12, 4, True),
                                            (64, 4, True)])
def test_a_level_whose_children_do_not_fill_the_last_parent_is_refused(cores, share, ok):
    """The reference counts a level's caches with a ceil (system.cpp:76) but gives
    every parent share[l] / share[l-1] children (system.cpp:184-188): the last
    parent of an unfilled level reads child pointers past its level's array."""
    rc, text = _geometry_rc(_shared_l2(cores, share))
    if ok:
        assert rc == 0, text
    else:
        assert rc == PU_ENOTSUP and "system.cpp:184-188" in text and "system.cpp:76" in text
        with pytest.raises(P.UncoreError, match="fill every parent"):    # refused before any device is touched
            P.UncoreManager().init(P.config_from_dict(_shared_l2(cores, share)))


def test_unfilled_parents_are_refused_at_every_level():
    sim = _shared_l2(12, 2)      # 12 L1, 6 L2; an L3 of share 8 takes 4 L2 each: 6 % 4 != 0
    sim["system"]["num_levels"] = 3
    sim["system"]["cache"].append({"level": 2, "share": 8, "access_time": 9, "size": 131072, "block_size": 64,
                                   "num_ways": 8})
    assert _geometry_rc(sim)[0] == PU_ENOTSUP
    sim["system"]["num_cores"] = 16
    assert _geometry_rc(sim) == (0, "")


@pytest.mark.parametrize("sys_type", [0, 1])
def test_zero_flit_packets_are_refused(sys_type):
    """header_flits = 0 makes a message without data a packet of no flits
    (network.cpp:104).  The reference's free intervals then touch, so which of
    two its tree search returns depends on the tree's shape
    (queue_model_history_tree.cpp:66), and a link that has carried only such
    packets has a service rate of 1/0, whose waiting time is a NaN cast to an
    integer (queue_model_m_g_1.cpp:28-35): neither is restated."""
    for hf, want in ((0, PU_ENOTSUP), (-1, PU_ENOTSUP), (1, 0)):
        sim = CF.preset("C1", header_flits=hf, sys_type=sys_type)
        rc, text = _geometry_rc(sim)
        assert rc == want, text
        if want:
            assert "header_flits must be >= 1" in text and "network.cpp:104" in text
            with pytest.raises(P.UncoreError, match="header_flits"):
                P.UncoreManager().init(P.config_from_dict(sim))


def test_host_geometry_under_the_sanitizers(tmp_path):
    """common.cpp, config.cpp and geometry.cpp need no HIP: tests/cpp/geometry_check.cpp
    runs them under the address and undefined-behaviour sanitizers (144 links of the
    3D mesh, 16 buses of the bus system, 24 links of the TLB configuration; the
    refusals of unfilled parents and of zero-flit packets)."""
    assert run_cpp_check(tmp_path, "geometry_check.cpp").startswith("OK 184 queues")


def test_dram_bank_element_round_trip():
    """The optional <dram> element (pu_dram_cfg) parses, is written back only
    when banks > 0, and malformed or partial elements are refused."""
    sim = CF.default_config()
    assert P.config_from_dict(sim).sys.dram.banks == 0
    sim["system"]["dram"] = {"banks": 16, "row_bytes": 8192, "t_rcd": 14, "t_rp": 14, "t_burst": 4}
    cfg = P.config_from_dict(sim)
    d = cfg.sys.dram
    assert (d.banks, d.row_bytes, d.t_rcd, d.t_rp, d.t_burst) == (16, 8192, 14, 14, 4)
    buf, n = C.create_string_buffer(1 << 16), C.c_size_t(0)
    assert P.uncore.lib().pu_config_write_xml(C.byref(cfg), buf, len(buf), C.byref(n)) == 0
    text = buf.value.decode()
    assert "<dram>" in text and P.parse_config(text).sys.dram.row_bytes == 8192
    del sim["system"]["dram"]["t_rp"]
    with pytest.raises(P.UncoreError):
        P.config_from_dict(sim)
