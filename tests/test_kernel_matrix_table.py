"""The golden x kernel matrix's table (kernel_matrix.py), checked without a GPU:
the cells and the exclusions cover every (golden, kernel) pair exactly once,
the exclusions are the six cells whose queue headers cannot fit the LDS image,
and a golden added later gets its six cells without an edit."""
import os
import re
from collections import Counter

import golden_util
import kernel_matrix as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_names_are_the_engines_own():
    """The six names are the kernels engine.hip defines and jit.cpp loads."""
    with open(os.path.join(ROOT, "primesim_amd", "csrc", "engine.hip")) as f:
        defined = set(re.findall(r"^PU_JIT_KERNEL\((pu_jit_uncore_s\d_h\d),", f.read(), flags=re.M))
    with open(os.path.join(ROOT, "primesim_amd", "csrc", "jit.cpp")) as f:
        loaded = set(re.findall(r'"(pu_jit_uncore_s\d_h\d)"', f.read()))
    assert set(KM.KERNELS) == defined == loaded
    assert len(KM.KERNELS) == len(set(KM.KERNELS)) == 6


def test_cells_and_exclusions_cover_every_pair_once():
    names = golden_util.case_names()
    assert len(names) >= 39 and not any(n.startswith("big_") for n in names)
    every = Counter((g, k) for g in names for k in KM.KERNELS)
    got = Counter(KM.cells()) + Counter(KM.EXCLUDED.keys())
    assert got == every                                   # each pair once: no cell twice, none lost
    assert not set(KM.cells()) & set(KM.EXCLUDED)
    assert len(KM.cells()) == 6 * len(names) - 6


def test_exclusions_are_the_six_lds_cells():
    lds = ("pu_jit_uncore_s0_h1", "pu_jit_uncore_s1_h1", "pu_jit_uncore_s3_h1")
    assert set(KM.EXCLUDED) == {(g, k) for g in ("c5_prodcons", "mesh_8192") for k in lds}
    assert all(isinstance(r, str) and "3,400" in r for r in KM.EXCLUDED.values())
    # the reason, from the fixtures' own XML (not from the library): the
    # 2-D mesh of ceil(sqrt(N)) columns has 2 w (w - 1) link queues
    with open(os.path.join(ROOT, "primesim_amd", "csrc", "engine.hip")) as f:
        lds_q = int(re.search(r"^#define PU_LDS_Q (\d+)u", f.read(), flags=re.M).group(1))
    assert lds_q == 3400
    for g, width in (("c5_prodcons", 64), ("mesh_8192", 91)):
        assert 2 * width * (width - 1) > lds_q


def test_a_new_golden_is_picked_up(monkeypatch):
    names = golden_util.case_names()
    monkeypatch.setattr(KM, "case_names", lambda: names + ["zz_added_later"])
    new = [c for c in KM.cells() if c[0] == "zz_added_later"]
    assert new == [("zz_added_later", k) for k in KM.KERNELS]
    assert len(KM.cells()) == 6 * (len(names) + 1) - 6


def test_host_chunks_cut_inside_a_message():
    """Every golden's access_batch chunks hold a cut that is not a message
    boundary, tile the stream, and respect the resident command size."""
    for g in golden_util.case_names():
        c = KM.case(g)
        n = len(c.reqs)
        for cap in (None, KM.RESIDENT_CAP):
            cuts = KM.host_cuts(c.reqs, cap)
            assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:]))
            assert len(cuts) >= 4
            assert any(c.reqs["batch_start"][x] == 0 for x in cuts[1:-1])
            if cap:
                assert max(b - a for a, b in zip(cuts, cuts[1:])) <= cap
        h = KM.second_half_start(c.reqs)
        assert n // 2 <= h < n and c.reqs["batch_start"][h] == 1
        # four slices or more for the shortest replica at 0.5 us a request
        assert (n - h) * 0.5 >= 4 * KM.slice_budget_us(n - h)
