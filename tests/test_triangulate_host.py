"""eg3d_host_triangulate (include/eg3d_host_triangulate.h) == the oracle, bit for bit — valid, flags, and X where valid —
for both forms of the DLT system, on the tables of tests/triangulate_cases.py: the three rigs of coop_gn_cases.rigs(), every
row count of coop_gn_cases.ROWS, 4096 rows once, lengths 0 and 1, every kind in EG3D_TRI_REFINE, and in
EG3D_TRI_FROM_SCRATCH the kinds near / wild / singular / nan_obs plus the three cases of the DLT's choice of entries. A
track that is not valid keeps X0 (REFINE) or gets +0.0 (FROM_SCRATCH). Thread counts 1 and 4 give the same bytes. Then what
include/eg3d_triangulate.h promises beyond its signatures (those are held by tests/test_abi.py): the modes and flags, the
wrappers, the build guard's bound on K14. No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import forms
import test_abi
import triangulate_cases as tc
from edgegraph3d_amd import api, build, host

RIGS = ("c5", "wide", "tiny")


@functools.lru_cache(maxsize=None)
def reference(rig_name, mode, rows):
    with forms.oracle_rows(rows):
        return tc.oracle_rows(tc.rigs()[rig_name], tc.table(rig_name, mode), mode)


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
@pytest.mark.parametrize("mode", (0, 1), ids=("from_scratch", "refine"))
@pytest.mark.parametrize("rig_name", RIGS)
def test_host_statement_is_the_oracle(rig_name, mode, rows):
    rig, tab = tc.rigs()[rig_name], tc.table(rig_name, mode)
    want = reference(rig_name, mode, rows)
    got1 = host.triangulate(rig.P, *tab.args(), X0=tab.X0 if mode == 1 else None, mode=mode, dlt_rows=rows, n_threads=1)
    tc.assert_same(got1, want, "%s mode %d rows %d" % (rig_name, mode, rows))
    got4 = host.triangulate(rig.P, *tab.args(), X0=tab.X0 if mode == 1 else None, mode=mode, dlt_rows=rows, n_threads=4)
    for a, b in zip(got1, got4):
        assert a.tobytes() == b.tobytes()
    # the table does what it was built for: accepted and rejected solves, short tracks, and in mode 0 degenerate pairs
    assert 0 < int(want[0].sum()) < tab.n
    assert int((want[2] & tc.FLAG_SHORT).astype(bool).sum()) == 2
    if mode == 0:
        assert int((want[2] & tc.FLAG_DEGENERATE).astype(bool).sum()) >= len(tc.cg.ROWS)  # (the `singular` tracks at least)


def test_the_dlt_choice_cases_choose_what_they_say():
    """Index of the first minimal view id and the degenerate flag of the three cases, and that the second case would start
    elsewhere had the second occurrence been taken (so a wrong choice cannot pass unnoticed)."""
    rig = tc.rigs()["c5"]
    tracks = tc.dlt_choice_tracks(rig, np.random.default_rng(7))
    first_min = [int(np.argmin(t["view"])) for t in tracks]
    assert first_min == [2, 1, 5]
    assert list(tracks[1]["view"]).count(tracks[1]["view"].min()) == 2 and not np.array_equal(tracks[1]["xy"][1], tracks[1]["xy"][3])
    assert [bool(t["view"][m] == t["view"][-1]) for t, m in zip(tracks, first_min)] == [False, False, True]
    assert len(set(tracks[2]["view"].tolist())) > 1
    tab = tc.Table(tracks)
    for rows in forms.FORMS:
        with forms.oracle_rows(rows):
            want = tc.oracle_rows(rig, tab, 0)
        assert list(want[2]) == [0, 0, tc.FLAG_DEGENERATE]
        tc.assert_same(host.triangulate(rig.P, *tab.args(), mode=0, dlt_rows=rows), want, "dlt choice rows %d" % rows)


def test_the_forms_differ_and_follow_dlt_rows():
    """The two DLT systems give different start points: on tracks that Gauss-Newton rejects or stops early the results
    differ, so a host library that ignored dlt_rows would show here."""
    rig, tab = tc.rigs()["c5"], tc.table("c5", 0)
    a = host.triangulate(rig.P, *tab.args(), mode=0, dlt_rows=3)
    b = host.triangulate(rig.P, *tab.args(), mode=0, dlt_rows=2)
    assert a[0].tobytes() != b[0].tobytes()


def test_refusals_and_empty_input():
    rig, tab = tc.rigs()["c5"], tc.table("c5", 1)
    off, view, xy = tab.args()
    X, valid, flags = host.triangulate(rig.P, np.zeros(1, np.uint32), view[:0], xy[:0], X0=tab.X0[:0], mode=1)
    assert len(X) == len(valid) == len(flags) == 0
    bad_view = view.copy()
    bad_view[5] = rig.V
    desc = off.copy()
    desc[3] = desc[4] + 1
    long_off = np.array([0, 32768], np.uint32)
    for kw in (dict(obs_view=bad_view), dict(obs_off=desc), dict(mode=2), dict(dlt_rows=4), dict(X0=None, mode=1)):
        args = dict(cam_P=rig.P, obs_off=off, obs_view=view, obs_xy=xy, X0=tab.X0, mode=1)
        args.update(kw)
        with pytest.raises(ValueError):
            host.triangulate(**args)
    with pytest.raises(ValueError):
        host.triangulate(rig.P, long_off, np.zeros(32768, np.int32), np.zeros((32768, 2), np.float32), mode=0)
    n = 32767  # the longest list that passes
    host.triangulate(rig.P, np.array([0, n], np.uint32), np.arange(n, dtype=np.int32) % rig.V, np.ones((n, 2), np.float32), mode=0)


# ---- what the header promises beyond its signatures ------------------------------------------------------------------------------
def test_the_header_states_the_modes_and_flags_and_the_wrappers_are_there():
    text = open(os.path.join(test_abi.INC, "eg3d_triangulate.h")).read()   # (header_text drops the preprocessor lines)
    for name, value in (("EG3D_TRI_FROM_SCRATCH", "0"), ("EG3D_TRI_REFINE", "1"), ("EG3D_TRI_FLAG_SHORT", "1u"),
                        ("EG3D_TRI_FLAG_DEGENERATE", "2u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), text), name
    assert (api.TRI_FROM_SCRATCH, api.TRI_REFINE, api.TRI_FLAG_SHORT, api.TRI_FLAG_DEGENERATE) == (0, 1, 1, 2)
    assert callable(host.triangulate)
    for m in ("triangulate", "triangulate_device"):
        assert callable(getattr(api.Context, m)), m


def test_the_build_guard_holds_k14():
    """No spilled register in any K14 kernel; the solve kernel within four single-wave workgroups per SIMD (128 VGPRs, 8 LDS
    allocation units); no scratch and no LDS in the other three."""
    b = build.RESOURCE_BOUNDS["k14_"]
    assert b["vgpr_spill_count"] == 0 and b["sgpr_spill_count"] == 0
    assert b["private_segment_fixed_size"] <= 64 and b["group_segment_fixed_size"] <= 10240
    assert build.RESOURCE_BOUNDS["k14_solve"]["vgpr_count"] <= 128
    for k in ("k14_check", "k14_cut", "k14_stage"):
        assert build.RESOURCE_BOUNDS[k] == {"private_segment_fixed_size": 0, "group_segment_fixed_size": 0}
