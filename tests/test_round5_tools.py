"""CPU-side checks of the round-5 infrastructure: the build guard reads the kernels' resource figures from the built
library, the structure-tolerant comparator, and the oracle's convention switches (test hook)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from edgegraph3d_amd import api, build, host
from oracle import binding as ob
from parity_util import chain_ranges, compare_by_chain, compare_edgepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_guard_reads_the_code_objects_and_the_bounds_hold():
    """tools/kernel_resources.py finds every instantiation of the expand kernel in the built library with plausible
    figures, and the committed bounds of build.py hold for it (what build_hip() enforces). Round 6: the product libraries
    no longer carry the lane-per-chain engine's kernels; the variant built with -DEG3D_WITH_K3C_ENGINE does, within its
    own bounds."""
    if not os.path.exists(api.lib_path()):
        build.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    res = {n: r for n, r in kr.kernel_resources(api.lib_path()).items() if n.startswith("eg3d::")}
    expand = [n for n in res if "k3b_expand_t<" in n]
    assert len(expand) == 3 and not [n for n in res if "k3c_engine" in n]
    if os.path.exists(build.HIP_LIB_ENGINE):
        eng = {n: r for n, r in kr.kernel_resources(build.HIP_LIB_ENGINE).items() if n.startswith("eg3d::")}
        assert len([n for n in eng if "k3c_engine_t<" in n]) == 2
        assert kr.check_bounds(eng, dict(build.RESOURCE_BOUNDS, **build.ENGINE_RESOURCE_BOUNDS)) == []
    for n in expand:
        assert res[n]["vgpr_count"] == 128 and 0 < res[n]["group_segment_fixed_size"] <= 10240, (n, res[n])
    assert kr.check_bounds(res, build.RESOURCE_BOUNDS) == []
    # a bound that is exceeded is reported, a kernel that disappeared too
    bad = kr.check_bounds(res, {"k3b_expand_t<4, 0, 0>": {"vgpr_spill_count": -1}, "no_such_kernel": {"vgpr_spill_count": 0}})
    assert len(bad) == 2 and "no kernel matches" in bad[1]
    assert len(build.device_source_fingerprint()) == 16


def test_kernel_code_diff_says_same_and_differs():
    """tools/kernel_code_diff.py can say both things. A library against itself: every kernel `same`, exit 0. libeg3d.so
    against libeg3d_dlt4x4.so (the other form of the DLT system): non-zero exit, the three k3b_expand_t instantiations among
    the differing kernels, k6_compact_scan and k7_dedup_claim (no triangulation in them) among the same."""
    if not os.path.exists(build.HIP_LIB):
        build.build_hip()
    if not os.path.exists(build.HIP_LIB_DLT4X4):
        build.build_hip_dlt4x4()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_code_diff as kd
    a = kd.kernel_code(build.HIP_LIB)
    lines, bad = kd.diff(a, a)
    assert bad == 0 and len(lines) > 100 and all(l.startswith("same ") for l in lines[:-1]), lines[-1]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_code_diff.py"), build.HIP_LIB, build.HIP_LIB_DLT4X4],
                       capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    verdict = {l[l.index("eg3d::"):]: l.split()[0] for l in r.stdout.splitlines() if "eg3d::" in l}
    expand = [n for n in verdict if n.startswith("eg3d::k3b_expand_t<")]
    assert len(expand) == 3 and all(verdict[n] == "differs" for n in expand), expand
    assert verdict["eg3d::k6_compact_scan"] == "same" and verdict["eg3d::k7_dedup_claim"] == "same"
    assert not [l for l in r.stdout.splitlines() if l.startswith("only ")]  # the two forms hold the same set of kernels


def test_compare_by_chain_matches_chains_by_key_not_by_position():
    s = host.Synth(1)
    o = ob.Oracle(s.scene)
    a = o.match(s.seeds, 0, s.n_seeds, 4)
    rep = compare_by_chain(a, a)
    assert rep["chains_structurally_identical"] == rep["chains_in_both"] == len(chain_ranges(a)) > 10
    assert rep["points_X_bit_equal"] == rep["points_compared"] == a["n_points"] and rep["obs_xy_bit_equal"] == a["n_obs"]
    # drop the first chain of one side: the strict comparison fails at once, the tolerant one loses exactly that chain
    first = chain_ranges(a)[tuple(int(x) for x in a["key"][0][:3])]
    n0, o0 = first[1], int(a["obs_off"][first[1]])
    b = dict(a)
    b["n_points"], b["n_obs"] = a["n_points"] - n0, a["n_obs"] - o0
    b["X"], b["key"] = a["X"][n0:], a["key"][n0:]
    b["obs_off"] = a["obs_off"][n0:] - a["obs_off"][n0]
    for k in ("obs_view", "obs_pl", "obs_seg", "obs_xy"):
        b[k] = a[k][o0:]
    assert not compare_edgepoints(a, b)["ok"]
    rep = compare_by_chain(a, b)
    assert rep["chains_only_ref"] == 1 and rep["chains_only_got"] == 0
    assert rep["chains_structurally_identical"] == rep["chains_in_both"] == len(chain_ranges(a)) - 1
    assert rep["points_X_bit_equal"] == rep["points_compared"] == b["n_points"]


def test_oracle_convention_switches_are_a_hook_and_default_off():
    """orc_set_conventions(mask) changes arithmetic conventions of the unpinned OpenCV routines in the ORACLE only
    (tools/convention_report.py); mask 0 is the restatement the GPU path is held to, and setting it back restores it."""
    L = ob.lib()
    s = host.Synth(1)
    o = ob.Oracle(s.scene)
    base = o.match(s.seeds, 0, s.n_seeds, 2)
    try:
        L.orc_set_conventions(4 | 8)  # hypot + reversed rotation pairs in the DLT's Jacobi SVD
        alt = o.match(s.seeds, 0, s.n_seeds, 2)
    finally:
        L.orc_set_conventions(0)
    again = o.match(s.seeds, 0, s.n_seeds, 2)
    assert compare_edgepoints(base, again)["bitexact_X"]
    rep = compare_by_chain(base, alt)
    assert rep["chains_in_both"] > 10 and rep["share_chains_identical"] > 0.3
    assert rep["points_X_bit_equal"] < rep["points_compared"]          # the start of Gauss-Newton really moved ...
    assert rep["share_points_within_tol"] > 0.99                        # ... and the solutions barely


def test_a_removed_expand_switch_on_the_command_line_stops_the_build():
    """The decided A/B switches of the expand kernel are gone (DESIGN_LOG.md): a variant build that still passes one
    must fail in the preprocessor instead of building the product and timing it against itself. Preprocessing only."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    cmd = ([hipcc] + [f for f in build.HIP_FLAGS if f != "-shared"]
           + ["-I", build.INC_DIR, "-I", build.CSRC_DIR, "-I", build.HOST_DIR,
              "-E", os.path.join(build.CSRC_DIR, "eg3d_k3_chains.hip"), "-o", os.devnull])
    r = subprocess.run(cmd + ["-DEG3D_SIDE_WALK_BATCH=1"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0
    assert "A/B switches" in r.stderr and "EG3D_SIDE_WALK_BATCH" in r.stderr and "DESIGN_LOG.md" in r.stderr, r.stderr
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
