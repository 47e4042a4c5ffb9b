"""What tests/test_abi.py does for the frozen headers, for include/eg3d_sets_device.h: every function it declares against
its row in _cabi.EG3D_SETS_DEVICE, its three structs against their ctypes mirrors as gcc lays them out, and the table
against the symbols both product libraries export. No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, build
from edgegraph3d_amd import _cdefs as D

HEADER = "eg3d_sets_device.h"
MIRRORS = {"eg3d_device_polyline_sets": D.DevicePolylineSets, "eg3d_items_call": D.ItemsCall,
           "eg3d_sets_device_stats": D.SetsDeviceStats}
FROZEN = (_cabi.EG3D, _cabi.EG3D_HOST, _cabi.EG3D_RCCL)
OTHERS = (_cabi.EG3D_ACCUMULATE, _cabi.EG3D_HOST_ACCUMULATE, _cabi.EG3D_DEDUP_PHASES, _cabi.EG3D_HOST_DEDUP_PHASES,
          _cabi.EG3D_RCCL_CLAIMS, _cabi.EG3D_REPLAY_MERGE, _cabi.EG3D_HOST_REPLAY_MERGE)


def _structs():
    out = {}
    for body, name in test_abi.STRUCT.findall(test_abi.header_text(HEADER)):
        decls = [d for d in (x.strip() for x in body.split(";")) if d]
        out[name] = [re.search(r"(\w+)\s*$", piece).group(1) for d in decls for piece in d.split(",")]
    return out


def test_table_states_what_the_header_declares():
    declared, table = test_abi.header_functions(HEADER), _cabi.EG3D_SETS_DEVICE
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(table) == 6
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        assert (test_abi.ctypes_kind(restype), [test_abi.ctypes_kind(a) for a in argtypes]) == (ret, params), fn
    assert not [n for n in table if "probe" in n or "internal" in n]
    assert set(table) >= {"eg3d_upload_polyline_sets", "eg3d_polyline_matches_device", "eg3d_sets_from_communities_device",
                          "eg3d_polyline_item_samples", "eg3d_match_polyline_items"}


def test_the_frozen_tables_are_untouched_and_the_new_one_disjoint():
    assert [len(t) for t in FROZEN] == [36, 59, 10]
    names = [n for t in FROZEN + OTHERS + (_cabi.EG3D_SETS_DEVICE,) for n in t]
    assert len(names) == len(set(names))
    assert sorted(api.SETS_DEVICE_SYMBOLS) == sorted(_cabi.EG3D_SETS_DEVICE)
    assert not set(api.SETS_DEVICE_SYMBOLS) & set(api.EXPORTED_SYMBOLS)
    # the frozen headers define none of the new structs
    frozen_text = test_abi.header_text("eg3d.h") + test_abi.header_text("eg3d_host.h")
    for name in MIRRORS:
        assert name not in frozen_text, name


def test_mirrors_have_the_layout_gcc_gives_the_structs(tmp_path):
    structs = _structs()
    assert set(structs) == set(MIRRORS), set(structs) ^ set(MIRRORS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {"]
    for s, members in structs.items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", test_abi.INC, str(tmp_path / "layout.c"), "-o", exe])
    got = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            got[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            got[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    for cname, mirror in MIRRORS.items():
        assert got[cname]["size"] == C.sizeof(mirror), cname
        assert got[cname]["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_], cname
        assert got[cname]["fields"][0] == ["struct_size", 0, 4], cname   # new structs carry their size first


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = test_abi.exported(path)
    assert not set(_cabi.EG3D_SETS_DEVICE) - syms, set(_cabi.EG3D_SETS_DEVICE) - syms


def test_loaded_library_carries_the_entry_points():
    for name in _cabi.EG3D_SETS_DEVICE:   # (the C-ABI library loads without a GPU)
        assert hasattr(api.lib(), name), name
        assert _cabi.EG3D_SETS_DEVICE[name][1] == getattr(api.lib(), name).argtypes
    for m in ("upload_polyline_sets", "polyline_matches_device", "sets_from_communities_device", "polyline_item_samples",
              "match_polyline_items", "fetch_polyline_sets"):
        assert callable(getattr(api.Context, m)), m


def test_the_build_guard_holds_k13_to_no_spills_no_scratch_no_lds():
    b = build.RESOURCE_BOUNDS["k13_"]
    assert b == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 0}
