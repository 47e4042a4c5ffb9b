"""What tests/test_abi.py does for the frozen headers, for include/eg3d_colour.h and include/eg3d_host_colour.h: every
function they declare against its row in _cabi.EG3D_COLOUR / EG3D_HOST_COLOUR, eg3d_colour_stats against its ctypes mirror
as gcc lays it out, and the tables against the symbols both product libraries and the host library export. No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import forms
import test_abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D

HEADER, HOST_HEADER = "eg3d_colour.h", "eg3d_host_colour.h"
MIRRORS = {"eg3d_colour_stats": D.ColourStats}
FROZEN = (_cabi.EG3D, _cabi.EG3D_HOST, _cabi.EG3D_RCCL)
OTHERS = (_cabi.EG3D_ACCUMULATE, _cabi.EG3D_HOST_ACCUMULATE, _cabi.EG3D_DEDUP_PHASES, _cabi.EG3D_HOST_DEDUP_PHASES,
          _cabi.EG3D_RCCL_CLAIMS, _cabi.EG3D_REPLAY_MERGE, _cabi.EG3D_HOST_REPLAY_MERGE, _cabi.EG3D_SETS_DEVICE,
          _cabi.EG3D_TRIANGULATE, _cabi.EG3D_HOST_TRIANGULATE)
NEW = (_cabi.EG3D_COLOUR, _cabi.EG3D_HOST_COLOUR)


def _structs(header):
    out = {}
    for body, name in test_abi.STRUCT.findall(test_abi.header_text(header)):
        decls = [d for d in (x.strip() for x in body.split(";")) if d]
        out[name] = [re.search(r"(\w+)\s*$", piece).group(1) for d in decls for piece in d.split(",")]
    return out


@pytest.mark.parametrize("header,table,count", [(HEADER, _cabi.EG3D_COLOUR, 4), (HOST_HEADER, _cabi.EG3D_HOST_COLOUR, 5)],
                         ids=("device", "host"))
def test_table_states_what_the_header_declares(header, table, count):
    declared = test_abi.header_functions(header)
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(table) == count
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        assert (test_abi.ctypes_kind(restype), [test_abi.ctypes_kind(a) for a in argtypes]) == (ret, params), fn


def test_the_header_states_the_flag_and_the_deviations():
    text = open(os.path.join(test_abi.INC, HEADER)).read()   # (header_text drops the preprocessor lines)
    assert re.search(r"#define\s+EG3D_COLOUR_FLAG_EMPTY\s+1u\b", text)
    assert api.COLOUR_FLAG_EMPTY == 1
    for phrase in ("A clone (eg3d_clone) does NOT inherit them", "n == 0 is undefined behaviour in the reference", "JPEG is not read",
                   "the integer division"):
        assert phrase in text, phrase
    assert "JPEG is not read" in open(os.path.join(test_abi.INC, HOST_HEADER)).read()


def test_the_frozen_tables_are_untouched_and_the_new_ones_disjoint():
    assert [len(t) for t in FROZEN] == [36, 59, 10]
    names = [n for t in FROZEN + OTHERS + NEW for n in t]
    assert len(names) == len(set(names))
    assert sorted(api.COLOUR_SYMBOLS) == sorted(_cabi.EG3D_COLOUR)
    assert not set(api.COLOUR_SYMBOLS) & set(api.EXPORTED_SYMBOLS)
    assert api.EXPORTED_SYMBOLS == list(_cabi.EG3D)
    frozen_text = test_abi.header_text("eg3d.h") + test_abi.header_text("eg3d_host.h")
    for name in list(MIRRORS) + [n for t in NEW for n in t]:   # the frozen headers hold nothing of the new ones
        assert name not in frozen_text, name


def test_mirror_has_the_layout_gcc_gives_the_struct(tmp_path):
    structs = _structs(HEADER)
    assert set(structs) == set(MIRRORS), set(structs) ^ set(MIRRORS)
    assert not _structs(HOST_HEADER)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, '#include "%s"' % HOST_HEADER, "int main(void) {"]
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
    for f in ("n_points", "n_coloured", "n_empty", "n_obs_sampled", "ms_sample", "ms_mix", "ms_copy"):
        assert f in structs["eg3d_colour_stats"], f


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = test_abi.exported(path)
    assert not set(_cabi.EG3D_COLOUR) - syms, set(_cabi.EG3D_COLOUR) - syms
    assert not set(_cabi.EG3D_HOST_COLOUR) & syms   # (the product library does not carry the host statement)


def test_host_library_exports_the_table():
    syms = test_abi.exported(build.build_host())
    assert not set(_cabi.EG3D_HOST_COLOUR) - syms
    for name in _cabi.EG3D_HOST_COLOUR:
        assert _cabi.EG3D_HOST_COLOUR[name][1] == getattr(host.lib(), name).argtypes
    for f in ("colour_points", "write_ply", "read_png_rgb"):
        assert callable(getattr(host, f)), f


def test_loaded_library_carries_the_entry_points():
    for name in _cabi.EG3D_COLOUR:   # (the C-ABI library loads without a GPU)
        assert hasattr(api.lib(), name), name
        assert _cabi.EG3D_COLOUR[name][1] == getattr(api.lib(), name).argtypes
    for m in ("upload_images", "release_images", "colour_device", "colour_points"):
        assert callable(getattr(api.Context, m)), m


def test_the_build_guard_holds_k15():
    """No spilled register, no scratch and no LDS in either K15 kernel; the VGPR bounds are the build's counts."""
    b = build.RESOURCE_BOUNDS["k15_"]
    assert b["vgpr_spill_count"] == 0 and b["sgpr_spill_count"] == 0
    assert b["private_segment_fixed_size"] == 0 and b["group_segment_fixed_size"] == 0
    for k in ("k15_sample", "k15_mix"):
        assert 0 < build.RESOURCE_BOUNDS[k]["vgpr_count"] <= 64, k
    import json
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k15 = {n: r for n, r in rec.items() if "k15_" in n}
        assert len(k15) == 2, sorted(k15)
        for n, r in k15.items():
            key = "k15_sample" if "k15_sample" in n else "k15_mix"
            assert r["vgpr_count"] <= build.RESOURCE_BOUNDS[key]["vgpr_count"], n
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, n
