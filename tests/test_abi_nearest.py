"""include/eg3d/nearest.hpp and include/eg3d/host_nearest.hpp against their Python description, without a GPU — what
tests/test_abi_edges.py does for the .h headers of the subdirectories, done for the registry of the .hpp ABI headers
(_cabi.HPP_HEADERS, _cdefs.MIRRORS_HPP) with test_abi's own parsers: every function a header declares against its row,
every struct against its ctypes mirror and gcc's layout with the headers compiled as C99, every library against its tables
as nm lists it and as api.lib() / host.lib() load it. Then the refusals that need no device, the old registries' sizes and
the build guard's bound on K18."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import forms
import test_abi as abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D

HPP = _cabi.HPP_HEADERS
HEADER, HOST_HEADER = "eg3d/nearest.hpp", "eg3d/host_nearest.hpp"
COUNTS = {HEADER: 5, HOST_HEADER: 5}
MIRRORS = {cname: mirror for per_header in D.MIRRORS_HPP.values() for cname, mirror in per_header.items()}
# the C++ headers of the interface layer (classes, not ABI): not part of any registry
CXX_HEADERS = {"eg3d_edge_matcher.hpp", "eg3d_point_cloud.hpp", "eg3d_refapi.hpp", "eg3d_refapi_glm.hpp", "eg3d_transform_coordinate_system.hpp"}


def test_the_registry_names_the_hpp_abi_headers():
    found = set()
    for base, _, files in os.walk(abi.INC):
        rel = os.path.relpath(base, abi.INC)
        found |= {os.path.join(rel, f).replace(os.sep, "/") for f in files if f.endswith(".hpp") and rel != "."}
    assert found == set(HPP) == {HEADER, HOST_HEADER}
    assert {f for f in os.listdir(abi.INC) if f.endswith(".hpp")} == CXX_HEADERS      # (the top level holds no .hpp ABI header)
    assert HPP[HEADER][0] == "eg3d" and HPP[HOST_HEADER][0] == "host"
    # ... and stays out of the registries the older tests pin, which keep their sizes
    assert len(_cabi.HEADERS) == 17 and set(_cabi.EXT_HEADERS) == {"eg3d/edges.h", "eg3d/host_edges.h"}
    older = [fn for reg in (_cabi.HEADERS, _cabi.EXT_HEADERS) for _, table in reg.values() for fn in table]
    for _, table in HPP.values():
        assert not set(table) & set(older) and not set(table) & set(api.EXPORTED_SYMBOLS)
    assert set(D.MIRRORS_HPP) <= set(HPP)
    assert not set(MIRRORS) & {c for reg in (D.MIRRORS, D.MIRRORS_EXT) for per in reg.values() for c in per}
    frozen_text = abi.header_text("eg3d.h") + abi.header_text("eg3d_host.h")
    for name in [fn for _, table in HPP.values() for fn in table] + list(MIRRORS) + ["eg3d_cloud_index"]:
        assert name not in frozen_text, name
    for h in HPP:
        assert "Why .hpp" in open(os.path.join(abi.INC, h)).read(), h


@pytest.mark.parametrize("header", list(HPP))
def test_table_states_what_the_header_declares(header):
    declared, table = abi.header_functions(header), HPP[header][1]
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(table) == COUNTS[header]
    bad = []
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        got = (abi.ctypes_kind(restype), [abi.ctypes_kind(a) for a in argtypes])
        if got != (ret, params):
            bad.append((fn, "header", (ret, params), "table", got))
    assert not bad, bad
    assert not [n for n in table if "probe" in n or "internal" in n]


def test_every_struct_of_the_headers_has_a_mirror():
    for h in HPP:
        assert set(abi.header_structs((h,))) == set(D.MIRRORS_HPP.get(h, {})), h
    assert set(MIRRORS) == {"eg3d_cloud_index_stats", "eg3d_nearest_stats"}
    st = abi.header_structs((HOST_HEADER,))["eg3d_nearest_stats"]
    for f in ("n_thresholds", "thresholds", "n_queries", "n_dropped", "n_nonfinite", "n_within", "n_below", "sum_q32", "min_d2", "max_d2",
              "median_d2", "ms_kernel", "ms_copy"):
        assert f in st, f
    ix = abi.header_structs((HOST_HEADER,))["eg3d_cloud_index_stats"]
    for f in ("n_points", "n_dropped", "n_nonfinite", "n_indexed", "n_cells", "max_cell_points", "origin", "cell", "dims"):
        assert f in ix, f


@pytest.fixture(scope="module")
def hpp_layout(tmp_path_factory):
    """{struct: {"size", "fields"}} as gcc lays out the structs of the two headers, compiled as C99 with -Wall -Werror."""
    d = tmp_path_factory.mktemp("abi_nearest")
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in HPP] + ["int main(void) {"]
    for s, members in abi.header_structs(tuple(HPP)).items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (d / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(d / "layout")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", abi.INC, str(d / "layout.c"), "-o", exe])
    for h in HPP:   # each header alone, as C
        subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", os.path.join(abi.INC, h)])
    out = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            out[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            out[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    return out


@pytest.mark.parametrize("cname", sorted(MIRRORS))
def test_mirror_has_the_layout_of_the_c_struct(hpp_layout, cname):
    mirror, got = MIRRORS[cname], hpp_layout[cname]
    assert got["size"] == C.sizeof(mirror)
    assert got["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_]
    assert got["fields"][0] == ["struct_size", 0, 4]
    assert got["size"] % 8 == 0 and not [f for f in got["fields"] if f[2] == 8 and f[1] % 8]    # no padding surprises


def _names(library):
    return {fn for owner, table in HPP.values() if owner == library for fn in table}


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = abi.exported(path)
    assert not _names("eg3d") - syms, _names("eg3d") - syms
    assert not _names("host") & syms        # the host statement lives in libeg3d_host.so alone
    assert not [n for n in syms if "k18" in n.lower() and "eg3d" not in n]   # (kernels and launches stay in namespace eg3d)


def test_host_library_exports_the_table_and_not_the_device_one():
    syms = abi.exported(build.HOST_LIB)
    assert not _names("host") - syms and not _names("eg3d") & syms


@pytest.mark.parametrize("library,loaded", [("eg3d", api.lib), ("host", host.lib)], ids=("eg3d", "host"))
def test_loaded_library_declares_every_function_as_its_table_states(library, loaded):
    for owner, table in HPP.values():
        if owner != library:
            continue
        for name, (restype, argtypes) in table.items():
            fn = getattr(loaded(), name)
            assert fn.argtypes == argtypes and fn.restype == restype, name
    for m in ("cloud_index", "nearest_device", "nearest_points", "compare_clouds"):
        assert callable(getattr(api.Context, m)), m
    for m in ("close", "__enter__", "__exit__"):
        assert callable(getattr(api.CloudIndex, m)), m
    for f in ("cloud_nearest", "compare_clouds", "read_ply_points", "cloud_index_stats"):
        assert callable(getattr(host, f)), f


def test_the_headers_state_the_rules():
    text = open(os.path.join(abi.INC, HOST_HEADER)).read()
    for phrase in ("d2 = (dx * dx + dy * dy) + dz * dz", "d2 < md2", "0x7f800000", "0xffffffff", "2^21", "sum_q32", "(n_within - 1) / 2",
                   "max_dist > cell", "binary_little_endian"):
        assert phrase in text, phrase
    dev = open(os.path.join(abi.INC, HEADER)).read()
    for phrase in ("before or after its context is destroyed", "EG3D_NEAREST_ERR_FOREIGN", "EG3D_K18_GROUP"):
        assert phrase in dev, phrase
    core = open(os.path.join(build.CSRC_DIR, "eg3d_nearest_core.h")).read()
    for phrase in ("BOUNDS", "EG3D_HD", "monotone", "strict"):
        assert phrase in core, phrase
    for f in ("eg3d_k18_nearest.hip", "eg3d_api_nearest.hip"):
        assert '#include "eg3d_nearest_core.h"' in open(os.path.join(build.CSRC_DIR, f)).read() + open(os.path.join(build.CSRC_DIR, "eg3d_k18_nearest.h")).read()
    assert '#include "eg3d_nearest_core.h"' in open(os.path.join(build.HOST_DIR, "nearest.cpp")).read()
    assert "COMPARE" in open(os.path.join(build.ROOT, "DESIGN.md")).read()


def test_null_arguments_and_a_short_struct_are_refused_without_a_device():
    L = api.lib()
    h = C.c_void_p(0x77)
    st = D.CloudIndexStats(struct_size=C.sizeof(D.CloudIndexStats))
    assert L.eg3d_cloud_index_build(None, None, 0, None, 1.0, C.byref(h), C.byref(st)) == -1 and h.value == 0x77
    assert L.eg3d_cloud_index_build_device(None, None, None, 1.0, C.byref(h), None) == -1
    tiny = D.CloudIndexStats(struct_size=4)
    assert L.eg3d_cloud_index_build(None, None, 0, None, 1.0, C.byref(h), C.byref(tiny)) == -1
    assert b"struct_size" in L.eg3d_last_error()
    ns = D.nearest_stats_new()
    assert L.eg3d_cloud_nearest_device(None, None, None, None, 0.5, None, None, C.byref(ns)) == -1
    assert L.eg3d_cloud_nearest_points(None, None, 0, None, None, 0.5, None, None, None) == -1
    small = D.NearestStats(struct_size=16)
    assert L.eg3d_cloud_nearest_points(None, None, 0, None, None, 0.5, None, None, C.byref(small)) == -1
    assert b"struct_size" in L.eg3d_last_error()
    L.eg3d_cloud_index_free(None)
    host.lib().eg3d_host_free_points(None)
    assert host.lib().eg3d_host_read_ply_points(None, None, None) == -1


def _source_kernels():
    text = open(os.path.join(build.CSRC_DIR, "eg3d_k18_nearest.hip")).read()
    return {"eg3d::" + m for m in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(k18_\w+)\s*\(", text)}


def test_the_build_guard_holds_k18():
    """No spilled register, no scratch and no LDS in K18, in the bound and in the recorded figures of both libraries; the
    recorded k18_ kernels are the ones the source defines; what was recorded for K15 - K17 is still there."""
    b = build.RESOURCE_BOUNDS["k18_"]
    assert b == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 0}
    want = _source_kernels()
    assert want == {"eg3d::k18_" + k for k in ("init", "minmax", "keys", "gather", "cells", "max_cell", "query", "median")}
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k18 = {n: r for n, r in rec.items() if "k18_" in n}
        assert {re.sub(r"^void ", "", n).split("(")[0].split("<")[0] for n in k18} == want, sorted(k18)
        assert len([n for n in k18 if "k18_query<" in n]) == 3          # 1, 8 and 64 lanes per query
        for n, r in k18.items():
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, n
            assert r["group_segment_fixed_size"] == 0, n
        assert len([n for n in rec if "k17_" in n]) == 12 and len([n for n in rec if "k16_" in n]) == 1 and len([n for n in rec if "k15_" in n]) == 2
