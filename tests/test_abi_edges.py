"""include/eg3d/edges.h and include/eg3d/host_edges.h against their Python description, without a GPU — what tests/test_abi.py
does for the headers at the top of include/, done here for the registry of the headers in subdirectories
(_cabi.EXT_HEADERS, _cdefs.MIRRORS_EXT) with test_abi's own parsers: every function a header declares against its row, every
struct against its ctypes mirror and gcc's layout, every library against its tables as nm lists it and as api.lib() /
host.lib() load it. Then what the two headers promise beyond signatures, and the build guard's bound on K17."""
import ctypes as C
import json
import os
import subprocess

import pytest

import forms
import test_abi as abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D

EXT = _cabi.EXT_HEADERS
HEADER, HOST_HEADER = "eg3d/edges.h", "eg3d/host_edges.h"
COUNTS = {HEADER: 3, HOST_HEADER: 3}
MIRRORS = {cname: mirror for per_header in D.MIRRORS_EXT.values() for cname, mirror in per_header.items()}


def test_the_registry_names_the_headers_of_the_subdirectories():
    found = set()
    for base, _, files in os.walk(abi.INC):
        rel = os.path.relpath(base, abi.INC)
        found |= {os.path.join(rel, f).replace(os.sep, "/") for f in files if f.endswith(".h") and rel != "."}
    assert found == set(EXT) == {HEADER, HOST_HEADER}
    assert EXT[HEADER][0] == "eg3d" and EXT[HOST_HEADER][0] == "host"
    # ... and stays out of the registry test_abi.py pins
    assert not set(EXT) & set(_cabi.HEADERS) and len(_cabi.HEADERS) == 17
    every = [fn for _, table in _cabi.HEADERS.values() for fn in table]
    for _, table in EXT.values():
        assert not set(table) & set(every) and not set(table) & set(api.EXPORTED_SYMBOLS)
    assert set(D.MIRRORS_EXT) <= set(EXT) and not set(MIRRORS) & {c for per in D.MIRRORS.values() for c in per}
    frozen_text = abi.header_text("eg3d.h") + abi.header_text("eg3d_host.h")
    for name in [fn for _, table in EXT.values() for fn in table] + list(MIRRORS):
        assert name not in frozen_text, name


@pytest.mark.parametrize("header", list(EXT))
def test_table_states_what_the_header_declares(header):
    declared, table = abi.header_functions(header), EXT[header][1]
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
    for h in EXT:
        assert set(abi.header_structs((h,))) == set(D.MIRRORS_EXT.get(h, {})), h
    assert set(MIRRORS) == {"eg3d_device_edge_chains", "eg3d_edge_chain_set", "eg3d_edges_stats"}
    st = abi.header_structs((HOST_HEADER,))["eg3d_edges_stats"]
    for f in ("n_chains", "n_rings", "n_loops_dropped", "n_vertices_in", "n_vertices_kept", "longest_chain", "ms_trace",
              "ms_simplify", "ms_copy"):
        assert f in st, f
    assert abi.header_structs((HEADER,))["eg3d_device_edge_chains"] == abi.header_structs((HOST_HEADER,))["eg3d_edge_chain_set"]


@pytest.fixture(scope="module")
def ext_layout(tmp_path_factory):
    """{struct: {"size", "fields"}} as gcc lays out the structs of the two headers (C99: the headers are C)."""
    d = tmp_path_factory.mktemp("abi_edges")
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in EXT] + ["int main(void) {"]
    for s, members in abi.header_structs(tuple(EXT)).items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (d / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(d / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", abi.INC, str(d / "layout.c"), "-o", exe])
    out = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            out[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            out[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    return out


@pytest.mark.parametrize("cname", sorted(MIRRORS))
def test_mirror_has_the_layout_of_the_c_struct(ext_layout, cname):
    mirror, got = MIRRORS[cname], ext_layout[cname]
    assert got["size"] == C.sizeof(mirror)
    assert got["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_]
    if cname == "eg3d_edges_stats":
        assert got["fields"][0] == ["struct_size", 0, 4]


def _names(library):
    return {fn for owner, table in EXT.values() if owner == library for fn in table}


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = abi.exported(path)
    assert not _names("eg3d") - syms, _names("eg3d") - syms
    assert not _names("host") & syms        # the host statement lives in libeg3d_host.so alone
    assert not [n for n in syms if "k17" in n.lower() and "eg3d" not in n]   # (kernels and launches stay in namespace eg3d)


def test_host_library_exports_the_table_and_not_the_device_one():
    syms = abi.exported(build.HOST_LIB)
    assert not _names("host") - syms and not _names("eg3d") & syms


@pytest.mark.parametrize("library,loaded", [("eg3d", api.lib), ("host", host.lib)], ids=("eg3d", "host"))
def test_loaded_library_declares_every_function_as_its_table_states(library, loaded):
    for owner, table in EXT.values():
        if owner != library:
            continue
        for name, (restype, argtypes) in table.items():
            fn = getattr(loaded(), name)
            assert fn.argtypes == argtypes and fn.restype == restype, name
    for m in ("edge_chains_device", "edge_chains"):
        assert callable(getattr(api.Context, m)), m
    for f in ("edge_chains", "write_ply_edges"):
        assert callable(getattr(host, f)), f


def test_the_headers_state_the_rules_and_the_deviation():
    text = open(os.path.join(abi.INC, HOST_HEADER)).read()
    for phrase in ("simplify_polyline", "update_length", "get_segments_list", "E1", "smallest polyline id", "2 * n_polylines - n_loops",
                   "finite and >= 0"):
        assert phrase in text, phrase
    core = open(os.path.join(build.CSRC_DIR, "eg3d_edges_core.h")).read()
    for phrase in ("DEVIATION (E1)", "BOUNDS", "PINNED", "EG3D_HD"):
        assert phrase in core, phrase
    assert "EDGES" in open(os.path.join(build.ROOT, "DESIGN.md")).read()


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    st = D.EdgesStats(struct_size=C.sizeof(D.EdgesStats))
    assert L.eg3d_edge_chains_device(None, None, 0.01, 1, None, None, C.byref(st)) == -1
    assert L.eg3d_edge_chains(None, None, 0.01, 1, None, None, None) == -1
    tiny = D.EdgesStats(struct_size=4)
    assert L.eg3d_edge_chains(None, None, 0.01, 1, None, None, C.byref(tiny)) == -1
    assert b"struct_size" in L.eg3d_last_error()
    L.eg3d_free_edge_chains(None)
    empty = D.EdgeChains()
    L.eg3d_free_edge_chains(C.byref(empty))
    host.lib().eg3d_host_free_edge_chains(None)
    assert host.lib().eg3d_host_write_ply_edges(None, C.byref(empty), None) == -1


def test_the_build_guard_holds_k17():
    """No spilled register and no scratch in K17, LDS only in the simplification (the staged chain), in the bound and in the
    recorded figures of both libraries; every kernel the parent recorded is still recorded."""
    b = build.RESOURCE_BOUNDS["k17_"]
    assert b == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 12288}
    want = {"eg3d::k17_" + k for k in ("check_polylines", "check_offsets", "check_rows", "successors", "jump", "cut_rings", "heads",
                                       "chain_sizes", "fill", "simplify", "compact", "length")}
    for lib in ("libeg3d", "libeg3d_dlt4x4"):
        rec = json.load(open(os.path.join(build.ROOT, "profiles", "kernel_resources_%s.json" % lib)))
        k17 = {n: r for n, r in rec.items() if "k17_" in n}
        assert {n.split("(")[0] for n in k17} == want, sorted(k17)
        for n, r in k17.items():
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, n
            assert r["group_segment_fixed_size"] == (12288 if "k17_simplify" in n else 0), n
        assert len([n for n in rec if "k16_" in n]) == 1 and len([n for n in rec if "k15_" in n]) == 2
