"""The whole C ABI against its Python description, without a GPU: every struct of include/eg3d.h and include/eg3d_host.h
against its ctypes mirror (edgegraph3d_amd/_cdefs.py) and against the frozen layout of tests/golden/abi_layout.json, every
function the three public headers declare against its row in edgegraph3d_amd/_cabi.py, and the symbols the built libraries
export. A public struct is changed by editing abi_layout.json on purpose; a function is added by adding its row."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import forms
from edgegraph3d_amd import _cabi
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api, build, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_layout.json")
TABLES = {"eg3d.h": _cabi.EG3D, "eg3d_host.h": _cabi.EG3D_HOST, "eg3d_rccl.h": _cabi.EG3D_RCCL}
MIRRORS = {
    "eg3d_scene": D.Scene, "eg3d_seeds": D.Seeds, "eg3d_edgepoints": D.EdgePoints, "eg3d_candidates": D.Candidates,
    "eg3d_stage_times": D.StageTimes, "eg3d_polyline_sets": D.PolylineSets, "eg3d_matched_intervals": D.MatchedIntervals,
    "eg3d_set_candidates": D.SetCandidates, "eg3d_device_edgepoints": D.DeviceEdgePoints, "eg3d_filter_stats": D.FilterStats,
    "eg3d_dedup_stats": D.DedupStats, "eg3d_device_graph3d": D.DeviceGraph3D, "eg3d_replay_stats": D.ReplayStats,
    "eg3d_polyline_matches": D.PolylineMatches, "eg3d_polymatch_stats": D.PolymatchStats, "eg3d_simgraph": D.Simgraph,
    "eg3d_simgraph_stats": D.SimgraphStats, "eg3d_louvain_params": D.LouvainParams, "eg3d_communities": D.Communities,
    "eg3d_louvain_stats": D.LouvainStats, "eg3d_fund_params": D.FundParams, "eg3d_fund_stats": D.FundStats,
    "eg3d_synth_config": D.SynthConfig, "eg3d_plg_view": D.PlgView, "eg3d_graph3d": D.Graph3D,
}
STRUCT = re.compile(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def header_text(name):
    """A public header without its comments and preprocessor lines."""
    t = open(os.path.join(INC, name)).read()
    return re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/|//[^\n]*", " ", t, flags=re.S), flags=re.M)


def header_structs():
    """{struct name: [member names]} of the two headers that define structs, as the C text states them."""
    out = {}
    for h in ("eg3d.h", "eg3d_host.h"):
        for body, name in STRUCT.findall(header_text(h)):
            decls = [d for d in (x.strip() for x in body.split(";")) if d]
            out[name] = [re.search(r"(\w+)\s*$", piece).group(1) for d in decls for piece in d.split(",")]
    return out


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def c_layout(tmp_path_factory):
    """{struct: {"size": sizeof, "fields": [[member, offsetof, sizeof], ...]}} as gcc lays the headers' structs out: one C99
    program over every struct and every member the headers name, compiled and run once."""
    d = tmp_path_factory.mktemp("abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d.h"', '#include "eg3d_host.h"', "int main(void) {"]
    for s, members in header_structs().items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (d / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(d / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, str(d / "layout.c"), "-o", exe])
    out = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            out[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            out[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    return out


def test_every_struct_of_the_headers_has_a_mirror():
    assert set(header_structs()) == set(MIRRORS), set(header_structs()) ^ set(MIRRORS)
    assert len(MIRRORS) == 25


@pytest.mark.parametrize("cname", sorted(MIRRORS))
def test_mirror_has_the_layout_of_the_c_struct(c_layout, cname):
    mirror, got = MIRRORS[cname], c_layout[cname]
    assert got["size"] == C.sizeof(mirror)
    assert got["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_]
    # a struct that carries its own size carries it first: the library reads it before anything else
    if any(f[0] == "struct_size" for f in got["fields"]):
        assert got["fields"][0] == ["struct_size", 0, 4]


def test_layout_is_the_frozen_one(c_layout):
    """tests/golden/abi_layout.json was written from the headers of the commit its first key names: a public struct changes
    only together with a deliberate edit of that file."""
    frozen = json.load(open(GOLDEN))
    assert list(frozen)[0] == "generated_from"
    assert len(frozen["structs"]) == 25
    assert c_layout == frozen["structs"]


def test_stats_structs_keep_their_named_fields():
    fields = [f[0] for f in D.DedupStats._fields_]
    for f in ("n_points_in", "n_dedup_kept", "n_gn_inliers", "n_kept", "n_obs_kept", "ms_dedup", "ms_filter", "ms_compact",
              "ms_copy"):
        assert f in fields
    assert fields[0] == "struct_size" and D.FilterStats._fields_[0][0] == "struct_size"


# ---- signatures --------------------------------------------------------------------------------------------------------------
C_KINDS = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "unsigned": "u32", "unsigned int": "u32", "int64_t": "i64",
           "uint64_t": "u64", "size_t": "u64", "unsigned long long": "u64", "float": "f32", "double": "f64", "void": "void"}
CTYPES_KINDS = {None: "void", C.c_void_p: "ptr", C.c_char_p: "ptr", C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64",
                C.c_uint64: "u64", C.c_float: "f32", C.c_double: "f64"}


def c_kind(text, named):
    """The kind of a C parameter (`named`: a parameter name may follow the type) or return type, from its text."""
    if "*" in text or "[" in text:
        return "ptr"
    words = [w for w in text.split() if w not in ("const", "struct")]
    for n in ((len(words), len(words) - 1) if named else (len(words),)):
        if n > 0 and " ".join(words[:n]) in C_KINDS:
            return C_KINDS[" ".join(words[:n])]
    raise AssertionError("cannot classify %r" % text)


def ctypes_kind(t):
    if t in CTYPES_KINDS:
        return CTYPES_KINDS[t]
    assert isinstance(t, type) and issubclass(t, C._Pointer), "cannot classify %r" % (t,)
    return "ptr"


def header_functions(name):
    """{function: (return kind, [parameter kinds])} of every `type name(params);` the header declares."""
    t = STRUCT.sub("", header_text(name)).replace('extern "C" {', "")
    t = re.sub(r"typedef[^;{]*;|\bstruct\s+\w+\s*;", "", t)   # (opaque handle types, forward declarations)
    decl = re.compile(r"([^;{}()]+?)\b(\w+)\s*\(([^()]*)\)\s*;", re.S)
    out = {}
    for ret, fn, params in decl.findall(t):
        assert fn not in out, fn
        out[fn] = (c_kind(ret, False), [c_kind(p, True) for p in ([] if params.strip() == "void" else params.split(","))])
    assert not decl.sub("", t).replace("}", "").strip(), "text of %s that is no declaration: %r" % (name, decl.sub("", t).strip())
    return out


@pytest.mark.parametrize("header", sorted(TABLES))
def test_table_states_what_the_header_declares(header):
    declared, table = header_functions(header), TABLES[header]
    assert set(declared) == set(table), set(declared) ^ set(table)
    bad = []
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        got = (ctypes_kind(restype), [ctypes_kind(a) for a in argtypes])
        if got != (ret, params):
            bad.append((fn, "header", (ret, params), "table", got))
    assert not bad, bad


def test_tables_cover_105_functions_and_api_lists_its_own():
    assert [len(TABLES[h]) for h in sorted(TABLES)] == [36, 59, 10]   # (ten: gather create / destroy / set_mode /
    #                                  set_chunk_bytes, allgather, concat, comm unique_id / init / query / destroy)
    assert len(_cabi.EG3D_HOST) > 24
    assert sorted(api.EXPORTED_SYMBOLS) == sorted(_cabi.EG3D)
    for name in ("eg3d_dedup_device", "eg3d_dedup_resident", "eg3d_gn_filter_device", "eg3d_compact_device",
                 "eg3d_filter_resident", "eg3d_detect_communities", "eg3d_free_communities", "eg3d_similarity_graph",
                 "eg3d_free_simgraph", "eg3d_estimate_fundamental"):
        assert name in api.EXPORTED_SYMBOLS, name


# ---- symbols -----------------------------------------------------------------------------------------------------------------
def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_the_table_and_no_test_hook(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = exported(path)
    assert not set(_cabi.EG3D) - syms, set(_cabi.EG3D) - syms
    # no test hooks in the product library: the probes live in tests/probe/libeg3d_probe.so
    assert not [n for n in syms if "probe" in n or "internal" in n], syms
    assert "eg3d_host_estimate_fundamental" not in syms  # (libeg3d.so does not carry the host statement)


def test_host_and_gather_libraries_export_their_tables():
    assert not set(_cabi.EG3D_HOST) - exported(build.HOST_LIB)
    # the RCCL gather library: symbol table only — loading it would pull /opt/rocm's librccl into a process that may already
    # hold the torch wheel's ROCm runtime (distributed.gather_lib() is lazy for the same reason)
    assert not set(_cabi.EG3D_RCCL) - exported(build.RCCL_LIB)
    for name in _cabi.EG3D_HOST:
        assert hasattr(host.lib(), name), name


def test_loaded_library_carries_the_replay_entry_points():
    """The C-ABI library loads without a GPU, every function of the table declared on it."""
    assert hasattr(api.lib(), "eg3d_replay_device") and hasattr(api.lib(), "eg3d_free_graph3d")
    assert _cabi.EG3D["eg3d_replay_device"][1] == api.lib().eg3d_replay_device.argtypes
