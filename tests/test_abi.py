"""The whole C ABI against its Python description, without a GPU, driven by the registry of edgegraph3d_amd/_cabi.py: every
header of include/ has a row in _cabi.HEADERS; every function a header declares is held to its row in that header's table,
every struct to its ctypes mirror (_cdefs.MIRRORS) and to the frozen layouts of tests/golden/abi_layout.json (eg3d.h,
eg3d_host.h) and abi_layout_later.json (the later headers); and every built library is held to the tables HEADERS gives it,
as nm lists it and as api.lib() / host.lib() load it. A public struct is changed by editing its layout file on purpose; a
function is added by adding its row; a header by adding its table, its HEADERS row and its count below."""
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
GOLDEN_LATER = os.path.join(ROOT, "tests", "golden", "abi_layout_later.json")
HEADERS, FROZEN_HEADERS = _cabi.HEADERS, _cabi.FROZEN_HEADERS
LATER_HEADERS = [h for h in HEADERS if h not in FROZEN_HEADERS]
MIRRORS = {cname: mirror for per_header in D.MIRRORS.values() for cname, mirror in per_header.items()}
# functions per header: a table grows or shrinks only together with its figure here
COUNTS = {"eg3d.h": 36, "eg3d_host.h": 59, "eg3d_rccl.h": 10, "eg3d_accumulate.h": 2, "eg3d_host_accumulate.h": 5,
          "eg3d_dedup_phases.h": 5, "eg3d_host_dedup_phases.h": 4, "eg3d_rccl_claims.h": 2, "eg3d_replay_merge.h": 1,
          "eg3d_host_replay_merge.h": 1, "eg3d_sets_device.h": 6, "eg3d_triangulate.h": 2, "eg3d_host_triangulate.h": 1,
          "eg3d_colour.h": 4, "eg3d_host_colour.h": 5, "eg3d_transform.h": 2, "eg3d_host_transform.h": 10}
# the structs of the later headers: each carries its own size, first
LATER_STRUCTS = ("eg3d_device_polyline_sets", "eg3d_items_call", "eg3d_sets_device_stats", "eg3d_tri_stats",
                 "eg3d_colour_stats", "eg3d_transform_stats", "eg3d_similarity_stats")
STRUCT = re.compile(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
MEMBER = re.compile(r"(\w+)\s*(\[\d+\])?\s*$")


def tables(library):
    """The tables of one library ("eg3d", "host" or "rccl") in HEADERS' order."""
    return [table for owner, table in HEADERS.values() if owner == library]


def names(library):
    return {fn for table in tables(library) for fn in table}


def header_text(name):
    """A public header without its comments and preprocessor lines."""
    t = open(os.path.join(INC, name)).read()
    return re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/|//[^\n]*", " ", t, flags=re.S), flags=re.M)


def header_structs(headers=tuple(HEADERS)):
    """{struct name: [member names]} of the given headers (default: all of HEADERS), as the C text states them."""
    out = {}
    for h in headers:
        for body, name in STRUCT.findall(header_text(h)):
            decls = [d for d in (x.strip() for x in body.split(";")) if d]
            out[name] = [MEMBER.search(piece).group(1) for d in decls for piece in d.split(",")]
    return out


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def c_layout(tmp_path_factory):
    """{struct: {"size": sizeof, "fields": [[member, offsetof, sizeof], ...]}} as gcc lays the headers' structs out: one C99
    program over every header of HEADERS, every struct and every member they name, compiled and run once."""
    d = tmp_path_factory.mktemp("abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in HEADERS] + ["int main(void) {"]
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


def test_every_header_of_the_include_directory_has_its_row():
    assert set(HEADERS) == {f for f in os.listdir(INC) if f.endswith(".h")}
    assert list(HEADERS)[:3] == list(FROZEN_HEADERS) and len(HEADERS) == 17
    assert {owner for owner, _ in HEADERS.values()} == {"eg3d", "host", "rccl"}


def test_every_struct_of_the_headers_has_a_mirror():
    for h in HEADERS:   # (a header without a row in _cdefs.MIRRORS defines no struct)
        assert set(header_structs((h,))) == set(D.MIRRORS.get(h, {})), h
    assert set(D.MIRRORS) <= set(HEADERS)
    assert len(MIRRORS) == 32 and len(MIRRORS) == sum(len(per_header) for per_header in D.MIRRORS.values())
    assert set(header_structs(LATER_HEADERS)) == set(LATER_STRUCTS)


@pytest.mark.parametrize("cname", sorted(MIRRORS))
def test_mirror_has_the_layout_of_the_c_struct(c_layout, cname):
    mirror, got = MIRRORS[cname], c_layout[cname]
    assert got["size"] == C.sizeof(mirror)
    assert got["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_]
    # a struct that carries its own size carries it first: the library reads it before anything else
    if any(f[0] == "struct_size" for f in got["fields"]) or cname in LATER_STRUCTS:
        assert got["fields"][0] == ["struct_size", 0, 4]


def test_layout_is_the_frozen_one(c_layout):
    """tests/golden/abi_layout.json was written from the headers of the commit its first key names: a public struct changes
    only together with a deliberate edit of that file."""
    frozen = json.load(open(GOLDEN))
    assert list(frozen)[0] == "generated_from"
    assert len(frozen["structs"]) == 25
    assert {s: c_layout[s] for s in header_structs(FROZEN_HEADERS)} == frozen["structs"]


def test_layout_of_the_later_structs_is_the_frozen_one(c_layout):
    """The same for the structs of the later headers, in tests/golden/abi_layout_later.json."""
    frozen = json.load(open(GOLDEN_LATER))
    assert list(frozen)[0] == "generated_from"
    assert sorted(frozen["structs"]) == sorted(LATER_STRUCTS)
    assert {s: c_layout[s] for s in header_structs(LATER_HEADERS)} == frozen["structs"]


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


@pytest.mark.parametrize("header", list(HEADERS))
def test_table_states_what_the_header_declares(header):
    declared, table = header_functions(header), HEADERS[header][1]
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(table) == COUNTS[header]
    bad = []
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        got = (ctypes_kind(restype), [ctypes_kind(a) for a in argtypes])
        if got != (ret, params):
            bad.append((fn, "header", (ret, params), "table", got))
    assert not bad, bad
    assert not [n for n in table if "probe" in n or "internal" in n]


def test_every_name_has_one_table_and_the_frozen_headers_hold_nothing_of_the_later_ones():
    assert set(COUNTS) == set(HEADERS) and sum(COUNTS.values()) == 155
    every = [fn for _, table in HEADERS.values() for fn in table]
    assert len(every) == len(set(every)), sorted(fn for fn in set(every) if every.count(fn) > 1)
    frozen_text = header_text("eg3d.h") + header_text("eg3d_host.h")
    for name in [fn for h in LATER_HEADERS for fn in HEADERS[h][1]] + list(LATER_STRUCTS):
        assert name not in frozen_text, name


def test_frozen_tables_keep_their_named_functions_and_api_lists_its_own():
    assert api.EXPORTED_SYMBOLS == list(_cabi.EG3D)
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
    assert not names("eg3d") - syms, names("eg3d") - syms
    # no test hooks in the product library: the probes live in tests/probe/libeg3d_probe.so
    assert not [n for n in syms if "probe" in n or "internal" in n], syms
    # the host statements live in libeg3d_host.so alone; the grid builder is the one host function the product library shares
    host_only = names("host") - {"eg3d_host_build_grid"}
    assert not host_only & syms, host_only & syms


def test_host_and_gather_libraries_export_their_tables():
    assert not names("host") - exported(build.HOST_LIB)
    # the RCCL gather library: symbol table only — loading it would pull /opt/rocm's librccl into a process that may already
    # hold the torch wheel's ROCm runtime (distributed.gather_lib() is lazy for the same reason)
    assert not names("rccl") - exported(build.RCCL_LIB)


def test_loaded_library_carries_the_replay_entry_points():
    """The C-ABI library loads without a GPU, every function of the table declared on it."""
    assert hasattr(api.lib(), "eg3d_replay_device") and hasattr(api.lib(), "eg3d_free_graph3d")
    assert _cabi.EG3D["eg3d_replay_device"][1] == api.lib().eg3d_replay_device.argtypes


@pytest.mark.parametrize("library,loaded", [("eg3d", api.lib), ("host", host.lib)], ids=("eg3d", "host"))
def test_loaded_library_declares_every_function_as_its_table_states(library, loaded):
    """The C-ABI library and the host library load without a GPU, every function of every table declared on them."""
    for table in tables(library):
        for name, (restype, argtypes) in table.items():
            fn = getattr(loaded(), name)
            assert fn.argtypes == argtypes and fn.restype == restype, name
