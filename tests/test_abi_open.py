"""The open registry of ABI headers (_cabi.OPEN_HEADERS, _cdefs.MIRRORS_OPEN) against the headers it names, without a GPU.
Everything here is derived from the registry with test_abi's own parsers, so the next header is a new row and this file
stays as it is: every function a header declares against its row, every struct against its ctypes mirror and gcc's layout
with the headers compiled as C99, every library against its tables as nm lists it and as api.lib() / host.lib() load it.
The three older registries keep the sizes their own tests pin."""
import ctypes as C
import os
import subprocess

import pytest

import forms
import test_abi as abi
from edgegraph3d_amd import _cabi, api, build, host
from edgegraph3d_amd import _cdefs as D

OPEN = _cabi.OPEN_HEADERS
MIRRORS = {cname: mirror for per_header in D.MIRRORS_OPEN.values() for cname, mirror in per_header.items()}
OLDER = (_cabi.HEADERS, _cabi.EXT_HEADERS, _cabi.HPP_HEADERS)
OLDER_SUFFIXES = (".h", ".hpp")     # what the older tests collect under include/


def test_the_registry_names_every_header_the_older_registries_cannot():
    found = set()
    for base, _, files in os.walk(abi.INC):
        rel = os.path.relpath(base, abi.INC)
        found |= {(f if rel == "." else os.path.join(rel, f).replace(os.sep, "/")) for f in files if not f.endswith(OLDER_SUFFIXES)}
    assert found == set(OPEN)
    assert {owner for owner, _ in OPEN.values()} <= {"eg3d", "host", "rccl"}
    # the older registries at their pinned sizes, and no name in two places
    assert [len(r) for r in OLDER] == [17, 2, 2]
    older = [fn for reg in OLDER for _, table in reg.values() for fn in table]
    mine = [fn for _, table in OPEN.values() for fn in table]
    assert len(set(mine)) == len(mine) and not set(mine) & set(older) and not set(mine) & set(api.EXPORTED_SYMBOLS)
    assert set(D.MIRRORS_OPEN) <= set(OPEN)
    assert not set(MIRRORS) & {c for reg in (D.MIRRORS, D.MIRRORS_EXT, D.MIRRORS_HPP) for per in reg.values() for c in per}
    frozen_text = "".join(abi.header_text(h) for h in _cabi.FROZEN_HEADERS)
    for name in mine + list(MIRRORS):
        assert name not in frozen_text, name


@pytest.mark.parametrize("header", list(OPEN))
def test_table_states_what_the_header_declares(header):
    declared, table = abi.header_functions(header), OPEN[header][1]
    assert set(declared) == set(table), set(declared) ^ set(table)
    bad = []
    for fn, (ret, params) in declared.items():
        restype, argtypes = table[fn]
        got = (abi.ctypes_kind(restype), [abi.ctypes_kind(a) for a in argtypes])
        if got != (ret, params):
            bad.append((fn, "header", (ret, params), "table", got))
    assert not bad, bad
    assert not [n for n in table if "probe" in n or "internal" in n]


def test_every_struct_of_the_headers_has_a_mirror():
    for h in OPEN:
        assert set(abi.header_structs((h,))) == set(D.MIRRORS_OPEN.get(h, {})), h
    assert len(MIRRORS) == sum(len(per) for per in D.MIRRORS_OPEN.values())


@pytest.fixture(scope="module")
def open_layout(tmp_path_factory):
    """{struct: {"size", "fields"}} as gcc lays out the structs of the registry's headers, compiled as C99 with -Wall -Werror."""
    d = tmp_path_factory.mktemp("abi_open")
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in OPEN] + ["int main(void) {"]
    for s, members in abi.header_structs(tuple(OPEN)).items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, m, s, m, s, m) for m in members]
    (d / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(d / "layout")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", abi.INC, str(d / "layout.c"), "-o", exe])
    for h in OPEN:   # each header alone, as C
        subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", os.path.join(abi.INC, h)])
    out = {}
    for w in (l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        if w[0] == "S":
            out[w[1]] = {"size": int(w[2]), "fields": []}
        else:
            out[w[1]]["fields"].append([w[2], int(w[3]), int(w[4])])
    return out


@pytest.mark.parametrize("cname", sorted(MIRRORS))
def test_mirror_has_the_layout_of_the_c_struct(open_layout, cname):
    mirror, got = MIRRORS[cname], open_layout[cname]
    assert got["size"] == C.sizeof(mirror)
    assert got["fields"] == [[f[0], getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size] for f in mirror._fields_]
    if any(f[0] == "struct_size" for f in got["fields"]):
        assert got["fields"][0] == ["struct_size", 0, 4]
    assert got["size"] % 8 == 0 and not [f for f in got["fields"] if f[2] == 8 and f[1] % 8]    # no padding surprises


def _names(library):
    return {fn for owner, table in OPEN.values() if owner == library for fn in table}


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_product_library_exports_its_tables(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    syms = abi.exported(path)
    assert not _names("eg3d") - syms, _names("eg3d") - syms
    assert not _names("host") & syms        # the host statements live in libeg3d_host.so alone


def test_host_library_exports_its_tables_and_not_the_device_ones():
    syms = abi.exported(build.HOST_LIB)
    assert not _names("host") - syms and not _names("eg3d") & syms


@pytest.mark.parametrize("library,loaded", [("eg3d", api.lib), ("host", host.lib)], ids=("eg3d", "host"))
def test_loaded_library_declares_every_function_as_its_table_states(library, loaded):
    n = 0
    for owner, table in OPEN.values():
        if owner != library:
            continue
        for name, (restype, argtypes) in table.items():
            fn = getattr(loaded(), name)
            assert fn.argtypes == argtypes and fn.restype == restype, name
            n += 1
    assert n == len(_names(library)) > 0
