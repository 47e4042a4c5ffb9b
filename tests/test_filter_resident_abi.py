"""The C ABI of the device-resident filter stage, without a GPU: both product libraries export the three entry points,
the ctypes mirror of eg3d_filter_stats has the size and the member offsets a C compiler gives the header's struct, and
Context carries the bindings."""
import ctypes as C
import os
import subprocess

import pytest

import forms
from edgegraph3d_amd import _cdefs as D
from edgegraph3d_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eg3d_gn_filter_device", "eg3d_compact_device", "eg3d_filter_resident")


@pytest.mark.parametrize("rows", list(forms.FORMS), ids=[forms.IDS[r] for r in forms.FORMS])
def test_both_libraries_export_the_entry_points(rows):
    path = forms.lib_path(rows)
    if not os.path.exists(path):
        from edgegraph3d_amd import build
        (build.build_hip if rows == 3 else build.build_hip_dlt4x4)()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in SYMBOLS:
        assert name in exported, (name, path)
        assert name in api.EXPORTED_SYMBOLS


def test_filter_stats_mirror_matches_the_header(tmp_path):
    fields = [f[0] for f in D.FilterStats._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eg3d.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(eg3d_filter_stats));\n'
                   + "".join('  printf("%%zu\\n", offsetof(eg3d_filter_stats, %s));\n' % f for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == C.sizeof(D.FilterStats)
    assert nums[1:] == [getattr(D.FilterStats, f).offset for f in fields]
    assert fields[0] == "struct_size" and D.FilterStats.struct_size.offset == 0 and D.FilterStats.struct_size.size == 4


def test_context_has_the_bindings():
    for name in ("gn_filter_device", "compact_device", "filter_resident", "device_alloc", "upload"):
        assert callable(getattr(api.Context, name)), name
