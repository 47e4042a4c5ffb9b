"""The one way the tests build a C or C++ caller of the libraries (examples/, tests/refapi/)."""
import os
import subprocess

from edgegraph3d_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edgegraph3d_amd")
DEFAULT_LIB = os.path.join(PKG, "libeg3d.so")   # for a caller that links the default library whichever form its test runs under


def build_caller(source, out_dir, *, lib=None, std="c++17", extra=()):
    """Compile `source` (relative to the repository root, or absolute) and link it against `lib` — a build of libeg3d, by
    path; default: the one api.lib() loads, so a test that runs per DLT form links the form it tests — libeg3d_host and the
    HIP runtime. `extra`: further compiler flags (-I, -D, -w). Returns the executable's path, inside `out_dir`."""
    lib = os.path.abspath(lib or api.lib_path())
    libdir = os.path.dirname(lib)
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(source))[0])
    subprocess.check_call(["g++" if "++" in std else "gcc", "-std=" + std, "-O1", "-pthread", "-I", os.path.join(ROOT, "include")]
                          + list(extra) + [os.path.join(ROOT, source), "-L", libdir, "-l:" + os.path.basename(lib), "-L", PKG,
                                           "-leg3d_host", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe
