#!/bin/bash
# eg3d_host_is_matched (host/matched.cpp over csrc/eg3d_matched_core.h) under AddressSanitizer + UBSan, as a stand-alone
# program: tools/matched_asan_main.cpp with its own main, the host sources it calls compiled into it. No GPU, nothing loaded
# into Python. The intervals of its second half are the oracle's replay of the oracle's pipeline 3 on synthetic config 0, the
# points every 20 px sample and every epipolar hit of the curve sets, the expected answers the restatement's
# (tests/matched_ref.py); they are written to a temporary text file first.
set -e
cd "$(dirname "$0")/.."
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT
python - "$tmp/synth0.txt" <<'PY'
import sys
sys.path[:0] = [".", "tests"]
import numpy as np
import matched_ref as R
from edgegraph3d_amd import build, host
build.build_host(), build.build_oracle()
from oracle import binding as ob
s = host.Synth(0)
orc = ob.Oracle(s.scene)
g = orc.replay_matches(orc.match(s.seeds, 0, s.n_seeds, 1))
S = R.Scene(s.scene_np(), ob.lib())
a = R.stage_a(S, *s.polyline_sets(), None)
V, nt = S.V, a["n_tasks"]
hv = np.repeat(np.tile(np.arange(V), nt), np.diff(a["list_off"].astype(np.int64)))
pts = list(zip(a["task_view"], a["task_pl"], a["task_seg"], a["task_xy"])) + list(zip(hv, a["hit_pl"], a["hit_seg"], a["hit_xy"]))
rows = R.rows_of(g)
bits = lambda xy: "%x %x" % tuple(int(t) for t in np.asarray(xy, np.float32).view(np.uint32))
with open(sys.argv[1], "w") as f:
    ni = len(g["iv_start_seg"])
    f.write("%d %d %d\n" % (len(g["iv_off"]) - 1, ni, len(pts)))
    f.write(" ".join(str(int(o)) for o in g["iv_off"]) + "\n")
    for i in range(ni):
        f.write("%d %s %d %s\n" % (g["iv_start_seg"][i], bits(g["iv_start_xy"][i]), g["iv_end_seg"][i], bits(g["iv_end_xy"][i])))
    for v, p, sg, xy in pts:
        gid = S.gid(int(v), int(p))
        f.write("%d %d %d %s %d\n" % (v, p, sg, bits(xy), R.is_matched(rows.get(gid), S.vertices(gid), int(sg), (xy[0], xy[1]))))
PY
g++ -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-omit-frame-pointer -I include -I edgegraph3d_amd/csrc -o $tmp/matched_asan tools/matched_asan_main.cpp \
    edgegraph3d_amd/host/matched.cpp edgegraph3d_amd/host/scenegen.cpp
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $tmp/matched_asan $tmp/synth0.txt
