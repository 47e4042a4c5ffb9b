"""-m gpu: examples/edge_matcher_refpoints --resident-dedup. All three stages (polyline matches of pipelines 1 and 2, the
reference points) matched device-only, each deduplicated on the device against the claims of the stages before it, only
the survivors copied: the JSON written must be the default path's, byte for byte, with and without --filter."""
import re
import subprocess

import pytest

import cbuild
import forms

pytestmark = pytest.mark.gpu


def test_resident_dedup_writes_the_same_json(eg3d_form, tmp_path):
    lib = forms.lib_path(eg3d_form)
    exe = cbuild.build_caller("examples/edge_matcher_refpoints.cpp", tmp_path, lib=lib)
    d = str(tmp_path)
    subprocess.check_call([exe, "--make-synthetic", "1", d])
    common = [d + "/input.json", d + "/plgs.bin"]
    stages = ["--all-pairs", "--sets1", d + "/sets1.txt", "--sets2", d + "/sets2.txt"]
    for name, extra in (("plain", []), ("filtered", ["--filter"])):
        outs = {}
        for mode, flag in (("host", []), ("resident", ["--resident-dedup"])):
            path = "%s/%s_%s.json" % (d, name, mode)
            r = subprocess.run([exe] + common + [path] + stages + extra + flag, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            outs[mode] = (open(path, "rb").read(), r.stdout)
        assert len(outs["host"][0]) > 1000
        assert outs["resident"][0] == outs["host"][0], name
        # the same counts on both paths; on the resident one every stage reports its device dedup, and each kept only a part
        kept = [re.search(r"kept (\d+) edge-points", o[1]).group(1) for o in outs.values()]
        assert kept[0] == kept[1] and int(kept[0]) > 0
        per_stage = re.findall(r"dedup on the device: (\d+) of (\d+) points kept", outs["resident"][1])
        assert len(per_stage) == 3 and "dedup on the device" not in outs["host"][1]
        assert sum(int(k) for k, _ in per_stage) == int(kept[0])
        assert all(0 < int(k) < int(n) for k, n in per_stage), per_stage
