"""The child process of the rehash test (tests/test_gpu_replay_merge.py): EG3D_REPLAY_TABLE_BITS is read when a context is
created, so the parent sets it and runs this. The C2 window in five seed ranges, each matched and replayed on a clone and its
graph merged into the first context's accumulator, materialised after the last: python replay_merge_child.py <out.npz> writes
the final graph, the accumulated pairs and, per merge, the table's slots and the nodes of the shard's graph."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import replay_gpu_cases as rc  # noqa: E402
from edgegraph3d_amd import api, host  # noqa: E402

if __name__ == "__main__":
    s = host.Synth(2)
    ctx = api.Context(s.scene)
    clone = None
    try:
        ctx.upload_seeds(s.seeds)
        clone = ctx.clone()
        b, e, k = 1550, 1800, 5
        edges = [b + (e - b) * i // k for i in range(k + 1)]
        slots, nodes = [], []
        for i in range(k):
            d = clone.match_resident(edges[i], edges[i + 1], device_only=True)
            _, dv, st = clone.replay_device(to_host=False)
            g, _, sta = ctx.replay_merge(dv, d["n_points"], st["n_pairs"], reset=(i == 0), materialise=(i == k - 1))
            slots.append(sta["table_slots"])
            nodes.append(st["n_nodes"])
        out = {"slots": np.array(slots, np.uint64), "shard_nodes": np.array(nodes, np.uint64), "pairs": np.uint64(sta["n_pairs"])}
        for f in rc.FIELDS + rc.ARRAYS:
            out[f] = g[f]
        np.savez(sys.argv[1], **out)
    finally:
        if clone is not None:
            clone.close()
        ctx.close()
