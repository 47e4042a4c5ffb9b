"""The child process of the table-growth test (tests/test_gpu_replay_accumulate.py): EG3D_REPLAY_TABLE_BITS is read when a
context is created, so the parent sets it and runs this. The C2 window in five match steps, each followed by an accumulate
without materialisation but the last: python replay_accumulate_child.py <out.npz> writes the final graph and, per step, the
table's slots and the accumulated pairs."""
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
    try:
        ctx.upload_seeds(s.seeds)
        b, e, k = 1550, 1800, 5
        edges = [b + (e - b) * i // k for i in range(k + 1)]
        slots, pairs = [], []
        for i in range(k):
            ctx.match_resident(edges[i], edges[i + 1], device_only=True)
            g, _, st = ctx.replay_accumulate(None, reset=(i == 0), materialise=(i == k - 1))
            slots.append(st["table_slots"])
            pairs.append(st["n_pairs"])
        out = {"slots": np.array(slots, np.uint64), "pairs": np.array(pairs, np.uint64)}
        for f in rc.FIELDS + rc.ARRAYS:
            out[f] = g[f]
        np.savez(sys.argv[1], **out)
    finally:
        ctx.close()
