"""An independent numpy restatement of the 3-D edge model (include/eg3d/host_edges.h): trace, simplify, length. It shares no
code with csrc/eg3d_edges_core.h and reads the rules from the header's text alone: the trace starts its walks at the
TERMINALS and takes the rings from what is left (the library walks polylines in ascending id), the incidences come from
pl_start / pl_end (the library reads the conn table), and the linearizable test is evaluated for all interior points at
once. Arithmetic: np.float32 operations in the stated order; the squared distance of `length` in float64, rounded once."""
import numpy as np

F = np.float32


def trace(g):
    """[(nodes, ring)] in chain order; nodes: the node ids of the chain's vertices."""
    ps, pe = np.asarray(g["pl_start"], np.int64), np.asarray(g["pl_end"], np.int64)
    inc = {}
    for p in range(len(ps)):
        if ps[p] != pe[p]:
            inc.setdefault(int(ps[p]), []).append(p)
            inc.setdefault(int(pe[p]), []).append(p)
    used, found = set(), []

    def walk(v, p):
        """from node v along polyline p until a node that is not pass-through (or v again): (nodes, polylines)"""
        nodes, pls = [v], []
        while True:
            used.add(p)
            pls.append(p)
            v = int(pe[p] if ps[p] == v else ps[p])
            nodes.append(v)
            if len(inc[v]) != 2 or v == nodes[0]:
                return nodes, pls
            p = inc[v][0] if inc[v][1] == p else inc[v][1]

    for v in sorted(inc):
        if len(inc[v]) == 2:
            continue
        for p in inc[v]:
            if p in used:
                continue
            nodes, pls = walk(v, p)
            if len(pls) == 1:
                nodes = [int(ps[p]), int(pe[p])]
            elif pls[-1] < pls[0]:
                nodes, pls = nodes[::-1], pls[::-1]
            found.append((min(pls), nodes, False))
    for p in range(len(ps)):
        if ps[p] == pe[p] or p in used:
            continue
        nodes, pls = walk(int(ps[p]), p)       # nodes[-1] == nodes[0]
        nodes = nodes[:-1]
        i = nodes.index(min(nodes))
        nodes, pls = nodes[i:] + nodes[:i], pls[i:] + pls[:i]   # pls[0] leaves the smallest node, pls[-1] arrives there
        if pls[-1] < pls[0]:
            nodes, pls = [nodes[0]] + nodes[:0:-1], pls[::-1]
        found.append((min(pls), nodes + [nodes[0]], True))
    found.sort(key=lambda c: c[0])
    return [(nodes, ring) for _, nodes, ring in found]


def distance_point_line_sq(p, a, b):
    """p, a, b: float32 arrays [..., 3] that broadcast against each other; the result has a leading axis at least. glm's
    cross and dot, operation for operation in float32."""
    p, a, b = np.atleast_2d(np.asarray(p, F)), np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        d0, d1, d2 = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        v0, v1, v2 = a[..., 0] - p[..., 0], a[..., 1] - p[..., 1], a[..., 2] - p[..., 2]
        cx = d1 * v2 - v1 * d2
        cy = d2 * v0 - v2 * d0
        cz = d0 * v1 - v0 * d1
        return ((cx * cx + cy * cy) + cz * cz) / ((d0 * d0 + d1 * d1) + d2 * d2)


def simplify(P, max_dist, info=None):
    """simplify_polyline on the points P [n, 3] float32: the kept indices. info["rounds"]: the largest number of times the
    do-while of find_compatible_se_eb ran. All candidates of one find_max_se / find_min_eb are evaluated at once (every
    interior point of every candidate interval: the same float32 operations, element by element) and the first that is
    linearizable in the reference's order is taken."""
    P = np.asarray(P, F)
    with np.errstate(over="ignore"):
        maxsq = F(max_dist) * F(max_dist)

    def find_max_se(start, max_se):
        if max_se <= start:
            return start
        cand = np.arange(max_se, start + 1, -1)                  # cur_se = max_se .. start + 2
        if len(cand):
            inner = np.arange(start + 1, max_se)
            off = distance_point_line_sq(P[inner][None, :, :], P[start], P[cand][:, None, :]) > maxsq
            good = ~np.any(off & (inner[None, :] < cand[:, None]), axis=1)
            if good.any():
                return int(cand[np.argmax(good)])
        return start + 1

    def find_min_eb(end, min_eb):
        if min_eb >= end:
            return end
        cand = np.arange(min_eb, end - 1)                        # cur_eb = min_eb .. end - 2
        if len(cand):
            inner = np.arange(min_eb + 1, end)
            off = distance_point_line_sq(P[inner][None, :, :], P[cand][:, None, :], P[end]) > maxsq
            good = ~np.any(off & (inner[None, :] > cand[:, None]), axis=1)
            if good.any():
                return int(cand[np.argmax(good)])
        return end - 1

    start, end = 0, len(P) - 1
    front, back = [start], [end]
    while end > start + 1:
        max_se, min_eb, rounds = end, start, 0
        while True:
            rounds += 1
            se = find_max_se(start, max_se)
            if se == end:
                eb = 0
                break
            eb = find_min_eb(end, min_eb)
            max_se -= 1
            min_eb += 1
            if not eb < se:
                break
        if info is not None:
            info["rounds"] = max(info.get("rounds", 0), rounds)
        if se == end:
            break
        front.append(se)
        if se != eb:
            back.append(eb)
        start, end = se, eb
    return front + back[::-1]


def length(P):
    P = np.asarray(P, F)
    if len(P) < 2:
        return F(0)
    d = (P[1:] - P[:-1]).astype(np.float64)                                     # the float32 differences, widened
    sq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)  # summed in float64, rounded once
    return np.add.accumulate(np.sqrt(sq), dtype=F)[-1]                          # 0 + d1 + d2 + ...: one after the other


def edge_chains(g, max_dist, simplify_on=True, info=None):
    """The dict host.edge_chains returns, without the times."""
    X = np.asarray(g["node_X"], F).reshape(-1, 3)
    chains = trace(g)
    chain_off, chain_node, flags, s_off, s_node, lengths = [0], [], [], [0], [], []
    for nodes, ring in chains:
        chain_node += nodes
        chain_off.append(len(chain_node))
        flags.append(1 if ring else 0)
        kept = list(nodes)
        if simplify_on:
            if len(nodes) >= 3 and nodes[0] == nodes[-1]:   # E1: without the closing vertex, which is appended again
                kept = [nodes[i] for i in simplify(X[nodes[:-1]], max_dist, info)] + [nodes[-1]]
            else:
                kept = [nodes[i] for i in simplify(X[nodes], max_dist, info)]
        s_node += kept
        s_off.append(len(s_node))
        lengths.append(length(X[kept]))
    ps, pe = np.asarray(g["pl_start"]), np.asarray(g["pl_end"])
    sizes = np.diff(chain_off)
    return {"chain_off": np.array(chain_off, np.uint64), "chain_node": np.array(chain_node, np.uint32),
            "flags": np.array(flags, np.uint32), "s_off": np.array(s_off, np.uint64), "s_node": np.array(s_node, np.uint32),
            "length": np.array(lengths, F),
            "stats": {"n_chains": len(chains), "n_rings": int(sum(flags)), "n_loops_dropped": int(np.sum(ps == pe)),
                      "n_vertices_in": len(chain_node), "n_vertices_kept": len(s_node),
                      "longest_chain": int(sizes.max()) if len(sizes) else 0}}


ARRAYS = ("chain_off", "chain_node", "flags", "s_off", "s_node", "length")
COUNTS = ("n_chains", "n_rings", "n_loops_dropped", "n_vertices_in", "n_vertices_kept", "longest_chain")


def difference(got, want):
    """None when the two results are equal array for array and bit for bit, counts included; else what differs."""
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: %s%s vs %s%s" % (k, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            i = int(np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[0]) // a.itemsize
            return "%s differs first at %d: %r vs %r" % (k, i, a[i], b[i])
    for k in COUNTS:
        if int(got["stats"][k]) != int(want["stats"][k]):
            return "stats.%s: %d vs %d" % (k, got["stats"][k], want["stats"][k])
    return None
