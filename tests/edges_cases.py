"""Hand-built graphs for the 3-D edge model (include/eg3d/host_edges.h): for every rule of the trace and of the
simplification the smallest shape at which it can go wrong, and seeded random graphs. cases() gives {name: (graph, max_dist)};
a graph is the geometric half of a graph3d dict (n_nodes, n_real_nodes, n_polylines, node_X, pl_start, pl_end, conn_off,
conn_pl), its conn rows in ascending polyline id with a loop linked once, as the replay builds them."""
import numpy as np

F = np.float32


def make_graph(n_nodes, polylines, X=None):
    """polylines: [(start, end)]. X: [n_nodes, 3] or None (every node at its id on the x axis)."""
    ps = np.array([p[0] for p in polylines], np.uint32)
    pe = np.array([p[1] for p in polylines], np.uint32)
    rows = [[] for _ in range(n_nodes)]
    for i, (s, e) in enumerate(polylines):
        rows[s].append(i)
        if e != s:
            rows[e].append(i)
    off = np.zeros(n_nodes + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    if X is None:
        X = np.stack([np.arange(n_nodes), np.zeros(n_nodes), np.zeros(n_nodes)], 1)
    X = np.ascontiguousarray(X, F).reshape(n_nodes, 3)
    return {"n_nodes": n_nodes, "n_real_nodes": n_nodes, "n_polylines": len(polylines), "node_X": X, "pl_start": ps, "pl_end": pe,
            "conn_off": off, "conn_pl": np.array([p for r in rows for p in r], np.uint32)}


def path(points, seed=None, extra_nodes=0):
    """A path through `points` [n, 3]; with a seed its node ids and polyline ids (and each polyline's direction) are shuffled."""
    n = len(points)
    node = np.arange(n)
    order = np.arange(n - 1)
    flip = np.zeros(n - 1, bool)
    if seed is not None:
        rng = np.random.default_rng(seed)
        node = rng.permutation(n + extra_nodes)[:n]
        order = rng.permutation(n - 1)
        flip = rng.random(n - 1) < 0.5
    X = np.zeros((n + extra_nodes, 3), F)
    X[node] = np.asarray(points, F)
    pls = [None] * (n - 1)
    for k in range(n - 1):
        a, b = int(node[k]), int(node[k + 1])
        pls[order[k]] = (b, a) if flip[k] else (a, b)
    return make_graph(n + extra_nodes, pls, X)


def ring(n, seed=None, radius=10.0):
    t = 2 * np.pi * np.arange(n) / n
    pts = np.stack([radius * np.cos(t), radius * np.sin(t), 0.1 * np.arange(n)], 1)
    g = path(np.concatenate([pts, pts[:1]]), None)
    # close it: the path's last node becomes its first
    pls = [(int(s), int(e) % n) for s, e in zip(g["pl_start"], g["pl_end"])]
    X = g["node_X"][:n]
    if seed is not None:
        rng = np.random.default_rng(seed)
        node, order = rng.permutation(n), rng.permutation(n)
        Xs = np.zeros_like(X)
        Xs[node] = X
        shuffled = [None] * n
        for k, (s, e) in enumerate(pls):
            shuffled[order[k]] = (int(node[s]), int(node[e]))
        pls, X = shuffled, Xs
    return make_graph(n, pls, X)


def polyline_points(n, corners, seed=0):
    """n points along a polyline with the given number of corners: exactly collinear runs on an integer lattice, so that a
    simplification keeps the corners and the reference restatement stays quick on long chains."""
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(1, n - 1), corners, replace=False).tolist()) if corners else []
    steps = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)]
    pts, p, k = [], np.zeros(3), 0
    for i in range(n):
        pts.append(p.copy())
        if i in cuts:
            k += 1
        p = p + np.array(steps[k % len(steps)], float)
    return np.array(pts, F)


def arc(n, radius=100.0, sweep=np.pi / 2):
    t = sweep * np.arange(n) / (n - 1)
    return np.stack([radius * np.cos(t), radius * np.sin(t), 0.25 * t], 1).astype(F)


def random_graph(seed):
    """<= 200 nodes, degrees 0-4 (a loop counts once in a row and not at all in a degree), one polyline per unordered pair,
    loops included; positions on a small integer lattice, so that collinear runs and exact ties occur."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 201))
    deg = np.zeros(n, int)
    pairs, pls = set(), []
    # a few long runs first (chains and rings), then random pairs
    free = list(rng.permutation(n))
    while len(free) >= 3 and rng.random() < 0.8:
        k = int(rng.integers(3, min(len(free), 40) + 1))
        run, free = free[:k], free[k:]
        closed = rng.random() < 0.3
        for a, b in zip(run, run[1:] + ([run[0]] if closed else [])):
            a, b = int(a), int(b)
            if a != b and (min(a, b), max(a, b)) not in pairs:
                pairs.add((min(a, b), max(a, b)))
                pls.append((a, b))
                deg[a] += 1
                deg[b] += 1
    for _ in range(int(rng.integers(0, n))):
        a, b = int(rng.integers(n)), int(rng.integers(n))
        if a == b:
            if (a, a) not in pairs and rng.random() < 0.5:
                pairs.add((a, a))
                pls.append((a, a))
            continue
        if deg[a] >= 4 or deg[b] >= 4 or (min(a, b), max(a, b)) in pairs:
            continue
        pairs.add((min(a, b), max(a, b)))
        pls.append((a, b))
        deg[a] += 1
        deg[b] += 1
    order = rng.permutation(len(pls))
    pls = [pls[i] for i in order]
    X = rng.integers(0, 6, (n, 3)).astype(F)
    return make_graph(n, pls, X), float(rng.choice([0.0, 0.5, 1.0, 2.5]))


def random_cases(count=40, seed0=0x17ED6E5):
    return {"random_%02d" % i: random_graph(seed0 + i) for i in range(count)}


def trace_cases():
    c = {}
    c["empty"] = make_graph(0, [])
    c["nodes_without_polylines"] = make_graph(3, [])
    c["one_polyline"] = make_graph(2, [(1, 0)])
    # 0 - 1 - 2 with the polyline at node 2 numbered first: the chain runs 2, 1, 0 ... and stored against that direction
    c["path_reversed_orientation"] = make_graph(3, [(1, 2), (0, 1)])
    c["path_reversed_orientation_b"] = make_graph(3, [(2, 1), (1, 0)])
    # a star: hub 0, arms of 1, 2 and 5 polylines
    star, nxt = [], 1
    for arm in (1, 2, 5):
        prev = 0
        for _ in range(arm):
            star.append((prev, nxt))
            prev, nxt = nxt, nxt + 1
    star = [star[i] for i in (3, 0, 7, 5, 1, 6, 2, 4)]
    c["star_1_2_5"] = make_graph(nxt, star, np.random.default_rng(5).integers(0, 9, (nxt, 3)))
    for n in (3, 64, 65):
        c["ring_%d" % n] = ring(n, seed=n)
    # the smallest node (0) lies between polylines 1 and 2; polyline 0 is elsewhere on the ring
    c["ring_smallest_node_off_polyline_0"] = make_graph(4, [(2, 3), (0, 1), (3, 0), (1, 2)],
                                                        [[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 1]])
    # hub 0 with a closed chain 0-1-2-3-0 and one arm 0-4: first vertex == last vertex on an open chain
    c["closed_chain_on_a_hub"] = make_graph(5, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4)],
                                            [[0, 0, 0], [3, 0, 0], [3, 3, 0], [0, 3, 0], [-5, -5, 0]])
    c["closed_chain_on_a_hub_reversed"] = make_graph(5, [(3, 0), (2, 1), (2, 3), (1, 0), (4, 0)],
                                                     [[0, 0, 0], [3, 0, 0], [3, 3, 0], [0, 3, 0], [-5, -5, 0]])
    c["loop_on_a_pass_through_node"] = make_graph(3, [(0, 1), (1, 1), (1, 2)], [[0, 0, 0], [1, 1, 0], [2, 0, 0]])
    c["loop_on_an_isolated_node"] = make_graph(4, [(2, 2), (0, 1)])
    for n in (63, 64, 65, 1025):
        c["path_%d_shuffled" % n] = path(polyline_points(n + 1, 6, seed=n), seed=n, extra_nodes=3)
    # two chains 0-1-2-3 and 4-5-6-7 whose polyline ids interleave
    c["two_chains_interleaved"] = make_graph(8, [(4, 5), (0, 1), (5, 6), (1, 2), (6, 7), (2, 3)])
    return {k: (g, 0.01) for k, g in c.items()}


def simplify_cases():
    c = {}
    c["two_vertices"] = (path([[0, 0, 0], [1, 2, 3]]), 0.01)
    c["three_vertices"] = (path([[0, 0, 0], [1, 1, 0], [2, 0, 0]]), 0.01)
    c["collinear"] = (path([[i, 2 * i, -i] for i in range(5)]), 0.01)
    c["an_L"] = (path([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 1, 0], [2, 2, 0]]), 0.01)
    c["zigzag"] = (path([[i, i % 2, 0] for i in range(9)]), 0.01)
    # |cross|^2 / |d|^2 = 4 / 16 = 0.25 = 0.5 * 0.5 exactly: NOT > maxsq, the chain is linearizable
    c["quotient_equals_maxsq"] = (path([[0, 0, 0], [1, 0.5, 0], [4, 0, 0]]), 0.5)
    c["quotient_just_above_maxsq"] = (path([[0, 0, 0], [1, 0.5, 0], [4, 0, 0]]), float(np.nextafter(F(0.5), F(0))))
    c["ends_with_se_equal_eb"] = c["an_L"]
    # a shallow bend: the first four and the last four points are within tolerance of their chords, all five are not —
    # the first eb (1) lies before the first se (3) and find_compatible_se_eb goes round again
    # (y = 0.1 x^2: a chord over four points stays within 0.2 of them, the chord over all five is 0.37 from the middle one)
    c["first_eb_before_se"] = (path([[x, 0.1 * x * x, 0] for x in range(5)]), 0.3)
    for n in (65, 129):
        c["arc_%d" % n] = (path(arc(n), seed=n), 0.05)
    c["max_dist_zero_zigzag"] = (c["zigzag"][0], 0.0)
    c["max_dist_zero_collinear"] = (c["collinear"][0], 0.0)
    c["max_dist_huge"] = (c["zigzag"][0], 1e30)
    c["ring_simplified"] = (ring(65, seed=1), 0.5)
    return c


def cases():
    out = trace_cases()
    out.update(simplify_cases())
    return out


# ---- the inconsistencies eg3d_host_edge_chains refuses ------------------------------------------------------------------------
def broken_graphs():
    """{name: graph} — each is a sound graph with ONE of the listed inconsistencies."""
    def base():
        g = make_graph(4, [(0, 1), (1, 2), (2, 2), (2, 3)])
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    out = {}
    g = base(); g["pl_end"][1] = 4; out["node_id_out_of_range"] = g
    g = base(); g["pl_start"][0] = 0xFFFFFFFF; out["node_id_far_out_of_range"] = g
    g = base(); g["conn_pl"][0] = 4; out["polyline_id_out_of_range"] = g
    g = base(); g["conn_off"][1], g["conn_off"][2] = g["conn_off"][2], g["conn_off"][1]; out["conn_off_descends"] = g
    g = base(); g["conn_off"][0] = 1; out["conn_off_does_not_start_at_0"] = g
    g = base(); g["conn_off"][-1] -= 1; out["conn_off_ends_before_the_table"] = g
    g = base(); g["conn_off"][-1] += 1; g["conn_pl"] = np.append(g["conn_pl"], np.uint32(3)); out["conn_off_ends_past_the_table"] = g
    g = base(); g["conn_pl"][2] = g["conn_pl"][1]; out["polyline_twice_in_a_row"] = g       # node 1: [0, 1] -> [0, 0]
    g = base(); g["conn_pl"][0] = 3; out["entry_names_a_polyline_elsewhere"] = g            # node 0 lists 2-3
    # the loop linked twice: a table of 2 * n_polylines entries instead of 2 * n_polylines - n_loops
    g = base()
    at = int(g["conn_off"][2])
    g["conn_pl"] = np.insert(g["conn_pl"], at, np.uint32(2))
    g["conn_off"][3:] += 1
    out["loop_linked_twice"] = g
    return out
