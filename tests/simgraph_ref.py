"""Test reference of pipeline 1's compatibility graph: a restatement of the graph half of the reference's
polyline_matching_similarity_graph (matching/polyline_matching/polyline_matcher.cpp:222-327), of its text writer
(graph_adjacency_set_undirected_no_type_weighted.cpp:54-74) and of compute_polyline_matches_from_nodes_component_ids
(polyline_matcher.cpp:202-214) in Python.

The searches are polymatch_ref.Matcher.entry_results (pinned against the oracle's primitives by tests/test_polymatch_ref.py);
everything above them is written out as the reference has it: the sequential walk over the points, the node numbering by
first appearance through a dict, std::set iteration orders (sorted()), float sums in numpy float32 in the reference's order.
It imports nothing from the product libraries.
"""
import numpy as np

import polymatch_ref as pref

F32 = np.float32


def refpoint_weight(close_polylines):
    """compute_refpoint_weight (:191-200): int / (float) int."""
    non_empty = sum_pls = 0
    for spls in close_polylines:
        if len(spls) > 0:
            non_empty += 1
            sum_pls += len(spls)
    return F32(0.0) if non_empty == 0 else F32(F32(non_empty) / F32(sum_pls))


def weight_sum(weights, ids):
    """`float s = 0.0; for (id in ids) s += weights[id];` in the order given."""
    s = F32(0.0)
    for r in ids:
        s = F32(s + weights[r])
    return s


def compatibility(weights, a, b):
    """compute_compatibility (:171-189): a, b ascending; std::set_intersection / std::set_union give ascending ranges."""
    inter = weight_sum(weights, sorted(set(a) & set(b)))
    if inter == F32(0.0):
        return F32(0.0)
    return F32(inter / weight_sum(weights, sorted(set(a) | set(b))))


def similarity_graph(scene, points):
    """points: polymatch_ref.Matcher.entry_results of a seed range, ascending. Returns the arrays of eg3d_simgraph."""
    n_views = int(scene["n_views"])
    vpo = [int(x) for x in scene["view_pl_off"]]
    close_polylines = []
    close_refpoints = [[[] for _ in range(vpo[v + 1] - vpo[v])] for v in range(n_views)]
    node_of, nodes, adj = {}, [], []
    for refpoint_id, views, results in points:
        cur_cams_pls = set()
        for i, res in enumerate(results):
            for (pl, _) in res:
                cur_cams_pls.add((int(views[i]), int(pl)))
        cur = [set() for _ in range(n_views)]
        for (v, pl) in sorted(cur_cams_pls):
            cur[v].add(pl)
            close_refpoints[v][pl].append(refpoint_id)
        pl_ids = []
        for p in sorted(cur_cams_pls):
            if p not in node_of:
                node_of[p] = len(nodes)
                nodes.append(p)
                adj.append(set())
            pl_ids.append(node_of[p])
        for i in range(len(pl_ids)):
            for j in range(i + 1, len(pl_ids)):
                adj[pl_ids[i]].add(pl_ids[j])
                adj[pl_ids[j]].add(pl_ids[i])
        close_polylines.append(cur)
    visible = [set() for _ in range(n_views)]          # pointsVisibleFromCamN_
    for refpoint_id, views, _ in points:
        for v in views:
            visible[int(v)].add(refpoint_id)
    divided = [[[[r for r in close_refpoints[v1][pl] if r in visible[v2]] for v2 in range(n_views)]
                for pl in range(vpo[v1 + 1] - vpo[v1])] for v1 in range(n_views)]
    weights = {p[0]: refpoint_weight(close_polylines[i]) for i, p in enumerate(points)}
    wadj = [dict() for _ in nodes]
    for node1 in range(len(nodes)):
        for node2 in sorted(adj[node1]):
            if node1 < node2:
                (v1, p1), (v2, p2) = nodes[node1], nodes[node2]
                w = compatibility(weights, divided[v1][p1][v2], divided[v2][p2][v1])
                if w > 0.0:
                    wadj[node1][node2] = w
                    wadj[node2][node1] = w
    adj_off, adj_node, adj_w = [0], [], []
    for n in range(len(nodes)):
        for m in sorted(wadj[n]):
            adj_node.append(m)
            adj_w.append(wadj[n][m])
        adj_off.append(len(adj_node))
    cp_off, cp_view, cp_pl = [0], [], []
    for cur in close_polylines:
        for v in range(n_views):
            for pl in sorted(cur[v]):
                cp_view.append(v)
                cp_pl.append(pl)
        cp_off.append(len(cp_view))
    cr_off, cr_point = [0], []
    for v in range(n_views):
        for row in close_refpoints[v]:
            cr_point.extend(row)
            cr_off.append(len(cr_point))
    u = lambda a: np.array(a, np.uint32)
    return {"n_nodes": len(nodes), "node_view": u([n[0] for n in nodes]), "node_pl": u([n[1] for n in nodes]),
            "adj_off": u(adj_off), "adj_node": u(adj_node), "adj_w": np.array(adj_w, np.float32),
            "seed_begin": points[0][0] if points else 0, "n_points": len(points),
            "point_weight": np.array([weights[p[0]] for p in points], np.float32),
            "cp_off": u(cp_off), "cp_view": u(cp_view), "cp_pl": u(cp_pl), "n_polylines": vpo[-1],
            "cr_off": u(cr_off), "cr_point": u(cr_point),
            "n_pair_instances": sum(m * (m - 1) // 2 for m in np.diff(cp_off).tolist())}


def graph_text(g):
    """write_to_file: the directed edge count in the header, 1-based ids, the weight as an ofstream prints a float."""
    lines = ["p sp %d %d\n" % (g["n_nodes"], int(g["adj_off"][-1]))]
    for n1 in range(g["n_nodes"]):
        for k in range(int(g["adj_off"][n1]), int(g["adj_off"][n1 + 1])):
            lines.append("a %d %d %s\n" % (n1 + 1, int(g["adj_node"][k]) + 1, "%g" % float(g["adj_w"][k])))
    return "".join(lines)


def sets_from_communities(g, ids, n_views):
    """compute_polyline_matches_from_nodes_component_ids as the CSR of eg3d_polyline_sets."""
    num = (max(int(i) for i in ids) + 1) if len(ids) else 0
    res = [[set() for _ in range(n_views)] for _ in range(max(num, 0))]
    for i in range(g["n_nodes"]):
        if ids[i] >= 0:
            res[int(ids[i])][int(g["node_view"][i])].add(int(g["node_pl"][i]))
    row_off, pl_ids = [0], []
    for comp in res:
        for v in range(n_views):
            pl_ids.extend(sorted(comp[v]))
            row_off.append(len(pl_ids))
    return len(res), np.array(row_off, np.uint32), np.array(pl_ids, np.uint32)


def component_ids(g):
    """Connected components of the weighted adjacency, numbered in the order of their smallest node: stands in for a
    community detection in the end-to-end tests."""
    adj = [set(int(m) for m in g["adj_node"][g["adj_off"][n]:g["adj_off"][n + 1]]) for n in range(g["n_nodes"])]
    ids = np.zeros(g["n_nodes"], np.int64)
    for k, comp in enumerate(pref.components_stack_walk(g["n_nodes"], adj)):
        for n in comp:
            ids[n] = k
    return ids


class Graphs:
    """The restatement on seed ranges of one scene (the 10 px maps are built once)."""

    def __init__(self, scene, matcher=None):
        self.scene = scene
        self.m = matcher or pref.Matcher(scene)

    def graph(self, seeds, begin, end):
        g = similarity_graph(self.scene, self.m.entry_results(seeds, begin, end))
        g["seed_begin"] = begin
        return g
