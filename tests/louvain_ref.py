"""The definition of K11 (eg3d_detect_communities), restated with Python ints: a deterministic Louvain on exact fixed-point
weights. Synchronous sweeps, ties to the smaller label, singleton swap protection, phases; no float sum
anywhere: a float weight w is the integer q = round(w * 2^32) (exact product, ties to even, as llrint), every sum is an
integer sum, gains and the modularity numerator are exact integers, and doubles appear only in the two threshold tests.

The graph is a CSR as in eg3d_simgraph: both directions of every edge, neighbours strictly ascending, no self-loop."""
import numpy as np

DEFAULTS = dict(max_phases=200, max_sweeps=1000, sweep_threshold=1e-6, phase_threshold=1e-6)


def quantize(w):
    """q of a float32 weight: llrint((double)w * 2^32)."""
    return int(round(float(np.float32(w)) * 4294967296.0))


def csr_from_edges(n_nodes, edges):
    """(adj_off uint32, adj_node uint32, adj_w float32) of undirected edges (i, j, w): both directions, rows ascending."""
    rows = [dict() for _ in range(n_nodes)]
    for i, j, w in edges:
        assert i != j and j not in rows[i]
        rows[i][j] = w
        rows[j][i] = w
    off = np.zeros(n_nodes + 1, np.uint32)
    node, wt = [], []
    for i, r in enumerate(rows):
        for j in sorted(r):
            node.append(j)
            wt.append(r[j])
        off[i + 1] = len(node)
    return off, np.array(node, np.uint32), np.array(wt, np.float32)


def numer(rows, C, k, M):
    """N of the partition C of the current graph: (weight of the entries inside a community) * M - sum of a_c^2."""
    inside = 0
    for i, row in enumerate(rows):
        for j, q in row:
            if C[i] == C[j]:
                inside += q
    a = {}
    for i, c in enumerate(C):
        a[c] = a.get(c, 0) + k[i]
    return inside * M - sum(v * v for v in a.values())


def target(i, rows, C, k, a, size, M):
    x = C[i]
    e = {}
    for j, q in rows[i]:
        if j != i:
            e[C[j]] = e.get(C[j], 0) + q
    eix = e.get(x, 0)
    ax = a[x] - k[i]
    best, best_g = x, 0
    for y in sorted(e):
        if y == x:
            continue
        g = (e[y] - eix) * M - k[i] * (a[y] - ax)
        if g > best_g:                      # ascending y: an equal gain keeps the smaller label
            best, best_g = y, g
    if best != x and size[x] == 1 and size[best] == 1 and best > x:
        best = x
    return best


def louvain(n_nodes, adj_off, adj_node, adj_w, max_phases=0, max_sweeps=0, sweep_threshold=0.0, phase_threshold=0.0):
    """Returns ids (int64, -1 for a node without a row), the counters of eg3d_louvain_stats, N as a Python int, and `trace`:
    per phase the list [N0, N after every accepted sweep]. A parameter of 0 is its default."""
    max_phases = max_phases or DEFAULTS["max_phases"]
    max_sweeps = max_sweeps or DEFAULTS["max_sweeps"]
    sweep_threshold = sweep_threshold or DEFAULTS["sweep_threshold"]
    phase_threshold = phase_threshold or DEFAULTS["phase_threshold"]
    off = [int(v) for v in adj_off]
    live = [i for i in range(n_nodes) if off[i + 1] > off[i]]
    pos = {v: r for r, v in enumerate(live)}
    rows = [[(pos[int(adj_node[p])], quantize(adj_w[p])) for p in range(off[i], off[i + 1])] for i in live]
    M = sum(q for row in rows for _, q in row)
    member = list(range(len(live)))
    n_phases = n_sweeps = 0
    N = 0
    trace = []
    if M:
        MM = float(M) * float(M)
        for _ in range(max_phases):
            n = len(rows)
            k = [sum(q for _, q in row) for row in rows]
            C = list(range(n))
            N0 = Nprev = numer(rows, C, k, M)
            trace.append([N0])
            for _ in range(max_sweeps):
                a, size = [0] * n, [0] * n
                for i in range(n):
                    a[C[i]] += k[i]
                    size[C[i]] += 1
                T = [target(i, rows, C, k, a, size, M) for i in range(n)]
                n_sweeps += 1
                if T == C:
                    break
                Nnew = numer(rows, T, k, M)
                if float(Nnew - Nprev) < sweep_threshold * MM:
                    break
                C, Nprev = T, Nnew
                trace[-1].append(Nnew)
            n_phases += 1
            N = Nprev
            if C == list(range(n)):
                break
            new = {}
            for c in C:
                new.setdefault(c, len(new))
            C = [new[c] for c in C]
            member = [C[m] for m in member]
            if float(Nprev - N0) < phase_threshold * MM:
                break
            W = [dict() for _ in range(len(new))]
            for i, row in enumerate(rows):
                for j, q in row:
                    W[C[i]][C[j]] = W[C[i]].get(C[j], 0) + q
            rows = [sorted(r.items()) for r in W]
    ids = np.full(n_nodes, -1, np.int64)
    for r, v in enumerate(live):
        ids[v] = member[r]
    return dict(ids=ids, n_communities=(max(member) + 1 if member else 0), n_phases=n_phases, n_sweeps=n_sweeps,
                n_isolated=n_nodes - len(live), total_q=M, numer=N, numer_hi=(N >> 64) & (2 ** 64 - 1), numer_lo=N & (2 ** 64 - 1),
                modularity=(float(N) / (float(M) * float(M)) if M else 0.0), trace=trace)


def communities_text(ids):
    """The communities file as Grappolo writes it and the reference reads it: one id per line."""
    return "".join("%d\n" % int(i) for i in ids)


# ---- the hand graphs of the tests --------------------------------------------------------------------------------------------
def two_triangles():
    """Two triangles joined by a 0.1 edge, and an isolated node 6."""
    e = [(0, 1, 1.0), (0, 2, 1.0), (1, 2, 1.0), (3, 4, 1.0), (3, 5, 1.0), (4, 5, 1.0), (2, 3, 0.1)]
    return (7,) + csr_from_edges(7, e)


def clique(n=6, w=1.0):
    return (n,) + csr_from_edges(n, [(i, j, w) for i in range(n) for j in range(i + 1, n)])


def star(leaves=200, w=0.5):
    return (leaves + 1,) + csr_from_edges(leaves + 1, [(0, 1 + i, w) for i in range(leaves)])


def ring_of_cliques(n_cliques=30, size=5):
    e = []
    for c in range(n_cliques):
        b = c * size
        e += [(b + i, b + j, 1.0) for i in range(size) for j in range(i + 1, size)]
        e.append((b + size - 1, ((c + 1) % n_cliques) * size, 1.0))
    return (n_cliques * size,) + csr_from_edges(n_cliques * size, e)


def path(n=100, w=1.0):
    return (n,) + csr_from_edges(n, [(i, i + 1, w) for i in range(n - 1)])


def planted(seed, blocks=8, size=24, p_in=0.5, p_out=0.01):
    """blocks x size nodes; inside a block an edge with probability p_in and a weight in 0.05..1, between blocks with p_out
    and a weight in 0.01..0.2, from random.Random(seed)."""
    import random
    rnd = random.Random(seed)
    n = blocks * size
    e = []
    for i in range(n):
        for j in range(i + 1, n):
            if i // size == j // size:
                if rnd.random() < p_in:
                    e.append((i, j, rnd.uniform(0.05, 1.0)))
            elif rnd.random() < p_out:
                e.append((i, j, rnd.uniform(0.01, 0.2)))
    return (n,) + csr_from_edges(n, e)


def long_row(n=1501, size=5):
    """Node 0 is joined to all others by light edges (a row of n - 1 entries); the others form cliques of `size`."""
    e = [(0, i, 0.01) for i in range(1, n)]
    for b in range(1, n, size):
        e += [(b + i, b + j, 1.0) for i in range(size) for j in range(i + 1, size)]
    return (n,) + csr_from_edges(n, e)
