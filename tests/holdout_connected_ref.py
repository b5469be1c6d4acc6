"""Plain-Python restatement of the connected held-out edge split (``protect='connected'``;
DESIGN.md §4.4.1, include/dw_hip.h dw_edge_forest), written from the rule alone: Kruskal with a
union-find over Python ints, a breadth-first search for the components, nothing shared with
shallow_encoders/graph/holdout.py. Also the extra graphs of the CPU and GPU tests, each the
smallest shape at which one part of the kernels can go wrong."""
from collections import deque

import numpy as np

from holdout_ref import prio


def csr_edges(row_ptr, col):
    """The non-loop edges (u, v), u < v, in the row order of the CSR."""
    edges = []
    for x in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
            if int(col[e]) > x:
                edges.append((x, int(col[e])))
    return edges


def forest(row_ptr, col, seed):
    """The minimum spanning forest under prio as a set of edges (Kruskal): the edges in
    ascending priority, each taken when its ends are in different trees."""
    edges = csr_edges(row_ptr, col)
    root = list(range(len(row_ptr) - 1))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    taken = set()
    for u, v in sorted(edges, key=lambda e: prio(e[0], e[1], seed)):
        a, b = find(u), find(v)
        if a != b:
            root[a] = b
            taken.add((u, v))
    return taken


def components(row_ptr, col):
    """labels int32[V]: the smallest row of every row's connected component (breadth-first, rows
    in ascending order, so a component's first row is its smallest)."""
    V = len(row_ptr) - 1
    labels = [-1] * V
    for s in range(V):
        if labels[s] >= 0:
            continue
        labels[s] = s
        queue = deque([s])
        while queue:
            x = queue.popleft()
            for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
                y = int(col[e])
                if labels[y] < 0:
                    labels[y] = s
                    queue.append(y)
    return np.asarray(labels, dtype=np.int32)


def split_edges(row_ptr, col, weights, ratio, seed):
    """(row_ptr', col', weights', held [n_hold, 2], info) in holdout_ref.split_edges' format: the
    forest is protected, the n_hold other non-loop edges of smallest priority are held."""
    V = len(row_ptr) - 1
    edges = csr_edges(row_ptr, col)
    protected = forest(row_ptr, col, seed)
    candidates = [e for e in edges if e not in protected]
    n_want = round(ratio * len(edges))
    n_hold = min(n_want, len(candidates))
    held_set = set(sorted(candidates, key=lambda e: prio(e[0], e[1], seed))[:n_hold])
    held = [e for e in edges if e in held_set]
    new_ptr, new_col, new_w = [0], [], []
    for x in range(V):
        for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
            y = int(col[e])
            if (min(x, y), max(x, y)) in held_set:
                continue
            new_col.append(y)
            if weights is not None:
                new_w.append(float(weights[e]))
        new_ptr.append(len(new_col))
    labels = components(row_ptr, col)
    touched = {n for e in edges for n in e}
    info = {'n_edges': len(edges), 'n_want': n_want, 'n_candidates': len(candidates),
            'n_hold': n_hold, 'n_forest': len(protected),
            'n_components': len({int(labels[n]) for n in touched})}
    return (np.asarray(new_ptr, dtype=np.int64), np.asarray(new_col, dtype=np.int32),
            None if weights is None else np.asarray(new_w, dtype=np.float64),
            np.asarray(held, dtype=np.int64).reshape(-1, 2), info)


def degree_protected(row_ptr, col, seed):
    """The edges the degree rule protects: every node's non-loop edge of smallest priority."""
    best = {}
    for e in csr_edges(row_ptr, col):
        for node in e:
            if node not in best or prio(e[0], e[1], seed) < prio(best[node][0], best[node][1],
                                                                 seed):
                best[node] = e
    return set(best.values())


# ---- the graphs ----------------------------------------------------------------------------------
def from_edges(n_nodes, edges):
    """CSRGraph over rows 0 .. n_nodes (row 0 <unk>; node i is row i + 1, with or without an
    edge), each row's neighbours ascending."""
    from shallow_encoders.graph.csr import CSRGraph
    nbrs = [set() for _ in range(n_nodes + 1)]
    for a, b in edges:
        nbrs[a + 1].add(b + 1)
        nbrs[b + 1].add(a + 1)
    row_ptr = np.cumsum([0] + [len(s) for s in nbrs])
    col = [y for s in nbrs for y in sorted(s)]
    return CSRGraph.from_arrays(row_ptr, col)


def cycle(n=5000):
    """One cycle: n - 1 forest edges in a few rounds, so long chains of hooks; exactly one
    candidate, the edge of largest priority."""
    return from_edges(n, [(i, (i + 1) % n) for i in range(n)])


BRIDGE = (6, 8)          # rows of the bridge's ends in bridge()


def bridge():
    """Two 6-cliques (nodes 0-5 and 7-12) joined by the edge {5, 7}; node 6 has no edge."""
    edges = [(a + o, b + o) for o in (0, 7) for a in range(6) for b in range(a + 1, 6)]
    return from_edges(13, edges + [(5, 7)])


def grid(n=8):
    edges = [(r * n + c, r * n + c + 1) for r in range(n) for c in range(n - 1)]
    edges += [(r * n + c, (r + 1) * n + c) for r in range(n - 1) for c in range(n)]
    return from_edges(n * n, edges)


def three_cycles():
    """Disjoint cycles of 3, 4 and 5 nodes: three components, one candidate each."""
    edges, at = [], 0
    for n in (3, 4, 5):
        edges += [(at + i, at + (i + 1) % n) for i in range(n)]
        at += n
    return from_edges(12, edges)


def graphs():
    """name -> builder: the shared graphs of holdout_ref and the four above."""
    import holdout_ref as ref
    return {'karate': lambda: ref.karate(False), 'karate_weighted': lambda: ref.karate(True),
            'triplets': ref.triplets, 'rmat12': ref.rmat12, 'self_loops': ref.self_loops,
            'star': ref.star, 'path': ref.path, 'cycle': cycle, 'bridge': bridge, 'grid': grid,
            'three_cycles': three_cycles}
