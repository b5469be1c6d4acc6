"""Plain-Python-loop restatement of the held-out edge split (include/dw_hip.h
dw_edge_holdout) and of dw_roc_auc's integer U2, written from the rule alone: Python ints and
loops, nothing shared with shallow_encoders/graph/holdout.py. Also the graphs the CPU and GPU
tests share."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def prio(u, v, seed):
    assert u < v
    return mix64((((u << 32) | v) ^ mix64(seed & M64)) & M64)


def split_edges(row_ptr, col, weights, ratio, seed):
    """(row_ptr', col', weights', held [n_hold, 2], info) by the rule, one edge at a time."""
    V = len(row_ptr) - 1
    edges = []                       # non-loop edges (u, v), u < v, in row order of the CSR
    for x in range(V):
        for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
            y = int(col[e])
            if y > x:
                edges.append((x, y))
    pr = {e: prio(e[0], e[1], seed) for e in edges}
    best = {}                        # node -> its incident non-loop edge of smallest priority
    for e in edges:
        for node in e:
            if node not in best or pr[e] < pr[best[node]]:
                best[node] = e
    protected = set(best.values())
    candidates = [e for e in edges if e not in protected]
    n_want = round(ratio * len(edges))
    n_hold = min(n_want, len(candidates))
    held_set = set(sorted(candidates, key=lambda e: pr[e])[:n_hold])
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
    info = {'n_edges': len(edges), 'n_want': n_want, 'n_candidates': len(candidates),
            'n_hold': n_hold}
    return (np.asarray(new_ptr, dtype=np.int64), np.asarray(new_col, dtype=np.int32),
            None if weights is None else np.asarray(new_w, dtype=np.float64),
            np.asarray(held, dtype=np.int64).reshape(-1, 2), info)


def u2_counts(scores, labels):
    """(U2, n_pos, n_neg): U2 = sum over positives i of 2 #{negatives j: s_j < s_i} +
    #{negatives j: s_j = s_i}, with Python float comparisons (-0.0 == 0.0)."""
    pos = [float(s) for s, y in zip(scores, labels) if y]
    neg = sorted(float(s) for s, y in zip(scores, labels) if not y)
    import bisect
    u2 = 0
    for s in pos:
        lb, ub = bisect.bisect_left(neg, s), bisect.bisect_right(neg, s)
        u2 += 2 * lb + (ub - lb)
    return u2, len(pos), len(neg)


def auc(scores, labels):
    u2, n_pos, n_neg = u2_counts(scores, labels)
    return u2 / (2 * n_pos * n_neg)


# ---- the graphs ----------------------------------------------------------------------------------
def karate(weighted):
    import networkx as nx
    from shallow_encoders.graph.csr import CSRGraph
    g = nx.karate_club_graph()
    g = nx.relabel_nodes(g, {n: f'n{n + 1:02d}' for n in g.nodes})
    if not weighted:
        for _, _, data in g.edges(data=True):
            data.pop('weight', None)
    return CSRGraph.from_networkx(g)


def triplets():
    import networkx as nx
    from shallow_encoders.graph.csr import CSRGraph
    g = nx.Graph()
    for p in 'abc':
        g.add_edge(f'{p}1', f'{p}2')
        g.add_edge(f'{p}2', f'{p}3')
    return CSRGraph.from_networkx(g)


def rmat12():
    from shallow_encoders.graph.rmat import rmat_graph
    return rmat_graph(12, 40000, 0)


def self_loops():
    """60 nodes, random edges with repeats, 8 self-loops (a loop is one CSR entry), weighted."""
    from shallow_encoders.graph.edge_list import edge_list_csr
    rng = np.random.default_rng(5)
    src = rng.integers(0, 60, 300)
    dst = rng.integers(0, 60, 300)
    src[:8] = dst[:8] = np.arange(8) * 7
    return edge_list_csr(src, dst, weights=rng.random(300))


def star(n_leaves=9):
    from shallow_encoders.graph.edge_list import edge_list_csr
    return edge_list_csr(np.zeros(n_leaves, dtype=np.int64), np.arange(1, n_leaves + 1))


def path(n=8):
    from shallow_encoders.graph.edge_list import edge_list_csr
    return edge_list_csr(np.arange(n - 1), np.arange(1, n))


# the score sets of the AUC tests: (name, scores float64, labels uint8)
def auc_cases():
    rng = np.random.default_rng(11)
    n = 400
    y = (rng.random(n) < 0.4).astype(np.uint8)
    y[:2] = (1, 0)
    cont = rng.standard_normal(n) + y
    sep = np.where(y == 1, 2.0 + rng.random(n), rng.random(n))
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    inf = rng.standard_normal(n)
    inf[rng.random(n) < 0.2] = np.inf
    inf[rng.random(n) < 0.2] = -np.inf
    inf[rng.random(n) < 0.1] = -0.0
    inf[rng.random(n) < 0.1] = 0.0
    return [('continuous', cont, y),
            ('seven_values', np.round(3 * cont).clip(-3, 3) / 3, y),
            ('all_equal', np.full(n, 0.25), y),
            ('separated', sep, y),
            ('separated_reversed', -sep, y),
            ('signed_zeros', zeros, y),
            ('inf_and_zeros', inf, y)]
