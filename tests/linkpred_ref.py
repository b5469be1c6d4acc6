"""Host restatement of csrc/dw_linkpred.hip (TEST INFRASTRUCTURE): the rank-sampled non-edges of
dw_negative_edges (include/dw_hip.h) with oracle/philox.py's philox and bounded64, and the sums
of dw_edge_logreg in numpy — the operator in float32, everything after it in float64."""
import networkx as nx
import numpy as np

from oracle import philox as px

TAG_LINKPRED = 0x4C500000   # 'LP' (no other kernel's tag: oracle/philox.py TAG_*)
OPS = ('average', 'hadamard', 'weighted_l1', 'weighted_l2')


def sorted_rows(row_ptr, col):
    """col with every row ascending (what dw_csr_sort_copy builds)."""
    out = np.asarray(col, dtype=np.int64).copy()
    for r in range(len(row_ptr) - 1):
        out[row_ptr[r]:row_ptr[r + 1]].sort()
    return out


def rank_non_neighbour(c, first_node: int, k: int) -> int:
    """The k-th (0-based) node >= first_node that is not in the ascending row c: first_node + k +
    j, j the smallest index with c[j] - first_node - j > k (len(c) when there is none) — by the
    kernel's binary search."""
    lo, hi = 0, len(c)
    while lo < hi:
        mid = (lo + hi) >> 1
        if int(c[mid]) - first_node - mid > k:
            hi = mid
        else:
            lo = mid + 1
    return first_node + k + lo


def negative_edges(row_ptr, col_sorted, first_node: int, n: int, seed: int,
                   offset: int = 0) -> np.ndarray:
    """int64 [n, 2]: sample i, g = offset + i, from philox({lo g, hi g, 0, 'LP'}, seed)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_nodes = len(row_ptr) - 1 - first_node
    g = (np.arange(n, dtype=np.uint64) + np.uint64(offset % 2 ** 64))
    r = px.philox(g & np.uint64(px.MASK), g >> np.uint64(32), np.zeros(n, np.uint64),
                  np.full(n, TAG_LINKPRED, np.uint64), seed & px.MASK, (seed >> 32) & px.MASK)
    u = first_node + px.bounded64(r[0], r[1], n_nodes)
    out = np.empty((n, 2), dtype=np.int64)
    out[:, 0] = u
    z, w = r[2], r[3]
    for i in range(n):
        a, b = int(row_ptr[u[i]]), int(row_ptr[u[i] + 1])
        m = n_nodes - (b - a)
        if m <= 0:
            out[i, 1] = u[i]
            continue
        k = int(px.bounded64(z[i:i + 1], w[i:i + 1], m)[0])
        out[i, 1] = rank_non_neighbour(col_sorted[a:b], first_node, k)
    return out


def negative_edges_fast(row_ptr, col_sorted, first_node: int, n: int, seed: int,
                        offset: int = 0) -> np.ndarray:
    """negative_edges vectorised over the samples (the binary search in lock step), for the
    100,000-sample comparisons; equal to negative_edges (tests/test_linkpred.py)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    cs = np.asarray(col_sorted, dtype=np.int64)
    n_nodes = len(row_ptr) - 1 - first_node
    g = (np.arange(n, dtype=np.uint64) + np.uint64(offset % 2 ** 64))
    r = px.philox(g & np.uint64(px.MASK), g >> np.uint64(32), np.zeros(n, np.uint64),
                  np.full(n, TAG_LINKPRED, np.uint64), seed & px.MASK, (seed >> 32) & px.MASK)
    u = first_node + px.bounded64(r[0], r[1], n_nodes)
    a = row_ptr[u]
    deg = row_ptr[u + 1] - a
    m = n_nodes - deg
    assert (m > 0).all()
    # bounded64 with a per-sample bound: hi * m + ((lo * m) >> 32) >> 32, all below 2^64
    mm = m.astype(np.uint64)
    s32 = np.uint64(32)
    k = ((r[3] * mm + ((r[2] * mm) >> s32)) >> s32).astype(np.int64)
    lo, hi = np.zeros(n, np.int64), deg.copy()
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        idx = np.where(act, a + mid, 0)
        idx = np.minimum(idx, max(len(cs) - 1, 0))
        up = act & (cs[idx] - first_node - mid > k)
        down = act & ~up
        hi = np.where(up, mid, hi)
        lo = np.where(down, mid + 1, lo)
    return np.stack([u, first_node + k + lo], axis=1)


def edge_op(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The operator in float32, in the kernel's operation order."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    if op == 0:
        return (a + b) * np.float32(0.5)
    if op == 1:
        return a * b
    if op == 2:
        return np.abs(a - b)
    t = a - b
    return t * t


def features(table, op: int, pairs) -> np.ndarray:
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float32)
    return edge_op(op, table[pairs[:, 0]], table[pairs[:, 1]])


def logreg_sums(table, op: int, pairs, labels, coef):
    """dw_edge_logreg's out (float64 [d + 3]) and, for the tests' bounds, the sums of the terms'
    magnitudes (same layout; [d + 2] = 0) and (min |z|, max over samples of sum |w_j x_j|)."""
    x = features(table, op, pairs).astype(np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    d = x.shape[1]
    y = (np.asarray(labels) != 0).astype(np.float64)
    z = x @ coef[:d] + coef[d]
    e = np.exp(-np.abs(z))
    loss = np.log1p(e) + np.maximum(z, 0.0) - y * z
    sig = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    r = sig - y
    out = np.empty(d + 3)
    mag = np.zeros(d + 3)
    out[:d] = r @ x
    mag[:d] = np.abs(r) @ np.abs(x)
    out[d], mag[d] = r.sum(), np.abs(r).sum()
    out[d + 1], mag[d + 1] = loss.sum(), np.abs(loss).sum()
    out[d + 2] = float(((z > 0) == (y != 0)).sum())
    margin = (float(np.abs(z).min()), float((np.abs(x) @ np.abs(coef[:d])).max()))
    return out, mag, margin


def objective(x64: np.ndarray, y: np.ndarray, coef: np.ndarray, C: float = 1.0) -> float:
    """sklearn's objective C * sum(loss) + 0.5 ||w||^2 on float64 features."""
    d = x64.shape[1]
    z = x64 @ coef[:d] + coef[d]
    loss = np.log1p(np.exp(-np.abs(z))) + np.maximum(z, 0.0) - y * z
    return C * float(loss.sum()) + 0.5 * float(coef[:d] @ coef[:d])


def karate():
    """(graph with names n00..n33, row_ptr, col (networkx order), col_sorted): vocabulary ids
    1..34 in name order, row 0 = <unk>."""
    g = nx.relabel_nodes(nx.karate_club_graph(), {i: f'n{i:02d}' for i in range(34)})
    stoi = {v: i + 1 for i, v in enumerate(sorted(g.nodes))}
    row_ptr = np.zeros(36, dtype=np.int64)
    rows = [[]] + [[stoi[x] for x in g.neighbors(v)] for v in sorted(g.nodes)]
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([x for r in rows for x in r], dtype=np.int32)
    return g, row_ptr, col, sorted_rows(row_ptr, col)


def karate_problem(seed: int = 5):
    """The logistic-regression inputs of the driver tests: default_rng(2).normal((35, 8)) as the
    table, karate's 78 edges as positives, 78 restated negatives."""
    g, row_ptr, col, cs = karate()
    stoi = {v: i + 1 for i, v in enumerate(sorted(g.nodes))}
    table = np.random.default_rng(2).normal(size=(35, 8))
    pos = np.asarray([(stoi[a], stoi[b]) for a, b in g.edges], dtype=np.int64)
    neg = negative_edges(row_ptr, cs, 1, len(pos), seed)
    pairs = np.concatenate([pos, neg])
    labels = np.concatenate([np.ones(len(pos), np.uint8), np.zeros(len(neg), np.uint8)])
    return table, pairs, labels
