"""Float64 numpy restatement of dw_node_ovr (include/dw_hip.h) and the multi-label problems of
the one-vs-rest tests: the sums, the magnitude sum |terms| behind every entry (the scale of the
tests' error bound), the predictions under both rules with their decision margins, the top-k rule
on a score matrix, and sklearn's per-class objectives."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

THRESHOLD, TOP_K = 0, 1

# sums / pred / margin: per rule; mags: of the float entries (0 at the counts); scale: the largest
# sum_j |w_cj x_j| + |b_c|, what a margin is relative to; floats: the K (d + 1) + 1 entries before
# the 3 K counts
Pass = namedtuple('Pass', 'sums mags pred margin scale floats')


def _u64(masks):
    m = np.asarray(masks)
    return np.ascontiguousarray(m if m.dtype == np.uint64 else m.astype(np.int64)).view(np.uint64)


def bits(masks, n_classes):
    """bool [n, K] of uint64 bit patterns held in an int64 / uint64 array."""
    m = _u64(masks)
    return ((m[:, None] >> np.arange(n_classes, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def to_masks(Y):
    """int64 [n] bit patterns of a bool [n, K] matrix."""
    out = np.zeros(len(Y), dtype=np.uint64)
    for c in range(Y.shape[1]):
        out |= np.asarray(Y[:, c], dtype=np.uint64) << np.uint64(c)
    return out.view(np.int64)


def valid(table, ids, masks, n_classes):
    m = _u64(masks)
    high = np.zeros(len(m), dtype=bool) if n_classes >= 64 else (m >> np.uint64(n_classes)) != 0
    return (ids >= 0) & (ids < table.shape[0]) & ~high


def top_k(Z, k):
    """bool [n, K]: per row the k[i] highest scores, ties to the lowest column."""
    order = np.argsort(-Z, axis=1, kind='stable')
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(Z.shape[1])[None, :], axis=1)
    return rank < np.asarray(k)[:, None]


def ovr_sums(table, ids, masks, coef, n_classes):
    """One pass over the float32 rows table[ids] at coef float64 [K, d + 1]: a Pass whose sums
    are [K (d + 1) + 1 + 3 K] per rule (gradient rows, loss, tp[K], predicted[K], true[K]). A
    sample whose id is out of range or whose mask has a bit at or above K contributes nothing
    and has pred 0. margin[THRESHOLD]: the smallest |z|; margin[TOP_K]: the smallest gap between
    a sample's k-th and (k + 1)-th logit (0 < k < K)."""
    table = np.asarray(table, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    coef = np.asarray(coef, dtype=np.float64)
    K, d = int(n_classes), table.shape[1]
    assert coef.shape == (K, d + 1)
    ok = valid(table, ids, masks, K)
    X = table[ids[ok]].astype(np.float64)
    Y = bits(np.asarray(masks)[ok], K)
    W, b = coef[:, :d], coef[:, d]
    Z = X @ W.T + b
    e = np.exp(-np.abs(Z))
    hi, lo = 1.0 / (1.0 + e), e / (1.0 + e)
    R = np.where(Y, -np.where(Z >= 0, lo, hi), np.where(Z >= 0, hi, lo))   # sigmoid(z) - y
    pos, yz, soft = np.maximum(Z, 0.0), np.where(Y, Z, 0.0), np.log1p(e)
    loss = float((pos - yz + soft).sum())
    G = np.concatenate([R.T @ X, R.sum(axis=0)[:, None]], axis=1)
    Gm = np.concatenate([np.abs(R).T @ np.abs(X), np.abs(R).sum(axis=0)[:, None]], axis=1)
    k = Y.sum(axis=1)
    P = {THRESHOLD: Z > 0, TOP_K: top_k(Z, k)}
    sums, pred = {}, {}
    for rule, p in P.items():
        counts = np.concatenate([(p & Y).sum(axis=0), p.sum(axis=0), Y.sum(axis=0)])
        sums[rule] = np.concatenate([G.ravel(), [loss], counts.astype(np.float64)])
        full = np.zeros(len(ids), dtype=np.int64)
        full[ok] = to_masks(p)
        pred[rule] = full
    mags = np.concatenate([Gm.ravel(), [float((pos + np.abs(yz) + soft).sum())], np.zeros(3 * K)])
    top = -np.sort(-Z, axis=1)
    mid = (k > 0) & (k < K)
    rows = np.flatnonzero(mid)
    gaps = top[rows, k[mid] - 1] - top[rows, k[mid]]
    margin = {THRESHOLD: float(np.abs(Z).min()) if Z.size else np.inf,
              TOP_K: float(gaps.min()) if len(gaps) else np.inf}
    scale = float((np.abs(X) @ np.abs(W).T + np.abs(b)).max()) if len(X) else 0.0
    return Pass(sums, mags, pred, margin, scale, K * (d + 1) + 1)


def class_objectives(X, Y, rows, C=1.0):
    """[K]: per class sklearn's binary objective C * sum(loss) + 0.5 * ||w_c||^2 at the rows
    [K, d + 1] on float64 features X and the bool indicator matrix Y."""
    rows = np.asarray(rows, dtype=np.float64)
    Z = X @ rows[:, :-1].T + rows[:, -1]
    loss = np.maximum(Z, 0.0) - np.where(Y, Z, 0.0) + np.log1p(np.exp(-np.abs(Z)))
    return C * loss.sum(axis=0) + 0.5 * (rows[:, :-1] ** 2).sum(axis=1)


# (n, d, K): every node carries 1-3 labels; its features are the sum of its labels' centres plus
# unit Gaussian noise, rounded to float32. The centres are N(0, 0.5^2) per coordinate, a third of
# the single-label problems' distance (nodeclf_ref.py): the labels of the benchmark graphs are
# far from linearly separable from an embedding (published micro-F1 on BlogCatalog: 0.2-0.4), and
# so are these. On nearly separable labels (centres at 1.0 and above with d = 16, K = 7) the
# joint fit spends its max_iter = 100 before every class has converged and ends up to 5.6e-3
# above sklearn, whose max_iter counts per class: such a fit wants a larger max_iter.
PROBLEMS = {'m3': (300, 8, 3), 'm7': (1000, 16, 7), 'm40': (600, 128, 40)}


@lru_cache(maxsize=None)
def problem(name):
    """(table float32 [n + 1, d] with row 0 = <unk>, ids int64 [n] = 1 .. n, masks int64 [n])."""
    n, d, K = PROBLEMS[name]
    rng = np.random.default_rng(200 + K)
    centres = rng.normal(size=(K, d)) * 0.5
    Y = np.zeros((n, K), dtype=bool)
    for i in range(n):
        Y[i, rng.choice(K, size=rng.integers(1, min(3, K) + 1), replace=False)] = True
    x = Y.astype(np.float64) @ centres + rng.normal(size=(n, d))
    table = np.concatenate([np.zeros((1, d)), x]).astype(np.float32)
    ids = np.arange(1, n + 1, dtype=np.int64)
    masks = to_masks(Y)
    for a in (table, ids, masks):
        a.setflags(write=False)
    return table, ids, masks


@lru_cache(maxsize=None)
def sklearn_fit(name):
    """(OneVsRestClassifier(LogisticRegression()) fitted on the problem, its rows [K, d + 1],
    its per-class objectives in float64)."""
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    table, ids, masks = problem(name)
    K = PROBLEMS[name][2]
    X, Y = table[ids].astype(np.float64), bits(masks, K)
    clf = OneVsRestClassifier(LogisticRegression()).fit(X, Y.astype(np.int64))
    rows = np.stack([np.concatenate([e.coef_[0], e.intercept_]) for e in clf.estimators_])
    return clf, rows, class_objectives(X, Y, rows)


def closure(name):
    """The restatement as a fit_closure closure over a problem."""
    table, ids, masks = problem(name)
    K = PROBLEMS[name][2]
    return lambda coef: ovr_sums(table, ids, masks, coef, K).sums[THRESHOLD]
