"""Float64 numpy restatement of dw_node_softmax (include/dw_hip.h) and the test problems of the
node-classification tests: the sums, the magnitude sum |terms| behind every entry (the scale of
the tests' error bound), each sample's top-two logit gap, and sklearn's objective."""
from functools import lru_cache

import numpy as np


def valid(table, ids, labels, n_classes):
    return (ids >= 0) & (ids < table.shape[0]) & (labels >= 0) & (labels < n_classes)


def softmax_sums(table, ids, labels, coef, n_classes):
    """(sums [K (d + 1) + 2], magnitudes of the same shape, pred int32 [n], (smallest top-two
    logit gap, largest sum_j |w_kj x_j| + |b_k|)) of one pass over the float32 rows table[ids]
    at coef float64 [K, d + 1]. A sample whose id or label is out of range contributes nothing
    and has pred -1."""
    table = np.asarray(table, dtype=np.float32)
    ids, labels = np.asarray(ids, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    coef = np.asarray(coef, dtype=np.float64)
    K, d = int(n_classes), table.shape[1]
    assert coef.shape == (K, d + 1)
    ok = valid(table, ids, labels, K)
    X = table[ids[ok]].astype(np.float64)
    y = labels[ok]
    n = len(y)
    W, b = coef[:, :d], coef[:, d]
    Z = X @ W.T + b
    m = Z.max(axis=1)
    E = np.exp(Z - m[:, None])
    S = E.sum(axis=1)
    zy = Z[np.arange(n), y]
    loss = m + np.log(S) - zy
    R = E / S[:, None]
    R[np.arange(n), y] -= 1.0
    arg = Z.argmax(axis=1)
    G = np.concatenate([R.T @ X, R.sum(axis=0)[:, None]], axis=1)
    Gm = np.concatenate([np.abs(R).T @ np.abs(X), np.abs(R).sum(axis=0)[:, None]], axis=1)
    sums = np.concatenate([G.ravel(), [loss.sum(), float((arg == y).sum())]])
    mags = np.concatenate([Gm.ravel(), [(np.abs(m) + np.abs(np.log(S)) + np.abs(zy)).sum(), 0.0]])
    pred = np.full(len(ids), -1, dtype=np.int32)
    pred[ok] = arg
    top = np.sort(Z, axis=1)
    gap = float((top[:, -1] - top[:, -2]).min()) if n else np.inf
    scale = float((np.abs(X) @ np.abs(W).T + np.abs(b)).max()) if n else 0.0
    return sums, mags, pred, (gap, scale)


def loss_only(X, y, coef):
    """sum of the softmax losses of float64 features X at coef [K, d + 1]."""
    Z = X @ coef[:, :-1].T + coef[:, -1]
    m = Z.max(axis=1)
    return float((m + np.log(np.exp(Z - m[:, None]).sum(axis=1)) - Z[np.arange(len(y)), y]).sum())


def objective(X, y, coef_rows, C=1.0):
    """sklearn's objective C * sum(loss) + 0.5 * ||W||^2 at the free rows [K or 1, d + 1] (one
    row: the binary form, evaluated as the softmax over (0, z))."""
    rows = np.asarray(coef_rows, dtype=np.float64)
    full = np.concatenate([np.zeros((1, rows.shape[1])), rows]) if rows.shape[0] == 1 else rows
    return C * loss_only(X, y, full) + 0.5 * float(np.sum(rows[:, :-1] ** 2))


# (n, d, K): Gaussian clusters with float32-rounded features
PROBLEMS = {'k2': (34, 8, 2), 'k3': (300, 8, 3), 'k7': (1000, 16, 7), 'k40': (600, 128, 40)}


@lru_cache(maxsize=None)
def problem(name):
    """(table float32 [n + 1, d] with row 0 = <unk>, ids int64 [n] = 1 .. n, y int64 [n])."""
    n, d, K = PROBLEMS[name]
    rng = np.random.default_rng(100 + K)
    centres = rng.normal(size=(K, d)) * 1.5
    y = np.arange(n) % K
    rng.shuffle(y)
    x = centres[y] + rng.normal(size=(n, d))
    table = np.concatenate([np.zeros((1, d)), x]).astype(np.float32)
    table.setflags(write=False)
    ids = np.arange(1, n + 1, dtype=np.int64)
    ids.setflags(write=False)
    y.setflags(write=False)
    return table, ids, y


@lru_cache(maxsize=None)
def sklearn_fit(name):
    """(sklearn's LogisticRegression() fitted on the problem, its objective in float64)."""
    from sklearn.linear_model import LogisticRegression
    table, ids, y = problem(name)
    X = table[ids].astype(np.float64)
    clf = LogisticRegression().fit(X, y)
    rows = np.concatenate([clf.coef_, clf.intercept_[:, None]], axis=1)
    return clf, objective(X, y, rows)


def closure(name):
    """The restatement as a fit_closure closure over a problem."""
    table, ids, y = problem(name)
    K = PROBLEMS[name][2]
    return lambda coef: softmax_sums(table, ids, y, coef, K)[0]
