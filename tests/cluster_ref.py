"""Float64 numpy restatements of the clustering entry points (include/dw_hip.h: dw_kmeans_step,
dw_kmeans_seed, dw_partition_counts, dw_modularity_counts) and of the scores built on them, from
their definitions only: plain loops over clusters, samples and edges, no shared code with
shallow_encoders/graph/cluster.py. The uniforms come from oracle/philox.py."""
import math

import numpy as np

from oracle import philox

TAG_KMEANS = 0x4B4D0000


# ---- dw_kmeans_step ------------------------------------------------------------------------------
def step(table, ids, centroids, prev=None):
    """One Lloyd pass. Returns (labels int64 [n], out float64 [K (d + 1) + 2], mags (the sum of
    |terms| behind every float entry of out, 0 for the integer entries), margins float64 [n]:
    per valid sample (best-but-one score - best score) / sum |terms| of a score, inf for K = 1).
    A sample whose id is outside the table has label -1 and enters no sum."""
    table = np.asarray(table, dtype=np.float32)
    C = np.asarray(centroids, dtype=np.float64)
    V, d = table.shape
    K = C.shape[0]
    n = len(ids)
    ld = d + 1
    out = np.zeros(K * ld + 2)
    mags = np.zeros(K * ld + 2)
    labels = np.full(n, -1, dtype=np.int64)
    margins = np.full(n, np.inf)
    cnorm = np.array([sum(float(c) * float(c) for c in C[k]) for k in range(K)])
    counts = [0] * K
    changed = 0
    for i in range(n):
        v = int(ids[i])
        if 0 <= v < V:
            x = table[v].astype(np.float64)
            dots = C @ x
            s = cnorm - 2.0 * dots
            best = 0
            for k in range(1, K):
                if s[k] < s[best]:   # ties stay with the lowest k
                    best = k
            labels[i] = best
            if K > 1:
                scale = np.abs(C) @ np.abs(x)
                term = float(cnorm.max() + 2.0 * scale.max())
                others = np.delete(s, best)
                margins[i] = (float(others.min()) - float(s[best])) / max(term, 1e-300)
            out[best * ld:best * ld + d] += x
            mags[best * ld:best * ld + d] += np.abs(x)
            counts[best] += 1
            xx = float(x @ x)
            out[K * ld] += xx + float(s[best])
            mags[K * ld] += xx + float(cnorm[best]) + 2.0 * float(np.abs(C[best]) @ np.abs(x))
        if prev is None or int(prev[i]) != int(labels[i]):
            changed += 1
    for k in range(K):
        out[k * ld + d] = counts[k]
    out[K * ld + 1] = changed
    return labels, out, mags, margins


# ---- dw_kmeans_seed ------------------------------------------------------------------------------
def seed_uniform(seed, j):
    k0, k1 = seed & philox.MASK, (seed >> 32) & philox.MASK
    r = philox.philox(j, 0, 0, TAG_KMEANS, k0, k1)
    return philox.uniform53(int(r[0]), int(r[1]))


def seed_first(n, seed):
    return min(int(math.floor(seed_uniform(seed, 0) * n)), n - 1)


def seed_d2(X, chosen):
    """Squared distance of every row of X (float64) to the nearest of the rows X[chosen]."""
    d2 = np.full(len(X), np.inf)
    for c in chosen:
        diff = X - X[c]
        d2 = np.minimum(d2, (diff * diff).sum(axis=1))
    return d2


def seed_law(X, chosen):
    """The law of the next centre given the chosen ones: probability D2 / sum D2 per sample, or
    all mass on the lowest index not chosen when every D2 is zero."""
    d2 = seed_d2(X, chosen)
    total = d2.sum()
    p = np.zeros(len(X))
    if total > 0:
        return d2 / total
    p[min(i for i in range(len(X)) if i not in set(int(c) for c in chosen))] = 1.0
    return p


def seed_pick(X, chosen, seed, j):
    """Centre j by the header's rule with plain running sums: exact for data whose D2 are small
    integers (every order of summation gives the same doubles)."""
    d2 = seed_d2(X, chosen)
    total = float(d2.sum())
    if total == 0.0:
        return int(np.argmax(seed_law(X, chosen)))
    r = seed_uniform(seed, j) * total
    run = 0.0
    last = -1
    for i in range(len(X)):
        if d2[i] > 0.0:
            if run + d2[i] > r:
                return i
            last = i
        run += d2[i]
    return last


# ---- partitions ----------------------------------------------------------------------------------
def contingency(a, b, Ka, Kb):
    t = np.zeros((Ka, Kb), dtype=np.int64)
    for x, y in zip(a, b):
        if x >= 0 and y >= 0:
            t[int(x), int(y)] += 1
    return t


def nmi(a, b):
    """Mutual information over the arithmetic mean of the entropies, from the definitions."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    n = len(a)
    ca, cb, cab = {}, {}, {}
    for x, y in zip(a, b):
        ca[x] = ca.get(x, 0) + 1
        cb[y] = cb.get(y, 0) + 1
        cab[(x, y)] = cab.get((x, y), 0) + 1
    if len(ca) <= 1 and len(cb) <= 1:
        return 1.0
    mi = sum(c / n * math.log(c * n / (ca[x] * cb[y])) for (x, y), c in cab.items())
    ha = -sum(c / n * math.log(c / n) for c in ca.values())
    hb = -sum(c / n * math.log(c / n) for c in cb.values())
    return max(mi, 0.0) / max(0.5 * (ha + hb), np.finfo(float).eps)


def ari(a, b):
    """(RI - E[RI]) / (max RI - E[RI]) with pair counts n (n - 1) / 2, in exact rationals."""
    from fractions import Fraction
    a, b = [int(x) for x in a], [int(x) for x in b]
    n = len(a)
    ca, cb, cab = {}, {}, {}
    for x, y in zip(a, b):
        ca[x] = ca.get(x, 0) + 1
        cb[y] = cb.get(y, 0) + 1
        cab[(x, y)] = cab.get((x, y), 0) + 1

    def c2(m):
        return m * (m - 1) // 2
    index = sum(c2(c) for c in cab.values())
    sa, sb = sum(c2(c) for c in ca.values()), sum(c2(c) for c in cb.values())
    expected = Fraction(sa * sb, c2(n)) if n > 1 else Fraction(0)
    top = Fraction(sa + sb, 2)
    if top == expected:
        return 1.0
    return float((index - expected) / (top - expected))


def modularity_counts(row_ptr, col, labels, K):
    """int64 [K, 2]: per cluster the CSR entries inside it and its summed degree, a self-loop
    entry counting twice in both; rows of label -1 are skipped."""
    out = np.zeros((K, 2), dtype=np.int64)
    for u in range(len(row_ptr) - 1):
        lu = int(labels[u])
        if lu < 0:
            continue
        for e in range(int(row_ptr[u]), int(row_ptr[u + 1])):
            v = int(col[e])
            w = 2 if v == u else 1
            out[lu, 1] += w
            if int(labels[v]) == lu:
                out[lu, 0] += w
    return out
