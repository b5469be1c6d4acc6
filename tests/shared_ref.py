"""float64 numpy restatement of the shared-negatives SGNS step (TEST INFRASTRUCTURE).

The contract of dw_sgns_walks_shared (include/dw_hip.h): for walk w the
centres are positions i in [R, L - R) with h_i = w_in[walk[w, i]], the contexts walk[w, i + dl]
for dl in -R..-1, 1..R, and ALL centres of the walk take the S ids shared[w, :] as negatives,
each weighted lambda = 2R K / S:

    acc[0] = sum_i sum_ctx -log max(sigmoid(h_i . o_ctx), 1e-6)      acc[2] = #(sigmoid >= .5)
    acc[1] = lambda sum_i sum_s -log max(sigmoid(-h_i . o_s), 1e-6)  acc[3] = lambda #(sigmoid(h_i . o_s) >= .5)

and the gradients are the closed form of (acc[0] + acc[1]) * scale with the reference's clamp
mask per term (no gradient where the clamped sigmoid is below 1e-6). Every occurrence of an id
is its own term. Ids outside [0, V) drop their terms (a bad centre its row, a bad context or
shared id its column), as the kernels do under DW_S_BAD_INDEX.
"""
import math

import numpy as np

CLAMP_LOGIT = math.log(1e6)   # sigmoid(-x) = 1e-6 at x = ln(1e6 - 1): within 1e-6 of this


def _sig(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


def shared_ref(walks, shared_ids, w_in, w_out, R, K, scale=None):
    """Returns a dict: ``acc`` float64[4], ``g_in`` / ``g_out`` float64 (V, d), ``counts``
    (the raw positive / negative hit counts, before lambda), ``lam``, ``min_abs_logit`` (over
    the counted terms) and ``clamp_dist`` (the smallest distance of a counted logit from the
    clamp boundary: -ln 1e6 for a positive term, +ln 1e6 for a negative one), ``pos_logits`` /
    ``neg_logits`` (all counted logits) and ``bad`` (an id was out of range)."""
    walks = np.asarray(walks, dtype=np.int64)
    n, L = walks.shape
    ids = np.asarray(shared_ids, dtype=np.int64).reshape(n, -1)
    S = ids.shape[1]
    w_in = np.asarray(w_in, dtype=np.float64)
    w_out = np.asarray(w_out, dtype=np.float64)
    V = w_in.shape[0]
    nc = L - 2 * R
    lam = 2 * R * K / S
    if scale is None:
        scale = 1.0 / max(n * nc * 2 * R, 1)
    pos = np.arange(R, L - R)                                  # centre positions
    dl = np.arange(L)[None, :] - pos[:, None]
    band = (dl != 0) & (np.abs(dl) <= R)                       # [nc, L]: context of centre?
    acc = np.zeros(4)
    counts = np.zeros(2)
    g_in = np.zeros_like(w_in)
    g_out = np.zeros_like(w_out)
    min_abs, clamp_dist, bad = np.inf, np.inf, False
    pos_logits, neg_logits = [], []
    for w in range(n):
        wk, sh = walks[w], ids[w]
        ok_w = (wk >= 0) & (wk < V)
        ok_s = (sh >= 0) & (sh < V)
        bad = bad or not (ok_w.all() and ok_s.all())
        wk0, sh0 = np.where(ok_w, wk, 0), np.where(ok_s, sh, 0)
        h = w_in[wk0[pos]]
        o_w, o_s = w_out[wk0], w_out[sh0]
        m_p = band & ok_w[pos][:, None] & ok_w[None, :]        # counted positive terms
        m_n = ok_w[pos][:, None] & ok_s[None, :]               # counted negative terms
        x_p, x_n = h @ o_w.T, h @ o_s.T
        s_p, s_n = _sig(x_p), _sig(-x_n)
        acc[0] += (-np.log(np.maximum(s_p, 1e-6)))[m_p].sum()
        acc[1] += lam * (-np.log(np.maximum(s_n, 1e-6)))[m_n].sum()
        counts[0] += (s_p >= 0.5)[m_p].sum()
        counts[1] += (_sig(x_n) >= 0.5)[m_n].sum()
        c_p = np.where(m_p & (s_p >= 1e-6), s_p - 1.0, 0.0) * scale
        c_n = np.where(m_n & (s_n >= 1e-6), 1.0 - s_n, 0.0) * (lam * scale)
        np.add.at(g_in, wk0[pos], c_p @ o_w + c_n @ o_s)
        np.add.at(g_out, wk0, c_p.T @ h)
        np.add.at(g_out, sh0, c_n.T @ h)
        lp, ln = x_p[m_p], x_n[m_n]
        pos_logits.append(lp)
        neg_logits.append(ln)
        for v in (lp, ln):
            if v.size:
                min_abs = min(min_abs, float(np.abs(v).min()))
        if lp.size:
            clamp_dist = min(clamp_dist, float(np.abs(lp + CLAMP_LOGIT).min()))
        if ln.size:
            clamp_dist = min(clamp_dist, float(np.abs(ln - CLAMP_LOGIT).min()))
    acc[2] = counts[0]
    acc[3] = lam * counts[1]
    return {'acc': acc, 'g_in': g_in, 'g_out': g_out, 'counts': counts, 'lam': lam,
            'min_abs_logit': min_abs, 'clamp_dist': clamp_dist,
            'pos_logits': np.concatenate(pos_logits) if n else np.zeros(0),
            'neg_logits': np.concatenate(neg_logits) if n else np.zeros(0), 'bad': bad}


def repeated_noise(walks, shared_ids, R, K):
    """int64 [B', 2R, K]: each walk's S = 2R K shared ids reshaped for every one of its centres —
    the per-pair tensor under which the reference's step (and dw_sgns_walks) computes what the
    shared step computes at lambda = 1."""
    walks = np.asarray(walks)
    n, L = walks.shape
    ids = np.asarray(shared_ids, dtype=np.int64).reshape(n, -1)
    assert ids.shape[1] == 2 * R * K, 'lambda = 1 needs S = 2R K'
    nc = L - 2 * R
    return np.repeat(ids.reshape(n, 1, 2 * R, K), nc, axis=1).reshape(n * nc, 2 * R, K)
