"""The weighted walk kernels at hub rows and zero weights, against plain references.

Graph: weighted_ref.hub_graph() — a 2,500-neighbour hub (past REPLAY_CH = REPLAY_NCAP = 2048, a
209-bucket adjacency-hash row), eight rows of ~310 neighbours (several passes of the wave over
the LDS weight cache, a large part of the N(prev) stage), 1,344 rows of 9..64 (hashed rows) and
3,548 of at most 8 — with the weight families of weighted_ref.sym_weights.

  a. dw_alias_build: bit for bit the oracle's tables (oracle/philox.alias_tables), and,
     independently of the oracle, within the tables' own truncation of the weights' law.
  b. the Philox walkers (first_order_pick over prob_thr / alias in k_walk_deepwalk*, and in the
     16-, 8- and 4-lane k_walk_node2vec_fast with and without the adjacency hash; the counted
     launch with 12-byte picks): bit for bit oracle/philox.fast_walks.
  c. the weighted replay (k_walk_replay<2048, 2048>, fast = 0: the LDS branch in one and in
     several passes, the hub branch's three lane-0 passes, N(prev) staged in LDS and searched in
     HBM): bit for bit oracle/walk_ref.walks_replay, uniforms 0, 1 - 2^-53 and 0.5 included.
  d. the law, against the reference's rule (walk_ref on the weighted CSR) and not the product's
     own oracle: chi-square tests, family-wise alpha = 1e-3 over the N_LAW_TESTS tests (each
     passes when its p-value > 1e-3 / N_LAW_TESTS). Seeds are fixed and by (b) the device's walks
     are the oracle's, so each p-value was computed on the CPU from the oracle before any GPU
     run; they are recorded in the tests' docstrings.
  e. the status paths: a row of zero weights (ZeroDivisionError from the alias build, from the
     replay's LDS branch and from its hub branch), a negative weight (ValueError from the alias
     build), an infinite weight (the limit law: every step takes that edge).
"""
import numpy as np
import pytest
import torch

from oracle import philox as ph
from oracle import walk_ref

from shallow_encoders.graph.csr import CSRGraph
from shallow_encoders.graph.random_walk_generator import DeepWalk, Node2Vec

import weighted_ref as wr
from test_gpu_walk_law import _bins, _chi2_p

pytestmark = pytest.mark.gpu

P, Q = 0.25, 4.0
SEED = 77
L_FAST = 8
HUB, MIDS = wr.HUB_ID, np.array(wr.MID_IDS)
N_LAW_TESTS = 3
ALPHA = 1e-3 / N_LAW_TESTS

_C = {}


def _memo(key, make):
    if key not in _C:
        _C[key] = make()
    return _C[key]


def _weighted(weights):
    base = wr.hub_graph()
    return CSRGraph.from_arrays(base.row_ptr, base.col, weights, itos=base.itos)


def _graph(family):
    """(the weighted CSRGraph — one per family, so its device tensors are built once —, its
    weights)."""
    def make():
        w = wr.sym_weights(wr.hub_graph(), family)
        return _weighted(w), w
    return _memo(('graph', family), make)


def _tables(family):
    csr, w = _graph(family)
    return _memo(('tables', family), lambda: ph.alias_tables(csr.row_ptr, w))


def _degree_class():
    """Per vocabulary id: 0 (degree <= 8), 1 (9..64), 2 (65..2048), 3 (> 2048)."""
    return np.digitize(wr.hub_graph().degree(), [9, 65, 2049])


def _spread(cand, k):
    return cand[np.linspace(0, len(cand) - 1, k).astype(np.int64)]


def _node_kinds():
    deg = wr.hub_graph().degree()
    ids = np.arange(len(deg))
    leaf = (ids > MIDS[-1]) & (ids <= wr.N_LEAVES + 1)
    return {'low': ids[leaf & (deg <= 8)], 'mid_leaf': ids[leaf & (deg > 8)],
            'pendant': ids[ids > wr.N_LEAVES + 1]}


def _fast_starts():
    """256 starts: the hub 64 times, each of the eight ~310-neighbour nodes 8 times, 32 leaves
    of degree <= 8, 64 of degree 9..64, 32 pendant nodes."""
    k = _node_kinds()
    return np.concatenate([np.full(64, HUB), np.repeat(MIDS, 8), _spread(k['low'], 32),
                           _spread(k['mid_leaf'], 64), _spread(k['pendant'], 32)]).astype(np.int32)


def _fast_expected(family, method):
    def make():
        csr, _ = _graph(family)
        prob, alias = _tables(family)
        return ph.fast_walks(csr.row_ptr, csr.col, _fast_starts(), L_FAST, method, P, Q,
                             seed=SEED, walk_id0=0, prob_thr=prob, alias=alias)
    return _memo(('fast', family, method), make)


def _edge_weight(csr, w, u, x):
    """The weights of the directed edges u[i] -> x[i] (every one must exist)."""
    rp = np.asarray(csr.row_ptr, dtype=np.int64)
    V = csr.vocab_size
    row = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    key = row * V + np.asarray(csr.col, dtype=np.int64)
    order = np.argsort(key)
    want = np.asarray(u, dtype=np.int64) * V + np.asarray(x, dtype=np.int64)
    at = np.searchsorted(key[order], want)
    assert (key[order][np.minimum(at, len(key) - 1)] == want).all(), 'a step is not an edge'
    return w[order][at]


def _walker(csr, method, L, layout, **kw):
    p, q = kw.pop('p', P), kw.pop('q', Q)
    if method == 'node2vec':
        return Node2Vec(csr, L, p=p, q=q, layout=layout, **kw)
    return DeepWalk(csr, L, layout=layout, **kw)


# ---- a. alias tables ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', wr.FAMILIES)
def test_alias_tables_bit_exact_and_represent_the_weights(family, hip_device):
    csr, w = _graph(family)
    prob, alias = _tables(family)
    d = csr.device_tensors(hip_device, need_alias=True)
    got_prob = d['prob_thr'].cpu().numpy().view(np.uint32)
    got_alias = d['alias'].cpu().numpy()
    np.testing.assert_array_equal(got_prob, prob)
    np.testing.assert_array_equal(got_alias, alias)
    worst, zero_mass = wr.alias_mass_error(csr.row_ptr, got_prob, got_alias, w)
    print(f'{family}: worst mass error / bound {worst:.4f}, zero entries with mass {zero_mass}')
    assert worst <= 1.0
    assert zero_mass == 0


# ---- b. Philox walkers -------------------------------------------------------------------------
def test_fast_expected_walks_cover_every_degree_class():
    """The oracle's walks from _fast_starts put every degree class both at v (the row a step
    leaves) and at prev, in every family; 'zeros': no step crosses a zero-weight edge."""
    cls = _degree_class()
    for family in ('int', 'skew', 'zeros', 'float'):
        csr, w = _graph(family)
        for method in ('deepwalk', 'node2vec'):
            exp = _fast_expected(family, method)
            assert (exp > 0).all()
            assert set(cls[exp[:, 1:-1]].ravel()) == {0, 1, 2, 3}, (family, method)   # v
            assert set(cls[exp[:, :-2]].ravel()) == {0, 1, 2, 3}, (family, method)    # prev
            # the 5-step prefixes the shorter launches are compared with
            assert set(cls[exp[:, 1:4]].ravel()) == {0, 1, 2, 3}, (family, method)
            ew = _edge_weight(csr, w, exp[:, :-1].ravel(), exp[:, 1:].ravel())
            assert (ew > 0).all(), (family, method)
    _, z = _graph('zeros')
    assert (z == 0).mean() > 0.08


@pytest.mark.parametrize('L', [8, 5])
@pytest.mark.parametrize('method,layout,kernel', [
    ('deepwalk', 'indexed', 'dw_walk_fast_indexed'), ('deepwalk', 'csr', 'dw_walk_fast'),
    ('node2vec', 'indexed', 'dw_walk_fast_indexed'), ('node2vec', 'hash', 'dw_walk_fast_indexed'),
    ('node2vec', 'csr', 'dw_walk_fast')])
@pytest.mark.parametrize('family', ['int', 'skew', 'zeros', 'float'])
def test_weighted_fast_walkers_bit_exact_vs_philox_oracle(family, method, layout, kernel, L,
                                                           hip_device):
    """A walk is a function of its walk id and the step, so the walks of length 5 are the
    prefixes of the walks of length 8 (the inline walker's packed stores: L % 4 == 0 and not).
    A weighted graph never walks over the position index."""
    csr, _ = _graph(family)
    w = _walker(csr, method, L, layout, rng='philox', seed=SEED, device=hip_device)
    got = w.walk_batch(torch.as_tensor(_fast_starts()), walk_id0=0).cpu().numpy()
    assert w.last_walker == kernel
    assert csr.device_tensors(hip_device).get('n2v_rec') is None
    np.testing.assert_array_equal(got, _fast_expected(family, method)[:, :L])


@pytest.mark.parametrize('family', ['zeros', 'skew'])
def test_weighted_node2vec_lane_groups_and_counted_launch(family, hip_device):
    """A batch of 300,000 walks takes the 4-lane walker, 40,000 the 8- (or 16-)lane one, 4,096
    the 16-lane one: the same walks, the plain-CSR layout's too, and the oracle's for the first
    256. The counted launch (dw_walk_fast_counted, 12 bytes per proposal: col, prob_thr, alias)
    returns the walks of walk_batch at the 16- and the 4-lane size."""
    csr, _ = _graph(family)
    L = 5
    n_big = 300_000
    starts = (np.arange(n_big, dtype=np.int64) % (csr.vocab_size - 1) + 1).astype(np.int32)
    starts[:256] = _fast_starts()
    starts = torch.as_tensor(starts).to(hip_device)

    def make(layout):
        return Node2Vec(csr, L, p=P, q=Q, rng='philox', seed=SEED, layout=layout,
                        device=hip_device)
    w = make('hash')
    big = w.walk_batch(starts, walk_id0=0)
    assert w.last_walker == 'dw_walk_fast_indexed'
    assert torch.equal(w.walk_batch(starts[:40_000], walk_id0=0), big[:40_000])
    assert torch.equal(w.walk_batch(starts[:4096], walk_id0=0), big[:4096])
    assert torch.equal(make('csr').walk_batch(starts[:4096], walk_id0=0), big[:4096])
    np.testing.assert_array_equal(big[:256].cpu().numpy(),
                                  _fast_expected(family, 'node2vec')[:, :L])
    assert (big > 0).all()
    for n in (256, n_big):
        out = torch.empty((n, L), dtype=torch.int32, device=hip_device)
        c = make('indexed').count_traffic(starts[:n], walk_id0=0, out=out)
        assert torch.equal(out, big[:n])
        assert c['steps'] == n * (L - 1)
        # per step 32 B of row_ptr / adj_off and a 4-B store; per proposal block at least 4
        # proposals of 12 B (col, prob_thr, alias): 4 B each would be the unweighted count
        assert c['blocks'] >= c['steps'] - n
        assert c['bytes'] >= c['steps'] * 36 + c['blocks'] * 48


# ---- c. the weighted replay --------------------------------------------------------------------
REPLAY_L = 12
ONE_MINUS = 1.0 - 2.0 ** -53


def _replay_starts_and_uniforms():
    """64 starts — the hub 16 times, the eight ~310-neighbour nodes twice each, 8 leaves whose
    row STARTS with a zero weight in the 'zeros' family, 8 whose row ENDS with one, 8 other
    leaves, 8 pendant nodes — and uniforms from default_rng(1) with a few entries per walk
    overwritten by 0.0, 1 - 2^-53 and 0.5: the first draw of the zero-first rows is 0.0, of the
    zero-last rows 1 - 2^-53 (bisect_right's clamp to n - 1), of three hub starts one of each."""
    def make():
        base = wr.hub_graph()
        rp = np.asarray(base.row_ptr)
        z = wr.sym_weights(base, 'zeros')
        k = _node_kinds()
        leaves = np.concatenate([k['low'], k['mid_leaf']])
        leaves = leaves[base.degree()[leaves] >= 3]
        zero_first = leaves[z[rp[leaves]] == 0]
        zero_last = leaves[z[rp[leaves + 1] - 1] == 0]
        starts = np.concatenate([np.full(16, HUB), np.repeat(MIDS, 2), _spread(zero_first, 8),
                                 _spread(zero_last, 8), _spread(k['mid_leaf'], 8),
                                 _spread(k['pendant'], 8)]).astype(np.int32)
        u = np.random.default_rng(1).random((len(starts), REPLAY_L - 1))
        special = (0.0, ONE_MINUS, 0.5)
        for w in range(len(starts)):
            u[w, 1 + w % (REPLAY_L - 2)] = special[w % 3]
            u[w, 1 + (w + 5) % (REPLAY_L - 2)] = special[(w + 1) % 3]
        u[0:3, 0] = special
        u[32:40, 0] = 0.0
        u[40:48, 0] = ONE_MINUS
        return starts, u
    return _memo('replay_inputs', make)


@pytest.mark.parametrize('method,p,q', [('deepwalk', 1.0, 1.0), ('node2vec', 0.25, 4.0),
                                        ('node2vec', 2.0, 0.5)])
@pytest.mark.parametrize('family', ['int', 'dyadic', 'zeros'])
def test_weighted_replay_bit_exact_vs_reference_rule(family, method, p, q, hip_device):
    csr, w = _graph(family)
    starts, u = _replay_starts_and_uniforms()
    exp = walk_ref.walks_replay(walk_ref.CSR(csr.row_ptr, csr.col, w), starts, REPLAY_L, method,
                                p, q, u)
    # the walks take the branches under test
    assert int((exp[:, :-1] == HUB).sum()) >= 16          # rows of n > 2048: lane 0's three passes
    assert int(np.isin(exp[:, :-1], MIDS).sum()) >= 16    # 64 < n <= 2048: the LDS branch in passes
    assert int((exp[:, :-2] == HUB).sum()) >= 16          # N(prev) past NCAP: searched in HBM
    assert int(np.isin(exp[:, :-2], MIDS).sum()) >= 16    # N(prev) fills ~300 of the LDS stage
    if family == 'zeros':   # a zero weight first (draw 0.0) and last (draw 1 - 2^-53) in the row
        rp = np.asarray(csr.row_ptr)
        assert (w[rp[starts[32:40]]] == 0).all() and (w[rp[starts[40:48] + 1] - 1] == 0).all()
    wk = _walker(csr, method, REPLAY_L, 'indexed', p=p, q=q, device=hip_device)
    got = wk.walk_batch(torch.as_tensor(starts), uniforms=u).cpu().numpy()
    assert wk.last_walker == 'dw_walk_replay'
    np.testing.assert_array_equal(got, exp)


# ---- d. the law --------------------------------------------------------------------------------
def _ref_graph():
    csr, w = _graph('int')
    return _memo('ref_int', lambda: walk_ref.CSR(csr.row_ptr, csr.col, w))


def deepwalk_hub_pvalue(x):
    """Chi-square of the hub's successors x against w / sum w over all 2,500 neighbours."""
    ref = _ref_graph()
    nbrs = np.array(ref.neighbors(HUB))
    wt = np.array(ref.unnormalized_weights(HUB))
    order = np.argsort(nbrs)
    idx = np.searchsorted(nbrs[order], x)
    assert (nbrs[order][np.minimum(idx, len(nbrs) - 1)] == x).all(), 'a step left N(hub)'
    counts = np.bincount(idx, minlength=len(nbrs))
    expected = wt[order] / wt.sum() * len(x)
    assert expected.min() >= 5
    return _chi2_p(counts, expected)


def second_order_pvalue(t, v, x):
    """Chi-square of the samples x of P(. | prev = t, v) against walk_ref.node2vec_transition,
    binned as tests/test_gpu_walk_law.py bins (x == t, common neighbours, the rest)."""
    ref = _ref_graph()
    law = walk_ref.node2vec_transition(ref, t, v, P, Q)
    assert set(np.unique(x).tolist()) <= set(law), 'a step left N(v)'
    bins = _bins(law, t, v, ref, len(x))
    counts = [np.isin(x, b).sum() for b in bins]
    expected = [sum(law[int(y)] for y in b) * len(x) for b in bins]
    return _chi2_p(counts, expected) + (len(bins),)


def law_pairs():
    """(t, v, walks launched) of the two second-order tests: a leaf of degree 9..64 -> the hub,
    and the hub -> the ~310-neighbour node its heaviest such edge leads to (the first of them).
    The walk counts give about 3,000 samples of x (at least 2,000 asserted)."""
    ref = _ref_graph()
    leaf = int(_node_kinds()['mid_leaf'][0])
    wt = dict(zip(ref.neighbors(HUB), ref.unnormalized_weights(HUB)))
    mid = int(max(MIDS, key=lambda m: (wt[int(m)], -int(m))))
    return {'leaf-hub': (leaf, HUB, 128_000), 'hub-mid': (HUB, mid, 5_000_000)}


def test_weighted_deepwalk_law_on_hub_vs_reference_rule(hip_device):
    """40 * 2,500 walks of length 2 from the hub, seed 9: the successors against w / sum w.
    From the oracle, before any GPU run: chi2 2534.0 over 2,500 neighbours, p-value 0.308."""
    csr, _ = _graph('int')
    n = 40 * wr.N_LEAVES
    starts = torch.full((n,), HUB, dtype=torch.int32, device=hip_device)
    big = DeepWalk(csr, 2, rng='philox', seed=9, device=hip_device).walk_batch(starts, walk_id0=0)
    plain = DeepWalk(csr, 2, rng='philox', seed=9, layout='csr', device=hip_device).walk_batch(
        starts[:4096], walk_id0=0)
    assert torch.equal(plain, big[:4096])
    pv, stat = deepwalk_hub_pvalue(big[:, 1].cpu().numpy())
    print(f'weighted DeepWalk from the hub: {n} walks, chi2 {stat:.1f}, p-value {pv:.3g}')
    assert pv > ALPHA, f'p-value {pv:.3g} <= {ALPHA:.2g}'


@pytest.mark.parametrize('kind', ['leaf-hub', 'hub-mid'])
def test_weighted_node2vec_second_order_law_vs_reference_rule(kind, hip_device):
    """Walks of length 3 from t, seed 2024, the rejection walker (layout 'hash'; the first 4,096
    walks also on 'csr' and in a 16-lane batch): the walks whose first step is v sample
    P(x | t, v), the reference's rule with weights (w * 1/p at x == t, w * 1/q at x in N(t)).
    From the oracle, before any GPU run:
      leaf-hub (t = 10, deg 13; v = the hub): 128,000 walks, 3,039 samples, 10 bins,
                chi2 12.9, p-value 0.166;
      hub-mid  (t = the hub; v = 2, deg 310): 5,000,000 walks, 3,476 samples, 13 bins,
                chi2 15.7, p-value 0.207."""
    csr, _ = _graph('int')
    t, v, n = law_pairs()[kind]
    starts = torch.full((n,), t, dtype=torch.int32, device=hip_device)

    def make(layout):
        return Node2Vec(csr, 3, p=P, q=Q, rng='philox', seed=2024, layout=layout,
                        device=hip_device)
    out = make('hash').walk_batch(starts, walk_id0=0)
    assert torch.equal(make('hash').walk_batch(starts[:4096], walk_id0=0), out[:4096])
    assert torch.equal(make('csr').walk_batch(starts[:4096], walk_id0=0), out[:4096])
    x = out[out[:, 1] == v][:, 2].cpu().numpy()
    pv, stat, n_bins = second_order_pvalue(t, v, x)
    print(f'{kind} (t={t}, v={v}): {n} walks, {len(x)} samples, {n_bins} bins, chi2 {stat:.1f}, '
          f'p-value {pv:.3g}')
    assert n <= 8_000_000 and len(x) >= 2000
    assert pv > ALPHA, f'p-value {pv:.3g} <= {ALPHA:.2g}'


# ---- e. status paths ---------------------------------------------------------------------------
def _zero_row_graph(which):
    """The 'int' family with every edge of one node at weight 0 (both directions): a leaf of
    degree 9..64 (one pass of the LDS branch), a ~310-neighbour node (several passes) or the hub
    (n > 2048: lane 0's hub branch). Returns (graph, weights, the node)."""
    base = wr.hub_graph()
    z = {'leaf': int(_node_kinds()['mid_leaf'][3]), 'mid': int(MIDS[2]), 'hub': HUB}[which]
    w = wr.sym_weights(base, 'int')
    row = np.repeat(np.arange(base.vocab_size), base.degree())
    w[(row == z) | (np.asarray(base.col) == z)] = 0.0
    return _weighted(w), w, z


@pytest.mark.parametrize('which', ['leaf', 'mid', 'hub'])
def test_zero_weight_row_raises_zero_division(which, hip_device):
    csr, w, z = _zero_row_graph(which)
    k = _node_kinds()
    away = np.concatenate([_spread(k['mid_leaf'], 24), _spread(k['low'], 8),
                           MIDS[[0, 1, 5, 7]]]).astype(np.int32)
    away = away[away != z]
    # Philox: the alias build refuses the graph, and keeps no table
    for make in (lambda: DeepWalk(csr, 4, rng='philox', device=hip_device),
                 lambda: Node2Vec(csr, 4, p=P, q=Q, rng='philox', layout='hash',
                                  device=hip_device)):
        for _ in range(2):   # (the refusal is not forgotten at the second call)
            with pytest.raises(ZeroDivisionError):
                make().walk_batch(torch.as_tensor(away), walk_id0=0)
            assert 'prob_thr' not in csr._dev and 'alias' not in csr._dev
    # replay: a batch that reaches the row raises; one that never does equals the oracle
    L = 6
    rng = np.random.default_rng(2)
    ref = walk_ref.CSR(csr.row_ptr, csr.col, w)
    for method, p, q in (('deepwalk', 1.0, 1.0), ('node2vec', 0.25, 4.0)):
        wk = _walker(csr, method, L, 'indexed', p=p, q=q, device=hip_device)
        reach = np.concatenate([away[:7], [z]]).astype(np.int32)
        with pytest.raises(ZeroDivisionError):
            wk.walk_batch(torch.as_tensor(reach), uniforms=rng.random((len(reach), L - 1)))
        assert wk.last_walker == 'dw_walk_replay'
        with pytest.raises(ZeroDivisionError):
            walk_ref.walks_replay(ref, reach, L, method, p, q, rng.random((len(reach), L - 1)))
        u = rng.random((len(away), L - 1))
        exp = walk_ref.walks_replay(ref, away, L, method, p, q, u)
        assert not (exp == z).any()
        got = wk.walk_batch(torch.as_tensor(away), uniforms=u).cpu().numpy()
        np.testing.assert_array_equal(got, exp)


def _chord(base):
    """A chord between two leaves of degree >= 3: (u, v, the edge u -> v, the edge v -> u)."""
    rp, col = np.asarray(base.row_ptr), np.asarray(base.col)
    u = int(_node_kinds()['mid_leaf'][5])
    e_uv = int(rp[u]) + int(np.flatnonzero(col[rp[u]:rp[u + 1]] != HUB)[0])
    v = int(col[e_uv])
    e_vu = int(rp[v]) + int(np.flatnonzero(col[rp[v]:rp[v + 1]] == u)[0])
    assert base.degree()[v] >= 3
    return u, v, e_uv, e_vu


def test_negative_weight_is_refused_by_the_alias_build(hip_device):
    """One edge of weight -1 in rows whose sums stay positive: no law, and floor(pl * 2^32) of
    a negative pl has no uint32 value. rng='philox' raises ValueError naming the negative weight
    (DW_S_NEG_WEIGHT from dw_alias_build, read by its existing status check) and keeps no
    table. (The replay path follows the reference's random.choices and is left alone.)"""
    base = wr.hub_graph()
    w = wr.sym_weights(base, 'int')
    u, v, e_uv, e_vu = _chord(base)
    w[[e_uv, e_vu]] = -1.0
    rp = np.asarray(base.row_ptr)
    assert (np.add.reduceat(w, rp[1:-1]) > 0).all()
    csr = _weighted(w)
    starts = torch.as_tensor(np.array([HUB, u, v, 2], dtype=np.int32))
    for make in (lambda: DeepWalk(csr, 4, rng='philox', device=hip_device),
                 lambda: DeepWalk(csr, 4, rng='philox', layout='csr', device=hip_device),
                 lambda: Node2Vec(csr, 4, p=P, q=Q, rng='philox', device=hip_device),
                 lambda: Node2Vec(csr, 4, p=P, q=Q, rng='philox', layout='csr',
                                  device=hip_device)):
        with pytest.raises(ValueError, match='negative weight'):
            make().walk_batch(starts, walk_id0=0)
        assert 'prob_thr' not in csr._dev and 'alias' not in csr._dev
    with pytest.raises(ValueError, match='negative weight'):
        csr.device_tensors(hip_device, need_alias=True)
    # the graph's other builds are not poisoned by the refused one
    assert csr.device_tensors(hip_device, need_adj=True)['adj_hash'].numel() > 0


def test_infinite_weight_takes_every_step(hip_device):
    """A +inf weight is kept, and pinned to the limit law of a weight growing without bound: in
    its row every finite entry scales to 0 (threshold 0: the alias is always taken) and aliases
    to the infinite entry (scaled NaN: never 'small', so it stays on the large stack and ends
    ALWAYS). The tables equal the oracle's bit for bit and a walker in such a row always leaves
    by that edge."""
    base = wr.hub_graph()
    w = wr.sym_weights(base, 'int')
    u, v, e_uv, e_vu = _chord(base)
    w[[e_uv, e_vu]] = np.inf
    csr = _weighted(w)
    d = csr.device_tensors(hip_device, need_alias=True)
    prob, alias = ph.alias_tables(csr.row_ptr, w)
    got_prob = d['prob_thr'].cpu().numpy().view(np.uint32)
    got_alias = d['alias'].cpu().numpy()
    np.testing.assert_array_equal(got_prob, prob)
    np.testing.assert_array_equal(got_alias, alias)
    rp = np.asarray(base.row_ptr)
    for node, e in ((u, e_uv), (v, e_vu)):
        a, b = int(rp[node]), int(rp[node + 1])
        k = e - a
        others = np.arange(a, b) != e
        assert got_prob[e] == ph.ALWAYS and got_alias[e] == k
        assert (got_prob[a:b][others] == 0).all() and (got_alias[a:b][others] == k).all()
    starts = torch.as_tensor(np.array([u, v] * 64, dtype=np.int32))
    for wk in (DeepWalk(csr, 5, rng='philox', seed=3, device=hip_device),
               DeepWalk(csr, 5, rng='philox', seed=3, layout='csr', device=hip_device),
               Node2Vec(csr, 5, p=P, q=Q, rng='philox', seed=3, layout='hash',
                        device=hip_device)):
        got = wk.walk_batch(starts, walk_id0=0).cpu().numpy()
        np.testing.assert_array_equal(got[0::2], np.tile([u, v, u, v, u], (64, 1)))
        np.testing.assert_array_equal(got[1::2], np.tile([v, u, v, u, v], (64, 1)))
