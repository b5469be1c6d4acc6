"""Device link prediction without a device (DESIGN.md "Device link prediction"): the restated
rank rule and its law, the entry points' argument checks through ctypes, the wrapper's
refusals, and the L-BFGS driver on a numpy closure against sklearn.

Significance (the convention of tests/test_gpu_walk_law.py): family-wise alpha = 1e-3 with a
Bonferroni correction over the N_TESTS statistical tests of this module; seeds are fixed."""
import ctypes

import numpy as np
import pytest
import torch

import linkpred_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import linkpred
from shallow_encoders.graph.csr import CSRGraph

N_TESTS = 1
ALPHA = 1e-3 / N_TESTS


# ---- the rank rule ----------------------------------------------------------------------------
def test_rank_rule_lists_the_non_neighbours_of_every_karate_node():
    _, row_ptr, _, cs = ref.karate()
    for u in range(1, 35):
        c = cs[row_ptr[u]:row_ptr[u + 1]]
        want = [v for v in range(1, 35) if v not in set(c.tolist())]
        assert len(want) == 34 - len(c)
        got = [ref.rank_non_neighbour(c, 1, k) for k in range(len(want))]
        assert got == want, u


@pytest.mark.parametrize('first_node', [0, 1, 3])
def test_rank_rule_on_a_row_of_degree_nn_minus_one(first_node):
    nn = 6
    nodes = list(range(first_node, first_node + nn))
    for missing in nodes:
        c = np.asarray([v for v in nodes if v != missing])
        assert ref.rank_non_neighbour(c, first_node, 0) == missing
    assert [ref.rank_non_neighbour(np.asarray([], dtype=np.int64), first_node, k)
            for k in range(nn)] == nodes


def test_vectorised_restatement_equals_the_plain_one():
    _, row_ptr, _, cs = ref.karate()
    for seed, off in ((0, 0), (7, 2 ** 32 + 5), (2 ** 40 + 3, 2 ** 63)):
        a = ref.negative_edges(row_ptr, cs, 1, 2000, seed, off)
        b = ref.negative_edges_fast(row_ptr, cs, 1, 2000, seed, off)
        np.testing.assert_array_equal(a, b)
    # samples are a function of offset + i alone
    np.testing.assert_array_equal(ref.negative_edges(row_ptr, cs, 1, 50, 3, 10)[5:],
                                  ref.negative_edges(row_ptr, cs, 1, 45, 3, 15))


def test_law_of_the_restated_sampler_on_karate():
    """chi-square of 200,000 samples against P(u, v) = 1 / (Nn (Nn - deg u)) over the 1,000
    non-adjacent ordered pairs (u == v included)."""
    from scipy.stats import chi2
    _, row_ptr, _, cs = ref.karate()
    n = 200_000
    s = ref.negative_edges_fast(row_ptr, cs, 1, n, seed=11)
    adj = np.zeros((35, 35), dtype=bool)
    for u in range(1, 35):
        adj[u, cs[row_ptr[u]:row_ptr[u + 1]]] = True
    assert not adj[s[:, 0], s[:, 1]].any()
    assert s.min() >= 1 and s.max() <= 34
    deg = np.diff(row_ptr)
    cells = [(u, v) for u in range(1, 35) for v in range(1, 35) if not adj[u, v]]
    assert len(cells) == 34 * 34 - 2 * 78
    expected = np.asarray([n / (34 * (34 - deg[u])) for u, _ in cells])
    counts = np.zeros((35, 35), dtype=np.int64)
    np.add.at(counts, (s[:, 0], s[:, 1]), 1)
    obs = np.asarray([counts[u, v] for u, v in cells])
    assert obs.sum() == n and expected.min() > 100
    stat = float(((obs - expected) ** 2 / expected).sum())
    pv = float(chi2.sf(stat, len(cells) - 1))
    print(f'negative pairs on karate: {n} samples, {len(cells)} cells, chi2 {stat:.1f}, '
          f'p-value {pv:.3g}')
    assert pv > ALPHA, f'p-value {pv:.3g} <= {ALPHA:.2g}'


# ---- the entry points' argument checks (no device call is made) -------------------------------
def _features(d=8, op=0, n=4, V=10, table=None):
    lib = _native.load()
    rc = lib.dw_edge_features(table, V, d, op, None, n, None, None, None)
    return rc, lib.dw_last_error_string()


def _logreg(d=8, op=0, n=4, V=10, table=None):
    lib = _native.load()
    rc = lib.dw_edge_logreg(table, V, d, op, None, None, n, None, None, None, 0, None, None)
    return rc, lib.dw_last_error_string()


@pytest.mark.parametrize('call', [_features, _logreg])
@pytest.mark.parametrize('kw', [dict(d=0), dict(d=513), dict(op=4), dict(op=-1), dict(n=-1),
                                dict(V=0), dict(V=2 ** 31)])
def test_abi_refuses_bad_sizes_before_the_pointers(call, kw):
    rc, err = call(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert b'bad sizes' in err and b'null pointer' not in err, err


@pytest.mark.parametrize('call', [_features, _logreg])
def test_abi_takes_the_limits_up_to_the_pointers(call):
    for kw in (dict(), dict(d=1), dict(d=512, op=3), dict(V=2 ** 31 - 1)):
        rc, err = call(**kw)
        assert rc == _native.DW_E_INVALID_ARG and b'null pointer' in err, (kw, err)
        assert call(n=0, **kw)[0] == _native.DW_OK


def test_abi_negative_edges_checks():
    lib = _native.load()

    def call(n_rows=35, first=1, n=4):
        rc = lib.dw_negative_edges(None, None, n_rows, first, n, 0, 0, None, None, None)
        return rc, lib.dw_last_error_string()
    for kw in (dict(n_rows=0), dict(n_rows=2 ** 31), dict(first=-1), dict(first=35), dict(n=-1)):
        rc, err = call(**kw)
        assert rc == _native.DW_E_INVALID_ARG and b'null pointer' not in err, (kw, err)
    rc, err = call()
    assert rc == _native.DW_E_INVALID_ARG and b'null pointer' in err
    assert call(n=0)[0] == _native.DW_OK


def test_abi_workspace_size():
    lib = _native.load()
    nb = ctypes.c_size_t(0)
    assert lib.dw_edge_logreg_workspace_bytes(0, 128, ctypes.byref(nb)) == _native.DW_OK
    assert nb.value == 131 * 8
    # one partial row of d + 3 doubles per block, a grid that grows with n up to a fixed cap
    assert lib.dw_edge_logreg_workspace_bytes(10 ** 4, 128, ctypes.byref(nb)) == _native.DW_OK
    small = nb.value
    assert lib.dw_edge_logreg_workspace_bytes(10 ** 9, 128, ctypes.byref(nb)) == _native.DW_OK
    assert small == 625 * 131 * 8 and nb.value == 1024 * 131 * 8
    for n, d in ((-1, 8), (4, 0), (4, 513)):
        assert lib.dw_edge_logreg_workspace_bytes(n, d, ctypes.byref(nb)) == \
            _native.DW_E_INVALID_ARG


# ---- the wrapper's refusals (all before any device work) --------------------------------------
def test_wrapper_refuses_unsampleable_graphs():
    # node 1 adjacent to every node, itself included: no non-neighbour
    full = CSRGraph.from_arrays([0, 0, 3, 4, 5], [1, 2, 3, 1, 1])
    with pytest.raises(ValueError, match='no non-neighbour'):
        linkpred.negative_edges(full, 4, 0)
    # <unk> (row 0) with a neighbour
    unk = CSRGraph.from_arrays([0, 1, 2, 2], [1, 0])
    with pytest.raises(ValueError, match='<unk>'):
        linkpred.negative_edges(unk, 4, 0)
    # a repeated neighbour: the word dw_csr_check_simple leaves (the device run is in
    # test_gpu_linkpred.py)
    _, row_ptr, _, _ = ref.karate()
    linkpred.check_negative_graph(row_ptr, 1, 0)
    with pytest.raises(ValueError, match='same neighbour twice'):
        linkpred.check_negative_graph(row_ptr, 1, _native.DW_S_DUP_NEIGHBOR)
    with pytest.raises(ValueError):
        linkpred.negative_edges(full, -1, 0)


def test_wrapper_refuses_unknown_names():
    table = torch.zeros((5, 4))
    pairs = torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(AssertionError, match='not supported'):
        linkpred.edge_embeddings_device(table, pairs, 'cosine')
    with pytest.raises(AssertionError, match='not supported'):
        linkpred.EdgeLogisticRegression('cosine')
    assert linkpred.EdgeLogisticRegression('HADAMARD').op == 1
    with pytest.raises(ValueError, match='penalty'):
        linkpred.EdgeLogisticRegression.from_params('hadamard', {'C': 2.0, 'penalty': 'l1'})
    csr = CSRGraph.from_arrays([0, 0, 1, 2], [2, 1])
    with pytest.raises(ValueError, match='solver'):
        linkpred.edge_classification_device(table[:3], csr, 0.5, 1, 'hadamard',
                                            classifier_params={'solver': 'saga'})
    clf = linkpred.EdgeLogisticRegression.from_params(
        'average', {'C': 0.5, 'fit_intercept': False, 'max_iter': 7, 'tol': 1e-3})
    assert (clf.C, clf.fit_intercept, clf.max_iter, clf.tol) == (0.5, False, 7, 1e-3)


def test_config_backend_field():
    from shallow_encoders.config_parser import load_config
    cfg = load_config('sge_sg_karate_club')
    assert cfg.downstream.edge_classification.backend == 'sklearn'
    cfg = load_config('sge_sg_karate_club',
                      overrides=['downstream.edge_classification.backend=device'])
    assert cfg.downstream.edge_classification.backend == 'device'
    with pytest.raises(ValueError, match='backend'):
        load_config('sge_sg_karate_club',
                    overrides=['downstream.edge_classification.backend=cuda'])


# ---- the L-BFGS driver on a numpy closure -----------------------------------------------------
SKLEARN_MARGIN = 0.0


def sklearn_objective(x64, y):
    from sklearn.linear_model import LogisticRegression
    sk = LogisticRegression().fit(x64, y)
    return ref.objective(x64, y, np.concatenate([sk.coef_[0], sk.intercept_]))


@pytest.mark.parametrize('op', range(4))
def test_lbfgs_driver_reaches_sklearns_objective(op):
    """The driver's final objective, recomputed here in float64, against sklearn's
    LogisticRegression() at its defaults on the same features. Measured gap (ours - sklearn) /
    sklearn on the CPU: average -2.6e-7, hadamard -3.4e-8, weighted_l1 -7.1e-8, weighted_l2
    -4.2e-9 — the driver stops on max|grad| <= 1e-4 of the unscaled objective, sklearn on the
    same bound of the objective divided by n C, so the driver ends below sklearn on all four
    (within 3.1e-12 of a tol = 1e-10 sklearn fit). The allowed excess is therefore none:
    SKLEARN_MARGIN = 0."""
    table, pairs, labels = ref.karate_problem()
    t32 = table.astype(np.float32)
    x64 = ref.features(t32, op, pairs).astype(np.float64)
    y = labels.astype(np.float64)
    clf = linkpred.EdgeLogisticRegression(ref.OPS[op])
    clf.fit_closure(lambda c: ref.logreg_sums(t32, op, pairs, labels, c)[0], 8)
    ours = ref.objective(x64, y, clf.full_coef())
    theirs = sklearn_objective(x64, y)
    print(f'{ref.OPS[op]}: objective {ours!r} vs sklearn {theirs!r}, gap '
          f'{(ours - theirs) / theirs:.3g}, {clf.n_iter_} iterations')
    assert clf.coef_.shape == (8,) and 0 < clf.n_iter_ <= 100
    assert abs(clf.objective_ - ours) <= 1e-12 * ours
    assert ours <= theirs * (1.0 + SKLEARN_MARGIN)


def test_lbfgs_driver_options():
    table, pairs, labels = ref.karate_problem()
    t32 = table.astype(np.float32)

    def sums(c):
        return ref.logreg_sums(t32, 1, pairs, labels, c)[0]
    free = linkpred.EdgeLogisticRegression('hadamard').fit_closure(sums, 8)
    fixed = linkpred.EdgeLogisticRegression('hadamard', fit_intercept=False).fit_closure(sums, 8)
    assert fixed.intercept_ == 0.0 and free.intercept_ != 0.0
    assert fixed.objective_ >= free.objective_
    short = linkpred.EdgeLogisticRegression('hadamard', max_iter=2).fit_closure(sums, 8)
    assert short.n_iter_ <= 2 and short.objective_ > free.objective_
    # the minimiser itself, on a quadratic with a known minimum
    a = np.arange(1.0, 6.0)
    x, f, it = linkpred.lbfgs_minimize(lambda v: (0.5 * float(a @ (v - 1) ** 2), a * (v - 1)),
                                       np.zeros(5), 100, 1e-10)
    np.testing.assert_allclose(x, np.ones(5), rtol=0, atol=1e-9)
    assert f <= 1e-18 and it <= 100
