"""The held-out edge split on the host (shallow_encoders/graph/holdout.py) against the loop
restatement tests/holdout_ref.py, the properties the protocol relies on, the cap at fixed inputs,
the integer U2 restatement against sklearn, and the options' validation. No GPU."""
import logging

import numpy as np
import pytest

import holdout_ref as ref
from shallow_encoders.graph.csr import CSRGraph
from shallow_encoders.graph.edge_list import edge_list_csr
from shallow_encoders.graph.holdout import split_edges

GRAPHS = {'karate': lambda: ref.karate(False), 'karate_weighted': lambda: ref.karate(True),
          'triplets': ref.triplets, 'rmat12': ref.rmat12, 'self_loops': ref.self_loops}
CASES = [(0.5, s) for s in range(5)] + [(0.1, 0), (0.9, 0)]


@pytest.fixture(scope='module', params=sorted(GRAPHS))
def graph(request):
    return GRAPHS[request.param]()


def _edge_set(csr):
    rows = np.repeat(np.arange(csr.vocab_size), np.diff(csr.row_ptr))
    col = csr.host_col()
    return {(int(a), int(b)) for a, b in zip(rows, col) if b >= a}


# ---- 1. the host path equals the loop restatement -------------------------------------------------
def test_host_split_equals_the_loop_restatement(graph):
    for ratio, seed in CASES:
        train, held, info = split_edges(graph, ratio, seed)
        row_ptr, col, w, held_ref, info_ref = ref.split_edges(
            graph.row_ptr, graph.host_col(), graph.weights, ratio, seed)
        np.testing.assert_array_equal(train.row_ptr, row_ptr)
        np.testing.assert_array_equal(train.col, col)
        assert train.col.dtype == np.int32 and held.dtype == np.int64
        np.testing.assert_array_equal(held, held_ref)
        assert info == info_ref
        if w is None:
            assert train.weights is None
        else:
            np.testing.assert_array_equal(train.weights, w)


# ---- 2. properties -------------------------------------------------------------------------------
def test_split_properties(graph):
    full = _edge_set(graph)
    loops = {e for e in full if e[0] == e[1]}
    deg = graph.degree()
    for ratio, seed in CASES:
        train, held, info = split_edges(graph, ratio, seed)
        tdeg = train.degree()
        assert np.all(tdeg[deg >= 1] >= 1) and np.all(tdeg[deg == 0] == 0)
        h = {(int(a), int(b)) for a, b in held}
        t = _edge_set(train)
        assert len(h) == len(held) and all(a < b for a, b in h)
        assert not (h & t) and (h | t) == full and loops <= t
        assert len(held) == info['n_hold'] == min(round(ratio * (len(full) - len(loops))),
                                                  info['n_candidates'])
        assert train.vocab_size == graph.vocab_size and list(train.itos[:3]) == list(graph.itos[:3])


def test_train_csr_is_the_edge_list_csr_of_the_surviving_edges():
    """The full graph is built from an edge list; dropping the held edges from that list (in its
    order) and building again gives the train CSR, weights included. Node ids 0 .. 59 all occur
    and keep an edge, so both builds rank them alike."""
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, 60, 300), rng.integers(0, 60, 300)
    src[:8] = dst[:8] = np.arange(8) * 7
    w = rng.random(300)
    full = edge_list_csr(src, dst, weights=w)
    assert full.vocab_size == 61
    train, held, _ = split_edges(full, 0.5, 3)
    h = {(int(a) - 1, int(b) - 1) for a, b in held}
    keep = np.asarray([(min(a, b), max(a, b)) not in h for a, b in zip(src, dst)])
    again = edge_list_csr(src[keep], dst[keep], weights=w[keep])
    np.testing.assert_array_equal(train.row_ptr, again.row_ptr)
    np.testing.assert_array_equal(train.col, again.col)
    np.testing.assert_array_equal(train.weights, again.weights)


def test_seeds_differ_and_ratio_zero_copies():
    g = ref.karate(True)
    a = split_edges(g, 0.5, 0)[1]
    b = split_edges(g, 0.5, 1)[1]
    assert a.shape == b.shape and not np.array_equal(a, b)
    train, held, info = split_edges(g, 0.0, 0)
    assert held.shape == (0, 2) and info['n_hold'] == 0
    np.testing.assert_array_equal(train.row_ptr, g.row_ptr)
    np.testing.assert_array_equal(train.col, g.col)
    np.testing.assert_array_equal(train.weights, g.weights)


# ---- 3. the cap at fixed inputs ------------------------------------------------------------------
def test_cap_at_fixed_inputs():
    for seed in range(5):
        info = split_edges(ref.karate(False), 0.5, seed)[2]
        assert (info['n_edges'], info['n_want'], info['n_hold']) == (78, 39, 39)
        assert 50 <= info['n_candidates'] <= 54
        info = split_edges(ref.path(), 0.5, seed)[2]
        assert (info['n_edges'], info['n_want']) == (7, 4)
        assert info['n_candidates'] in (1, 2) and info['n_hold'] == info['n_candidates']
    assert split_edges(ref.star(), 0.5, 0)[2] == {
        'n_edges': 9, 'n_want': 4, 'n_candidates': 0, 'n_hold': 0}
    g = ref.rmat12()
    assert g.vocab_size == 4097 and int(g.degree().max()) == 1035
    assert split_edges(g, 0.5, 0)[2] == {
        'n_edges': 32749, 'n_want': 16374, 'n_candidates': 29142, 'n_hold': 16374}


# ---- 4. U2 against sklearn -----------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.auc_cases(), ids=lambda c: c[0])
def test_u2_restatement_against_sklearn(case):
    from sklearn.metrics import roc_auc_score
    name, scores, labels = case
    got = ref.auc(scores, labels)
    # sklearn refuses an infinite score; AUC depends on the order alone, so it gets the scores
    # with +-inf moved to finite values beyond every finite score
    finite = np.where(np.isposinf(scores), 1e300, np.where(np.isneginf(scores), -1e300, scores))
    assert abs(got - roc_auc_score(labels, finite)) <= 1e-12
    if name in ('all_equal', 'signed_zeros'):
        assert got == 0.5
    if name == 'separated':
        assert got == 1.0
    if name == 'separated_reversed':
        assert got == 0.0


def test_auc_from_counts_refuses_an_empty_class():
    from shallow_encoders.graph.linkpred import auc_from_counts
    assert auc_from_counts(3, 1, 2) == 0.75
    with pytest.raises(ValueError):
        auc_from_counts(0, 0, 4)
    with pytest.raises(ValueError):
        auc_from_counts(0, 4, 0)


# ---- 5. validation -------------------------------------------------------------------------------
def test_split_refusals():
    g = ref.karate(False)
    for ratio in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError):
            split_edges(g, ratio, 0)
    dup = CSRGraph.from_arrays([0, 0, 2, 3, 4], [2, 2, 1, 1])
    with pytest.raises(ValueError, match='twice'):
        split_edges(dup, 0.5, 0)
    on_unk = CSRGraph.from_arrays([0, 1, 2], [1, 0])
    with pytest.raises(ValueError, match='malformed'):
        split_edges(on_unk, 0.5, 0)
    low = CSRGraph.from_arrays([0, 0, 1, 2], [0, 2])
    with pytest.raises(ValueError, match='malformed'):
        split_edges(low, 0.5, 0)


def test_config_validation():
    from shallow_encoders.config_parser.core import GraphDownstreamEdgeClassificationConfig as C
    assert (C().protocol, C().scorer) == ('reference', 'classifier')
    c = C(protocol='heldout', backend='device', scorer='dot')
    assert (c.protocol, c.scorer) == ('heldout', 'dot')
    with pytest.raises(ValueError, match='protocol'):
        C(protocol='paper')
    with pytest.raises(ValueError, match='scorer'):
        C(scorer='cosine')
    with pytest.raises(ValueError, match='backend=device'):
        C(protocol='heldout')


def test_dataset_options(caplog):
    from shallow_encoders.graph.datasets import (GraphTriplets, KarateClubDataset, RMATDataset,
                                                 RandomWalkDataset)
    plain = RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000)
    assert plain.heldout_edges is None and plain.holdout_info is None
    assert plain.full_csr is plain.csr
    ds = RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000, holdout_ratio=0.3,
                     holdout_seed=7)
    train, held, info = split_edges(plain.csr, 0.3, 7)
    np.testing.assert_array_equal(ds.heldout_edges, held)
    np.testing.assert_array_equal(ds.csr.row_ptr, train.row_ptr)
    np.testing.assert_array_equal(ds.csr.col, train.col)
    np.testing.assert_array_equal(ds.full_csr.row_ptr, plain.csr.row_ptr)
    assert ds.graph is ds.csr and ds.holdout_info == info and len(ds) == len(plain)
    with pytest.raises(ValueError, match='networkx'):
        KarateClubDataset(walks_per_node=1, walk_length=5, holdout_ratio=0.3)
    with pytest.raises(ValueError, match='networkx'):
        GraphTriplets(walks_per_node=1, walk_length=5, holdout_ratio=0.3)
    with pytest.raises(ValueError, match='hides no edge'):
        RandomWalkDataset(ref.star(), 1, 5, holdout_ratio=0.5)
    with caplog.at_level(logging.WARNING, logger='GraphDatasets'):
        capped = RandomWalkDataset(ref.path(), 1, 5, holdout_ratio=0.5)
    assert capped.holdout_info['n_hold'] < capped.holdout_info['n_want'] == 4
    assert any('asks for 4' in r.getMessage() for r in caplog.records)


def test_heldout_protocol_needs_a_holdout_dataset():
    from shallow_encoders.config_parser.core import GraphDownstreamEdgeClassificationConfig as C
    from shallow_encoders.graph.datasets import RMATDataset
    from tools import graph_model_downstream_classification as downstream
    plain = RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000)
    with pytest.raises(ValueError, match='holdout_ratio'):
        downstream.heldout_edge_classification_on_device(
            np.zeros((plain.csr.vocab_size, 4), dtype=np.float32), plain,
            C(protocol='heldout', backend='device'))
