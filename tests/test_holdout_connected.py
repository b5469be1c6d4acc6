"""The connected held-out edge split on the host (``split_edges(..., protect='connected')`` and
``connected_components`` of shallow_encoders/graph/holdout.py) against the Kruskal / breadth-first
restatement tests/holdout_connected_ref.py, the consequences of the rule, the counts at fixed
inputs, and the dataset option. No GPU."""
import functools
import logging

import numpy as np
import pytest

import holdout_connected_ref as cref
from shallow_encoders.graph.holdout import connected_components, split_edges

GRAPHS = cref.graphs()
RATIOS, SEEDS = (0.1, 0.5, 0.9), (0, 7)


@functools.lru_cache(maxsize=None)
def built(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def forest_of(name, seed):
    g = built(name)
    return frozenset(cref.forest(g.row_ptr, g.host_col(), seed))


@pytest.fixture(scope='module', params=sorted(GRAPHS))
def name(request):
    return request.param


def _edges(csr):
    return set(cref.csr_edges(csr.row_ptr, csr.host_col()))


# ---- 1. the host path equals the restatement ------------------------------------------------------
def test_host_split_equals_the_kruskal_restatement(name):
    g = built(name)
    for ratio in RATIOS:
        for seed in SEEDS:
            train, held, info = split_edges(g, ratio, seed, protect='connected')
            row_ptr, col, w, held_ref, info_ref = cref.split_edges(
                g.row_ptr, g.host_col(), g.weights, ratio, seed)
            np.testing.assert_array_equal(train.row_ptr, row_ptr)
            np.testing.assert_array_equal(train.col, col)
            assert train.col.dtype == np.int32 and held.dtype == np.int64
            np.testing.assert_array_equal(held, held_ref)
            assert info == info_ref
            if w is None:
                assert train.weights is None
            else:
                np.testing.assert_array_equal(train.weights, w)


# ---- 2. the consequences of the rule --------------------------------------------------------------
def test_residual_graph_keeps_the_components_and_the_forest(name):
    g = built(name)
    labels = cref.components(g.row_ptr, g.host_col())
    full = _edges(g)
    touched = {n for e in full for n in e}
    for ratio in RATIOS:
        for seed in SEEDS:
            train, held, info = split_edges(g, ratio, seed, protect='connected')
            np.testing.assert_array_equal(cref.components(train.row_ptr, train.col), labels)
            forest = forest_of(name, seed)
            h = {(int(a), int(b)) for a, b in held}
            assert not h & forest and forest <= _edges(train)
            # every edge the degree rule protects is a forest edge (the cut property) ...
            assert cref.degree_protected(g.row_ptr, g.host_col(), seed) <= forest
            # ... so the connected rule has no candidate the degree rule lacks
            assert info['n_candidates'] <= split_edges(g, ratio, seed)[2]['n_candidates']
            # the counts
            assert info['n_forest'] == len(forest) == len(touched) - info['n_components']
            assert info['n_candidates'] == info['n_edges'] - info['n_forest']
            assert info['n_hold'] == len(held) == min(round(ratio * len(full)),
                                                      info['n_candidates'])


def test_connected_components_equal_the_breadth_first_labels(name):
    g = built(name)
    labels, n = connected_components(g)
    want = cref.components(g.row_ptr, g.host_col())
    assert labels.dtype == np.int32
    np.testing.assert_array_equal(labels, want)
    assert n == len(set(want[1:].tolist()))


def test_the_bridge_is_never_held():
    g = cref.bridge()
    labels, n = connected_components(g)
    assert n == 2 and sorted(set(labels.tolist())) == [0, 1, 7]      # <unk>, the cliques, row 7
    for ratio in (0.1, 0.5, 0.9, 0.99):
        for seed in range(8):
            train, held, info = split_edges(g, ratio, seed, protect='connected')
            assert cref.BRIDGE not in {(int(a), int(b)) for a, b in held}
            assert cref.BRIDGE in _edges(train)
            assert (info['n_edges'], info['n_forest'], info['n_components']) == (31, 11, 1)


# ---- 3. the counts at fixed inputs ----------------------------------------------------------------
def test_counts_at_fixed_inputs():
    for seed in SEEDS:
        info = split_edges(built('karate'), 0.5, seed, protect='connected')[2]
        assert info == {'n_edges': 78, 'n_want': 39, 'n_candidates': 45, 'n_hold': 39,
                        'n_forest': 33, 'n_components': 1}
        assert 49 <= split_edges(built('karate'), 0.5, seed)[2]['n_candidates'] <= 50
        info = split_edges(built('rmat12'), 0.5, seed, protect='connected')[2]
        assert info == {'n_edges': 32749, 'n_want': 16374, 'n_candidates': 28655,
                        'n_hold': 16374, 'n_forest': 4094, 'n_components': 2}
        info = split_edges(built('self_loops'), 0.5, seed, protect='connected')[2]
        assert (info['n_forest'], info['n_candidates']) == (59, 201)
        for tree in ('triplets', 'star', 'path'):
            info = split_edges(built(tree), 0.5, seed, protect='connected')[2]
            assert info['n_candidates'] == 0 and info['n_hold'] == 0
        assert split_edges(built('path'), 0.5, seed)[2]['n_candidates'] in (1, 2)
        # a cycle: every edge but the one of largest priority is in the forest
        g = built('cycle')
        train, held, info = split_edges(g, 0.5, seed, protect='connected')
        assert (info['n_forest'], info['n_candidates'], info['n_hold']) == (4999, 1, 1)
        assert tuple(held[0]) == max(_edges(g), key=lambda e: cref.prio(e[0], e[1], seed))
        info = split_edges(built('three_cycles'), 0.5, seed, protect='connected')[2]
        assert (info['n_forest'], info['n_components'], info['n_candidates']) == (9, 3, 3)


def test_boruvka_rounds_at_fixed_inputs():
    """The rounds the host's forest takes (the kernels take the same: one rule)."""
    from shallow_encoders.graph import holdout
    for seed in SEEDS:
        for graph, rounds in (('karate', 2), ('rmat12', 4), ('self_loops', 3)):
            g = built(graph)
            x, y = holdout._entries(g)
            assert holdout._forest(g.vocab_size, x, y, holdout._prio(x, y, seed))[2] == rounds


# ---- 4. the argument ------------------------------------------------------------------------------
def test_protect_degree_is_the_default_and_unknown_rules_are_refused():
    for graph in ('karate_weighted', 'self_loops', 'path'):
        g = built(graph)
        a, held_a, info_a = split_edges(g, 0.5, 3)
        b, held_b, info_b = split_edges(g, 0.5, 3, protect='degree')
        assert info_a == info_b and set(info_a) == {'n_edges', 'n_want', 'n_candidates', 'n_hold'}
        np.testing.assert_array_equal(held_a, held_b)
        np.testing.assert_array_equal(a.row_ptr, b.row_ptr)
        np.testing.assert_array_equal(a.col, b.col)
        np.testing.assert_array_equal(a.weights, b.weights)
    with pytest.raises(ValueError, match='protect'):
        split_edges(built('karate'), 0.5, 0, protect='bridges')


# ---- 5. the dataset option ------------------------------------------------------------------------
def test_graph_rmat_dataset_with_a_connected_holdout(caplog):
    from shallow_encoders.graph.datasets import RMATDataset, RandomWalkDataset
    plain = RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000)
    ds = RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000, holdout_ratio=0.5,
                     holdout_seed=7, holdout_protect='connected')
    train, held, info = split_edges(plain.csr, 0.5, 7, protect='connected')
    np.testing.assert_array_equal(ds.heldout_edges, held)
    np.testing.assert_array_equal(ds.csr.row_ptr, train.row_ptr)
    np.testing.assert_array_equal(ds.csr.col, train.col)
    np.testing.assert_array_equal(ds.full_csr.row_ptr, plain.csr.row_ptr)
    assert ds.holdout_info == info and {'n_forest', 'n_components'} <= set(info)
    np.testing.assert_array_equal(connected_components(ds.csr)[0],
                                  connected_components(ds.full_csr)[0])
    with pytest.raises(ValueError, match='hides no edge.*holdout_protect=connected'):
        RandomWalkDataset(built('path'), 1, 5, holdout_ratio=0.5, holdout_protect='connected')
    with caplog.at_level(logging.WARNING, logger='GraphDatasets'):
        capped = RandomWalkDataset(built('three_cycles'), 1, 5, holdout_ratio=0.5,
                                   holdout_protect='connected')
    assert capped.holdout_info['n_hold'] == 3 < capped.holdout_info['n_want'] == 6
    assert any('holdout_protect=connected' in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError, match='protect'):
        RMATDataset(walks_per_node=1, walk_length=5, scale=8, n_edges=2000, holdout_ratio=0.5,
                    holdout_protect='bridges')
