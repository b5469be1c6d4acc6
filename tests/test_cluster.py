"""Community detection on the host (shallow_encoders/graph/cluster.py with device=None): the numpy
Lloyd pass against the plain-loop restatement, NMI / ARI against sklearn, modularity against
networkx, k-means on far blobs against sklearn.cluster.KMeans from the same init, and the
downstream.clustering config section.

The float bar is the project's: every float64 sum within 1e-10 * sum |terms|."""
import numpy as np
import pytest

import cluster_ref as ref
import holdout_ref
from shallow_encoders.graph import cluster

BOUND = 1e-10


def blobs(seed=0, n=400, d=8, k=4):
    """k unit-variance Gaussian blobs whose centres are 100 sigma apart along the axes."""
    rng = np.random.default_rng(seed)
    truth = np.arange(n) % k
    centres = 100.0 * np.eye(k, d)
    table = np.zeros((n + 1, d), dtype=np.float32)   # row 0: <unk>, never a sample
    table[1:] = (centres[truth] + rng.standard_normal((n, d))).astype(np.float32)
    return table, np.arange(1, n + 1, dtype=np.int64), truth


# ---- the host pass ------------------------------------------------------------------------------
@pytest.mark.parametrize('d,K,n', [(1, 1, 5), (3, 17, 200), (16, 4, 333), (130, 7, 64)])
def test_host_step_equals_restatement(d, K, n):
    rng = np.random.default_rng(100 * d + K)
    table = rng.standard_normal((50, d)).astype(np.float32)
    ids = rng.integers(0, 50, n)
    C = rng.standard_normal((K, d))
    prev = rng.integers(0, K, n)
    want_labels, want, mags, margins = ref.step(table, ids, C, prev)
    assert margins.min() > 2 * BOUND
    labels, out = cluster.kmeans_step_host(table[ids].astype(np.float64), C, prev)
    np.testing.assert_array_equal(labels, want_labels)
    ld = d + 1
    counts = out[:K * ld].reshape(K, ld)[:, d]
    np.testing.assert_array_equal(counts, want[:K * ld].reshape(K, ld)[:, d])
    assert out[-1] == want[-1]
    err = np.abs(out - want)
    print(f'{(d, K, n)}: worst |error| / sum|terms| '
          f'{float((err / np.maximum(mags, 1e-300))[mags > 0].max()):.3g}')
    assert (err <= BOUND * mags).all()
    assert cluster.kmeans_step_host(table[ids].astype(np.float64), C)[1][-1] == n


def test_host_step_ties_go_to_the_lowest_cluster():
    table = np.array([[0, 0], [2, 0], [1, 1], [1, 0]], dtype=np.float32)
    C = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 0.0], [0.0, 0.0]])
    ids = np.arange(4)
    labels, out = cluster.kmeans_step_host(table.astype(np.float64), C)
    np.testing.assert_array_equal(labels, ref.step(table, ids, C)[0])
    np.testing.assert_array_equal(labels, [0, 1, 0, 0])


# ---- the scores ---------------------------------------------------------------------------------
def partitions():
    rng = np.random.default_rng(3)
    n = 500
    a = rng.integers(0, 7, n)
    yield 'random', a, rng.integers(0, 5, n)
    yield 'correlated', a, np.where(rng.random(n) < 0.8, a % 4, rng.integers(0, 4, n))
    yield 'one-against-many', np.zeros(n, dtype=np.int64), a
    yield 'identical', a, a.copy()
    yield 'relabelled', a, (a + 3) % 7
    yield 'empty-class', np.where(a == 2, 6, a), rng.integers(0, 5, n) * 2   # gaps in both
    yield 'one-against-one', np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)


@pytest.mark.parametrize('name,a,b', list(partitions()), ids=[p[0] for p in partitions()])
def test_nmi_and_ari_equal_sklearn(name, a, b):
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    table = cluster.contingency(a, b)
    np.testing.assert_array_equal(table, ref.contingency(a, b, a.max() + 1, b.max() + 1))
    assert cluster.nmi(a, b) == pytest.approx(normalized_mutual_info_score(a, b), abs=1e-12)
    assert cluster.ari(a, b) == pytest.approx(adjusted_rand_score(a, b), abs=1e-12)
    assert cluster.nmi(a, b) == pytest.approx(ref.nmi(a, b), abs=1e-12)
    assert cluster.ari(a, b) == pytest.approx(ref.ari(a, b), abs=1e-12)


def test_contingency_skips_unassigned_samples():
    a = np.array([0, 1, -1, 1, 2])
    b = np.array([1, -1, 0, 1, 0])
    np.testing.assert_array_equal(cluster.contingency(a, b), [[0, 1], [0, 1], [1, 0]])
    with pytest.raises(IndexError):
        cluster.contingency(a, b, n_a=2)
    with pytest.raises(ValueError):
        cluster.contingency(a, b[:3])


def graphs():
    import networkx as nx
    k = nx.karate_club_graph()
    yield 'karate', k, [{v for v in k if k.nodes[v]['club'] == c} for c in ('Mr. Hi', 'Officer')]
    rng = np.random.default_rng(9)
    g = nx.gnm_random_graph(40, 120, seed=4)
    for v in (0, 5, 11, 12, 30):
        g.add_edge(v, v)
    lab = rng.integers(0, 4, 40)
    yield 'self-loops', g, [{v for v in g if lab[v] == c} for c in range(4)]
    two = nx.disjoint_union(nx.complete_graph(6), nx.complete_graph(5))
    two.add_edge(0, 6)
    yield 'two-cliques', two, [set(range(6)), set(range(6, 11))]


@pytest.mark.parametrize('name,g,parts', list(graphs()), ids=[p[0] for p in graphs()])
def test_modularity_equals_networkx(name, g, parts):
    import networkx as nx
    from shallow_encoders.graph.csr import CSRGraph
    csr = CSRGraph.from_networkx(nx.relabel_nodes(g, {v: f'n{v:02d}' for v in g}))
    labels = np.full(csr.vocab_size, -1, dtype=np.int64)
    for c, part in enumerate(parts):
        for v in part:
            labels[csr.node_id(f'n{v:02d}')] = c
    assert (labels[1:] >= 0).all()
    counts = cluster.modularity_counts(csr, labels)
    np.testing.assert_array_equal(
        counts, ref.modularity_counts(csr.row_ptr, csr.host_col(), labels, len(parts)))
    assert counts[:, 1].sum() == 2 * g.number_of_edges()   # a loop's entry counted twice
    want = nx.community.modularity(g, parts, weight=None)
    assert cluster.modularity(csr, labels) == pytest.approx(want, abs=1e-12)


def test_modularity_ignores_weights_and_unassigned_rows():
    csr = holdout_ref.self_loops()
    assert csr.weighted
    rng = np.random.default_rng(1)
    labels = rng.integers(-1, 3, csr.vocab_size)
    np.testing.assert_array_equal(
        cluster.modularity_counts(csr, labels, 3),
        ref.modularity_counts(csr.row_ptr, csr.host_col(), labels, 3))
    with pytest.raises(ValueError):
        cluster.modularity(csr, labels[:-1])


# ---- k-means ------------------------------------------------------------------------------------
BLOB_SEED = 0


def test_far_blobs_are_recovered_and_match_sklearn():
    from sklearn.cluster import KMeans
    table, ids, truth = blobs()
    labels, cent, inertia, n_iter = cluster.kmeans(table, ids, 4, n_init=4, seed=BLOB_SEED)
    assert labels.dtype == np.int64 and cent.shape == (4, 8) and n_iter >= 1
    assert cluster.nmi(truth, labels) == 1.0
    X = table[ids].astype(np.float64)
    # consistent: labels and inertia are those of the returned centroids, which are the means
    assert inertia == pytest.approx(((X - cent[labels]) ** 2).sum(), rel=1e-9)
    for k in range(4):
        np.testing.assert_allclose(cent[k], X[labels == k].mean(axis=0), rtol=1e-12, atol=1e-12)
    # from the same explicit init the objective is never above sklearn's
    init = X[[0, 1, 2, 3]]
    ours = cluster.kmeans(table, ids, 4, init=init)
    theirs = KMeans(n_clusters=4, init=init, n_init=1, algorithm='lloyd', tol=0.0).fit(X)
    print(f'inertia {ours[2]!r} (sklearn {theirs.inertia_!r}), {ours[3]} iterations')
    assert ours[2] <= theirs.inertia_ * (1 + 1e-12)
    assert cluster.nmi(truth, ours[0]) == 1.0


def test_restarts_and_inits():
    table, ids, truth = blobs(seed=1)
    one = cluster.kmeans(table, ids, 4, n_init=1, seed=5)
    many = cluster.kmeans(table, ids, 4, n_init=6, seed=5)
    assert many[2] <= one[2]
    again = cluster.kmeans(table, ids, 4, n_init=6, seed=5)
    np.testing.assert_array_equal(many[0], again[0])
    assert many[2] == again[2]
    rnd = cluster.kmeans(table, ids, 4, init='random', n_init=3, seed=2)
    assert set(rnd[0].tolist()) <= {0, 1, 2, 3}
    capped = cluster.kmeans(table, ids, 4, init=table[1:5].astype(np.float64) * 0.01, max_iter=1)
    assert capped[3] == 1
    X = table[ids].astype(np.float64)
    assert capped[2] == pytest.approx(((X - capped[1][capped[0]]) ** 2).sum(), rel=1e-9)
    with pytest.raises(ValueError):
        cluster.kmeans(table, ids, 0)
    with pytest.raises(ValueError):
        cluster.kmeans(table, ids, 4, init='farthest')
    with pytest.raises(ValueError):
        cluster.kmeans(table, ids[:3], 4)
    with pytest.raises(IndexError):
        cluster.kmeans(table, np.array([1, 2, len(table)]), 2)


def test_empty_cluster_keeps_its_centroid():
    table, ids, _ = blobs(seed=2)
    init = np.concatenate([table[1:4].astype(np.float64), np.full((1, 8), 1e4)])
    labels, cent, _, _ = cluster.kmeans(table, ids, 4, init=init)
    assert 3 not in set(labels.tolist())
    np.testing.assert_array_equal(cent[3], init[3])


def test_host_seeding_follows_the_restatement():
    rng = np.random.default_rng(7)
    X = rng.integers(-3, 4, size=(64, 2)).astype(np.float64)
    for seed in range(50):
        chosen, cent = cluster.kmeans_seed_host(X, 3, seed)
        assert chosen[0] == ref.seed_first(64, seed)
        assert chosen[1] == ref.seed_pick(X, chosen[:1], seed, 1)
        assert chosen[2] == ref.seed_pick(X, chosen[:2], seed, 2)
        np.testing.assert_array_equal(cent, X[chosen])
        assert cluster.seed_uniform(seed, 1) == ref.seed_uniform(seed, 1)
    want = [ref.seed_first(5, 11)]   # identical rows: the lowest index not chosen yet
    for _ in range(3):
        want.append(min(i for i in range(5) if i not in want))
    np.testing.assert_array_equal(cluster.kmeans_seed_host(np.ones((5, 3)), 4, 11)[0], want)


# ---- the config section -------------------------------------------------------------------------
def test_clustering_config():
    from shallow_encoders.common.path import CONFIG_PATH
    from shallow_encoders.config_parser import load_config_dict
    from shallow_encoders.config_parser.core import GraphDownstreamClusteringConfig
    from tools.utils import setup_pipeline
    cc = GraphDownstreamClusteringConfig()
    assert (cc.enable, cc.n_clusters, cc.n_init, cc.max_iter, cc.seed, cc.backend) == \
        (False, 0, 1, 100, 0, 'device')

    def load(*overrides):
        raw = load_config_dict('sge_sg_karate_club', CONFIG_PATH, list(overrides))
        return setup_pipeline(raw, task='downstream-classification').downstream.clustering
    assert load().enable is False
    got = load('downstream.clustering.enable=true', 'downstream.clustering.n_clusters=4',
               'downstream.clustering.backend=host')
    assert (got.enable, got.n_clusters, got.backend) == (True, 4, 'host')
    for bad in ('backend=sklearn', 'n_clusters=-1', 'n_clusters=1025', 'n_init=0', 'max_iter=0'):
        with pytest.raises(ValueError):
            load(f'downstream.clustering.{bad}')
    with pytest.raises(KeyError):
        load('downstream.clustering.tolerance=1')
