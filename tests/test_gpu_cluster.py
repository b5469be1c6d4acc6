"""Community detection on the GPU (csrc/dw_cluster.hip, shallow_encoders/graph/cluster.py):
dw_kmeans_step against the float64 restatement over every staging shape, both score splits and
both sides of the 64-cluster sums groups; dw_kmeans_seed against its law; dw_partition_counts and
dw_modularity_counts against plain loops; kmeans(device=...) against the host path; the tools on
a labelled edge list.

The bound: labels, counts and the changed count exactly, every float sum within
1e-10 * sum |terms| (test_gpu_nodeclf.py's bar). The random inputs must keep every sample's best
two scores further apart than twice that (asserted; no sample is skipped)."""
import os
import random

import numpy as np
import pytest
import torch

import cluster_ref as ref
import holdout_ref
from shallow_encoders import _native
from shallow_encoders.graph import cluster

pytestmark = pytest.mark.gpu

V = 50          # table rows: ids repeat
BOUND = 1e-10
GUARD = 8       # guard elements on either side of an output


def _inputs(d, K, n, seed=0):
    rng = np.random.default_rng(1000 * d + 10 * K + seed)
    table = rng.normal(size=(V, d)).astype(np.float32)
    ids = rng.integers(0, V, n)
    cent = rng.normal(size=(K, d))
    prev = rng.integers(0, K, n)
    return table, ids, cent, prev


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _run(table, ids, cent, prev, dev, check=True, table_dev=None):
    """(labels, out) as numpy, through guarded outputs whose guards must stay untouched."""
    t = torch.from_numpy(table).to(dev) if table_dev is None else table_dev
    i = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(cent, dtype=np.float64)).to(dev)
    p = None if prev is None else torch.from_numpy(np.asarray(prev, dtype=np.int32)).to(dev)
    n, (K, d) = len(ids), cent.shape
    lab_buf, lab = _guarded(n, torch.int32, -7, dev)
    out_buf, out = _guarded(K * (d + 1) + 2, torch.float64, -7.0, dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = cluster.step_workspace(n, d, K, dev)
    _native.call('dw_kmeans_step', _native.ptr(t), t.shape[0], d, _native.ptr(i), n,
                 _native.ptr(c), K, _native.ptr(p), lab.data_ptr(), out.data_ptr(),
                 _native.ptr(ws), ws.numel(), _native.ptr(st), _native.stream(dev))
    if check:
        _native.check_status(st, 'kmeans_step')
    for buf, fill in ((lab_buf, -7), (out_buf, -7.0)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all(), 'guard overwritten'
    return lab.cpu().numpy(), out.cpu().numpy(), int(st.item())


def _assert_equal(labels, out, want_labels, want, mags, d, K, what):
    np.testing.assert_array_equal(labels, want_labels, err_msg=str(what))
    exact = mags == 0          # the counts and the changed count
    np.testing.assert_array_equal(out[exact], want[exact], err_msg=str(what))
    err = np.abs(out - want)
    if (~exact).any():
        worst = float((err[~exact] / mags[~exact]).max())
        print(f'{what}: worst |error| / sum|terms| {worst:.3g}')
    assert (err <= BOUND * mags).all(), what


# ---- dw_kmeans_step -----------------------------------------------------------------------------
# K = 16 / 17: one centroid tile (the waves split the sample tiles) against two (they split the
# centroid tiles); K = 48 / 49: an idle wave against none; K = 64 / 65 and 128 / 129: both sides
# of the sums pass's cluster groups
@pytest.mark.parametrize('d,K', [(1, 1), (2, 2), (3, 17), (96, 16), (128, 64), (128, 65),
                                 (130, 7), (512, 3), (32, 1024), (20, 48), (20, 49), (8, 128),
                                 (8, 129), (512, 70)])
def test_step_equals_restatement(d, K, hip_device):
    for n in (1, 15, 16, 17, 1000, 4099):
        table, ids, cent, prev = _inputs(d, K, n)
        want_labels, want, mags, margins = ref.step(table, ids, cent, prev)
        assert margins.min() > 2 * BOUND, (d, K, n, margins.min())   # no sample skipped
        labels, out, _ = _run(table, ids, cent, prev, hip_device)
        _assert_equal(labels, out, want_labels, want, mags, d, K, (d, K, n))
        labels2, out2, _ = _run(table, ids, cent, prev, hip_device)
        assert out.tobytes() == out2.tobytes() and labels.tobytes() == labels2.tobytes()


def test_exact_ties_go_to_the_lowest_cluster(hip_device):
    """Small-integer rows and centroids, some centroids repeated: every product and sum is exact,
    so the device's labels and sums are the restatement's outright."""
    rng = np.random.default_rng(2)
    for d, K, n in ((4, 6, 300), (9, 40, 700), (16, 130, 1000)):
        table = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
        cent = rng.integers(-3, 4, size=(K, d)).astype(np.float64)
        cent[K // 2] = cent[0]
        cent[K - 1] = cent[1]
        cent[2] = cent[1]
        ids = rng.integers(0, V, n)
        want_labels, want, _, margins = ref.step(table, ids, cent)
        assert (margins == 0).any()
        labels, out, _ = _run(table, ids, cent, None, hip_device)
        np.testing.assert_array_equal(labels, want_labels)
        np.testing.assert_array_equal(out, want)
        assert not np.isin(labels, [K // 2, K - 1, 2]).any()


@pytest.mark.parametrize('d', [7, 128, 130])
def test_unaligned_table_and_odd_dim(d, hip_device):
    K, n = 6, 700
    table, ids, cent, prev = _inputs(d, K, n)
    want_labels, want, mags, _ = ref.step(table, ids, cent, prev)
    buf = torch.zeros(V * d + 1, dtype=torch.float32, device=hip_device)
    view = buf[1:].view(V, d)
    view.copy_(torch.from_numpy(table))
    assert view.data_ptr() % 16 == 4
    labels, out, _ = _run(table, ids, cent, prev, hip_device, table_dev=view)
    _assert_equal(labels, out, want_labels, want, mags, d, K, ('offset', d))


@pytest.mark.parametrize('K', [5, 70])
def test_empty_clusters_and_previous_labels(K, hip_device):
    d, n = 12, 500
    table, ids, cent, prev = _inputs(d, K, n)
    cent[1] = 1e3
    cent[K - 1] = -1e3          # never the nearest
    want_labels, want, mags, _ = ref.step(table, ids, cent, prev)
    labels, out, _ = _run(table, ids, cent, prev, hip_device)
    _assert_equal(labels, out, want_labels, want, mags, d, K, ('empty', K))
    rows = out[:K * (d + 1)].reshape(K, d + 1)
    assert not rows[1].any() and not rows[K - 1].any()
    # prev = NULL: everything counts as changed; prev = the labels themselves: nothing
    assert _run(table, ids, cent, None, hip_device)[1][-1] == n
    same_labels, same, _ = _run(table, ids, cent, labels, hip_device)
    assert same[-1] == 0 and same[:-1].tobytes() == out[:-1].tobytes()
    np.testing.assert_array_equal(same_labels, labels)


def test_empty_input_writes_nothing(hip_device):
    table, ids, cent, _ = _inputs(8, 3, 0)
    labels, out, st = _run(table, ids, cent, None, hip_device)
    assert labels.shape == (0,) and (out == -7.0).all() and st == 0
    lab, o = cluster.kmeans_step(torch.from_numpy(table).to(hip_device),
                                 torch.zeros(0, dtype=torch.int64, device=hip_device),
                                 torch.from_numpy(cent).to(hip_device))
    assert lab.shape == (0,) and not o.cpu().numpy().any()


@pytest.mark.parametrize('K', [4, 100])
@pytest.mark.parametrize('value', [-1, V, 2 ** 40])
def test_bad_ids_are_dropped_and_reported(value, K, hip_device):
    d, n = 20, 100
    table, ids, cent, prev = _inputs(d, K, n)
    ids = ids.copy()
    ids[7] = value
    ids[64] = value
    want_labels, want, mags, _ = ref.step(table, ids, cent, prev)
    assert want_labels[7] == -1 and want_labels[64] == -1
    labels, out, st = _run(table, ids, cent, prev, hip_device, check=False)
    assert st == _native.DW_S_BAD_INDEX
    _assert_equal(labels, out, want_labels, want, mags, d, K, ('bad id', value))
    with pytest.raises(IndexError):
        _run(table, ids, cent, prev, hip_device)


def test_step_refuses_bad_shapes(hip_device):
    t = torch.zeros((4, 8), device=hip_device)
    i = torch.zeros(3, dtype=torch.int64, device=hip_device)
    c = torch.zeros((2, 8), dtype=torch.float64, device=hip_device)
    with pytest.raises(ValueError):
        cluster.kmeans_step(t, i, c.float())
    with pytest.raises(ValueError):
        cluster.kmeans_step(t, i, torch.zeros((1025, 8), dtype=torch.float64, device=hip_device))
    with pytest.raises(ValueError):
        cluster.kmeans_step(torch.zeros((4, 513), device=hip_device), i,
                            torch.zeros((2, 513), dtype=torch.float64, device=hip_device))
    with pytest.raises(ValueError):
        cluster.kmeans_step(t, i, c, prev=torch.zeros(3, dtype=torch.int64, device=hip_device))
    with pytest.raises(_native.DWError):
        cluster.kmeans_step(t, i, c, workspace=torch.zeros(256, dtype=torch.uint8,
                                                           device=hip_device)[:16])


# ---- dw_kmeans_seed -----------------------------------------------------------------------------
def _seed(table, ids, K, seed, dev, check=True):
    chosen, cent = cluster.kmeans_seed(torch.from_numpy(table).to(dev),
                                       torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dev),
                                       K, seed, check=check)
    return chosen.cpu().numpy(), cent.cpu().numpy()


@pytest.mark.parametrize('d,K,n', [(3, 5, 40), (128, 64, 1000), (17, 300, 3000)])
def test_seed_indices_and_centroids(d, K, n, hip_device):
    rng = np.random.default_rng(d)
    table = rng.normal(size=(n, d)).astype(np.float32)   # n distinct rows
    ids = rng.permutation(n)
    chosen, cent = _seed(table, ids, K, 12345, hip_device)
    assert chosen.min() >= 0 and chosen.max() < n and len(set(chosen.tolist())) == K
    assert chosen[0] == ref.seed_first(n, 12345)
    np.testing.assert_array_equal(cent, table[ids[chosen]].astype(np.float64))
    again, cent2 = _seed(table, ids, K, 12345, hip_device)
    np.testing.assert_array_equal(chosen, again)
    assert cent.tobytes() == cent2.tobytes()
    other, _ = _seed(table, ids, K, 12346, hip_device)
    assert (other != chosen).any()


def test_seed_second_centre_follows_the_d2_law(hip_device):
    """64 points at integer coordinates (every D2 and partial sum exact, so the draw does not
    depend on the order of summation), 20,000 seeds: the second centre given the first equals the
    restatement's draw seed by seed, and a chi-square test holds the draws given each first
    centre pooled against the exact law at alpha = 1e-3 (tests/test_gpu_walk_law.py's level for
    one test)."""
    from scipy.stats import chi2
    rng = np.random.default_rng(4)
    n, n_seeds = 64, 20_000
    pts = rng.integers(-4, 5, size=(n, 2))
    table = pts.astype(np.float32)
    X = pts.astype(np.float64)
    ids = np.arange(n)
    t = torch.from_numpy(table).to(hip_device)
    i = torch.from_numpy(ids).to(hip_device)
    first = np.empty(n_seeds, dtype=np.int64)
    second = np.empty(n_seeds, dtype=np.int64)
    outs = [cluster.kmeans_seed(t, i, 2, seed, check=False)[0] for seed in range(n_seeds)]
    both = torch.stack(outs).cpu().numpy()
    first, second = both[:, 0], both[:, 1]
    for seed in range(0, n_seeds, 97):
        assert first[seed] == ref.seed_first(n, seed)
        assert second[seed] == ref.seed_pick(X, first[seed:seed + 1], seed, 1)
    # expected counts: sum over the seeds of the law given that seed's first centre
    laws = np.stack([ref.seed_law(X, [c]) for c in range(n)])
    expected = laws[first].sum(axis=0)
    counts = np.bincount(second, minlength=n).astype(np.float64)
    assert not counts[expected == 0].any()          # a point at distance 0 is never drawn
    keep = expected > 0
    assert expected[keep].min() >= 5
    stat = float(((counts[keep] - expected[keep]) ** 2 / expected[keep]).sum())
    pv = float(chi2.sf(stat, int(keep.sum()) - 1))
    print(f'second centre: {n_seeds} seeds, {int(keep.sum())} bins, chi2 {stat:.1f}, '
          f'p-value {pv:.3g}')
    assert pv > 1e-3


def test_seed_falls_back_on_identical_rows(hip_device):
    table = np.ones((9, 5), dtype=np.float32)
    for seed in (0, 1, 2, 3):
        chosen, cent = _seed(table, np.arange(9), 6, seed, hip_device)
        want = [ref.seed_first(9, seed)]
        for _ in range(5):
            want.append(min(i for i in range(9) if i not in want))
        np.testing.assert_array_equal(chosen, want)
        assert (cent == 1.0).all()
    # three distinct rows, five centres: the distinct ones first, then the lowest free indices
    table = np.repeat(np.array([[0.0], [5.0], [9.0]], dtype=np.float32), 4, axis=0)
    chosen, cent = _seed(table, np.arange(12), 5, 8, hip_device)
    assert len(set(chosen.tolist())) == 5
    assert set(cent[:3, 0].tolist()) == {0.0, 5.0, 9.0}
    taken = list(chosen[:3])
    for j in (3, 4):
        assert chosen[j] == min(i for i in range(12) if i not in taken)
        taken.append(chosen[j])


def test_seed_reports_bad_ids(hip_device):
    table = np.random.default_rng(0).normal(size=(20, 4)).astype(np.float32)
    ids = np.arange(20)
    ids[3] = 20
    with pytest.raises(IndexError):
        _seed(table, ids, 4, 0, hip_device)
    chosen, _ = _seed(table, ids, 19, 0, hip_device, check=False)
    assert len(set(chosen.tolist())) == 19
    with pytest.raises(ValueError):
        _seed(table, ids[:3], 4, 0, hip_device)


# ---- dw_partition_counts, dw_modularity_counts --------------------------------------------------
@pytest.mark.parametrize('Ka,Kb,n', [(1, 1, 10), (7, 5, 1000), (1024, 64, 20_000)])
def test_partition_counts_equal_restatement(Ka, Kb, n, hip_device):
    rng = np.random.default_rng(Ka)
    a = rng.integers(-1, Ka, n)
    b = rng.integers(-1, Kb, n)
    want = ref.contingency(a, b, Ka, Kb)
    got = cluster.contingency(torch.from_numpy(a).to(hip_device),
                              torch.from_numpy(b).to(hip_device), Ka, Kb)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cluster.contingency(a, b, Ka, Kb), want)
    assert cluster.nmi_from_table(got) == pytest.approx(cluster.nmi_from_table(want), abs=0)
    bad = torch.from_numpy(np.where(np.arange(n) == n // 2, Ka, a)).to(hip_device)
    with pytest.raises(IndexError):
        cluster.contingency(bad, torch.from_numpy(b).to(hip_device), Ka, Kb)


@pytest.mark.parametrize('graph', ['karate', 'rmat12', 'self_loops'])
def test_modularity_counts_equal_restatement(graph, hip_device):
    csr = {'karate': lambda: holdout_ref.karate(False), 'rmat12': holdout_ref.rmat12,
           'self_loops': holdout_ref.self_loops}[graph]()
    if graph == 'rmat12':
        assert int(csr.degree().max()) == 1035
    rng = np.random.default_rng(6)
    for K in (1, 5, 300):
        labels = rng.integers(-1, K, csr.vocab_size)
        labels[0] = -1
        want = ref.modularity_counts(csr.row_ptr, csr.host_col(), labels, K)
        got = cluster.modularity_counts(csr, torch.from_numpy(labels).to(hip_device), K)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(cluster.modularity_counts(csr, labels, K), want)
        assert cluster.modularity(csr, torch.from_numpy(labels).to(hip_device), K) == \
            cluster.modularity(csr, labels, K)
    bad = torch.from_numpy(np.full(csr.vocab_size, 7)).to(hip_device)
    with pytest.raises(IndexError):
        cluster.modularity_counts(csr, bad, 5)


# ---- kmeans(device=...) -------------------------------------------------------------------------
def _blobs(seed=0, n=400, d=8, k=4):
    rng = np.random.default_rng(seed)
    truth = np.arange(n) % k
    table = np.zeros((n + 1, d), dtype=np.float32)
    table[1:] = (100.0 * np.eye(k, d)[truth] + rng.standard_normal((n, d))).astype(np.float32)
    return table, np.arange(1, n + 1, dtype=np.int64), truth


def test_kmeans_on_device_equals_the_host_path(hip_device):
    table, ids, truth = _blobs()
    X = table[ids].astype(np.float64)
    init = X[[0, 1, 2, 3]]
    host = cluster.kmeans(table, ids, 4, init=init)
    dev = cluster.kmeans(table, ids, 4, init=init, device=hip_device)
    assert dev[0].dtype == torch.int64 and dev[0].device.type == 'cuda'
    np.testing.assert_array_equal(dev[0].cpu().numpy(), host[0])
    assert dev[3] == host[3]
    assert dev[2] == pytest.approx(host[2], rel=1e-10)
    np.testing.assert_allclose(dev[1], host[1], rtol=1e-10, atol=1e-10)
    assert cluster.nmi(torch.from_numpy(truth).to(hip_device), dev[0]) == 1.0
    # karate-sized tables: 34 rows, a few dimensions, from an explicit init
    rng = np.random.default_rng(3)
    for d, K in ((2, 2), (16, 4), (5, 34)):
        table = np.concatenate([np.zeros((1, d)), rng.normal(size=(34, d))]).astype(np.float32)
        ids = np.arange(1, 35)
        init = table[1:K + 1].astype(np.float64)
        host = cluster.kmeans(table, ids, K, init=init, max_iter=30)
        dev = cluster.kmeans(table, ids, K, init=init, max_iter=30, device=hip_device)
        np.testing.assert_array_equal(dev[0].cpu().numpy(), host[0])
        assert dev[3] == host[3]
        assert dev[2] == pytest.approx(host[2], rel=1e-10)


def test_kmeans_on_device_seeds_restarts_and_caps(hip_device):
    table, ids, truth = _blobs(seed=1)
    a = cluster.kmeans(table, ids, 4, n_init=4, seed=0, device=hip_device)
    b = cluster.kmeans(table, ids, 4, n_init=4, seed=0, device=hip_device)
    assert torch.equal(a[0], b[0]) and a[2] == b[2] and a[1].tobytes() == b[1].tobytes()
    assert cluster.nmi(truth, a[0].cpu().numpy()) == 1.0
    rnd = cluster.kmeans(table, ids, 4, init='random', n_init=2, seed=3, device=hip_device)
    host = cluster.kmeans(table, ids, 4, init='random', n_init=2, seed=3)
    np.testing.assert_array_equal(rnd[0].cpu().numpy(), host[0])
    X = table[ids].astype(np.float64)
    capped = cluster.kmeans(table, ids, 4, init=X[:4] * 0.01, max_iter=1, device=hip_device)
    assert capped[3] == 1
    lab = capped[0].cpu().numpy()
    assert capped[2] == pytest.approx(((X - capped[1][lab]) ** 2).sum(), rel=1e-9)


# ---- end to end ---------------------------------------------------------------------------------
def test_train_and_downstream_tools_report_the_clustering(tmp_path, hip_device):
    """A planted-partition graph (4 communities x 40 nodes) as an edge list plus a label file with
    10 labels withheld: tools/train.py, then the downstream tool with the clustering task on the
    device and on the host. Every key is reported; the communities are found well above chance."""
    import networkx as nx
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    g = nx.planted_partition_graph(4, 40, 0.3, 0.01, seed=7)
    edges = tmp_path / 'edges.txt'
    edges.write_text(''.join(f'{u} {v}\n' for u, v in g.edges()))
    withheld = set(np.random.default_rng(0).choice(160, 10, replace=False).tolist())
    labels = tmp_path / 'labels.csv'
    labels.write_text('node,community\n' + ''.join(
        f'{u},c{u // 40}\n' for u in range(160) if u not in withheld))
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_edge_list', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=km', f'datamodule.additional_parameters.path={edges}',
            f'datamodule.additional_parameters.labels_path={labels}',
            'datamodule.additional_parameters.labels_skip_rows=1',
            'datamodule.additional_parameters.walks_per_node=10',
            'datamodule.additional_parameters.walk_length=40',
            'datamodule.batch_size=64', 'model.embedding_size=16', 'train.optimizer.lr=0.05',
            'train.max_epochs=3',
            'downstream.edge_classification.enable=false',
            'downstream.node_classification.enable=false',
            'downstream.clustering.enable=true', 'downstream.clustering.n_init=4']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_edge_list', 'km', 'checkpoints', 'last.ckpt'))
    keys = {'cluster_inertia', 'cluster_modularity', 'cluster_iterations', 'cluster_nmi',
            'cluster_ari'}
    dev = downstream.main(base)
    assert set(dev) == keys
    host = downstream.main(base + ['downstream.clustering.backend=host'])
    assert set(host) == keys
    print(f'device {dev}\nhost {host}')
    assert dev['cluster_nmi'] > 0.5 and dev['cluster_modularity'] > 0.3
    assert dev['cluster_iterations'] >= 1 and dev['cluster_inertia'] > 0
    # unlabelled: the count must be named, and only the label-free keys are reported
    bare = [a for a in base if 'labels' not in a]
    with pytest.raises(ValueError, match='n_clusters'):
        downstream.main(bare)
    free = downstream.main(bare + ['downstream.clustering.n_clusters=4'])
    assert set(free) == {'cluster_inertia', 'cluster_modularity', 'cluster_iterations'}
    assert free['cluster_inertia'] == dev['cluster_inertia']   # the same table, K and seed
