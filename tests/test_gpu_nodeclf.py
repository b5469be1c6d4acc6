"""Device node classification on the GPU (csrc/dw_nodeclf.hip, shallow_encoders/graph/nodeclf.py):
dw_node_softmax against the float64 restatement at a derived bound over every instantiation and
tail, the fitted classifier against sklearn, the experiment loop against the sklearn path on
identical partitions, and train + downstream tools on a labelled edge list.

The bound: every entry within 1e-10 * sum |terms| (the bar test_edge_logreg_equals_restatement
holds float64 sums to; n * 2^-53 at n = 10,007 is 1e-12)."""
import os
import random

import numpy as np
import pytest
import torch

import nodeclf_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import nodeclf

pytestmark = pytest.mark.gpu

V = 50          # table rows: ids repeat
BOUND = 1e-10


def _inputs(d, K, n, seed=0):
    rng = np.random.default_rng(1000 * d + 10 * K + seed)
    table = rng.normal(size=(V, d)).astype(np.float32)
    ids = rng.integers(0, V, n)
    y = rng.integers(0, K, n)
    coef = rng.normal(size=(K, d + 1)) / np.sqrt(d)
    return table, ids, y, coef


def _run(table, ids, y, coef, K, dev, check=True, table_dev=None):
    t = torch.from_numpy(table).to(dev) if table_dev is None else table_dev
    i = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dev)
    l = torch.from_numpy(np.asarray(y, dtype=np.int32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).to(dev)
    pred = torch.full((len(ids),), -7, dtype=torch.int32, device=dev)
    out = nodeclf.softmax_sums(t, i, l, c, K, pred=pred, check=check)
    return out.cpu().numpy(), pred.cpu().numpy()


def _assert_equal(got, pred, want, mags, want_pred, what):
    err = np.abs(got[:-1] - want[:-1])
    worst = float((err / np.maximum(mags[:-1], 1e-300)).max())
    print(f'{what}: worst |error| / sum|terms| {worst:.3g}')
    assert (err <= BOUND * mags[:-1]).all(), what
    assert got[-1] == want[-1], what
    np.testing.assert_array_equal(pred, want_pred, err_msg=str(what))


# ---- dw_node_softmax --------------------------------------------------------------------------
@pytest.mark.parametrize('d,K', [(2, 2), (3, 3), (96, 7), (128, 16), (128, 17), (128, 47),
                                 (256, 64), (512, 5), (512, 64)])
def test_sums_equal_restatement(d, K, hip_device):
    for n in (1, 15, 17, 1000, 10_007):
        table, ids, y, coef = _inputs(d, K, n)
        want, mags, want_pred, (gap, scale) = ref.softmax_sums(table, ids, y, coef, K)
        assert gap > 1e-9 * scale, (d, K, n, gap, scale)
        got, pred = _run(table, ids, y, coef, K, hip_device)
        _assert_equal(got, pred, want, mags, want_pred, (d, K, n))
        again, pred2 = _run(table, ids, y, coef, K, hip_device)
        assert got.tobytes() == again.tobytes() and pred.tobytes() == pred2.tobytes()


def test_empty_input_writes_nothing(hip_device):
    table, ids, y, coef = _inputs(8, 3, 0)
    got, pred = _run(table, ids, y, coef, 3, hip_device)
    assert not got.any() and pred.shape == (0,)


@pytest.mark.parametrize('K', [3, 17])
def test_padded_classes_take_no_part(K, hip_device):
    """Every intercept -50: a padded logit of 0 would win the max and swallow the sum."""
    d, n = 24, 300
    table, ids, y, coef = _inputs(d, K, n)
    coef[:, d] = -50.0
    want, mags, want_pred, (gap, scale) = ref.softmax_sums(table, ids, y, coef, K)
    assert gap > 1e-9 * scale
    got, pred = _run(table, ids, y, coef, K, hip_device)
    assert pred.max() < K
    _assert_equal(got, pred, want, mags, want_pred, ('padded', K))


def test_large_logits_stay_finite(hip_device):
    d, K, n = 32, 5, 500
    table, ids, y, coef = _inputs(d, K, n)
    z = table[ids].astype(np.float64) @ coef[:, :d].T + coef[:, d]
    coef *= 1000.0 / np.abs(z).max()
    want, mags, want_pred, (gap, scale) = ref.softmax_sums(table, ids, y, coef, K)
    assert scale >= 1000.0 and gap > 1e-9 * scale
    got, pred = _run(table, ids, y, coef, K, hip_device)
    assert np.isfinite(got).all() and got[-2] > 1000.0
    _assert_equal(got, pred, want, mags, want_pred, 'range')


def test_ties_go_to_the_lowest_class(hip_device):
    """Rows 0 and 1 identical, row 2 their negative: a sample's argmax is 0 or 2, never 1."""
    d, n = 16, 400
    table, ids, y, coef = _inputs(d, 3, n)
    coef[1] = coef[0]
    coef[2] = -coef[0]
    _, pred = _run(table, ids, y, coef, 3, hip_device)
    z0 = table[ids].astype(np.float64) @ coef[0, :d] + coef[0, d]
    assert np.abs(z0).min() > 1e-9
    np.testing.assert_array_equal(pred, np.where(z0 > 0, 0, 2))
    assert (pred == 0).any() and (pred == 2).any()


@pytest.mark.parametrize('d', [7, 128, 130])
def test_unaligned_table_and_odd_dim(d, hip_device):
    """A table view offset by one float (4-B aligned only) gives the sums of the aligned copy's
    restatement; d = 7 and 130 are no multiples of 4."""
    K, n = 6, 700
    table, ids, y, coef = _inputs(d, K, n)
    want, mags, want_pred, _ = ref.softmax_sums(table, ids, y, coef, K)
    buf = torch.zeros(V * d + 1, dtype=torch.float32, device=hip_device)
    view = buf[1:].view(V, d)
    view.copy_(torch.from_numpy(table))
    assert view.data_ptr() % 16 == 4
    got, pred = _run(table, ids, y, coef, K, hip_device, table_dev=view)
    _assert_equal(got, pred, want, mags, want_pred, ('offset', d))
    got, pred = _run(table, ids, y, coef, K, hip_device)
    _assert_equal(got, pred, want, mags, want_pred, ('aligned', d))


@pytest.mark.parametrize('what,value', [('id', -1), ('id', V), ('id', 2 ** 40), ('label', -1),
                                        ('label', 'K')])
def test_bad_input_is_dropped_and_reported(what, value, hip_device):
    d, K, n = 20, 4, 100
    table, ids, y, coef = _inputs(d, K, n)
    ids, y = ids.copy(), y.copy()
    (ids if what == 'id' else y)[7] = K if value == 'K' else value
    keep = np.arange(n) != 7
    want, mags, want_pred, _ = ref.softmax_sums(table, ids[keep], y[keep], coef, K)
    with pytest.raises(IndexError):
        _run(table, ids, y, coef, K, hip_device)
    got, pred = _run(table, ids, y, coef, K, hip_device, check=False)
    assert pred[7] == -1
    _assert_equal(got, pred[keep], want, mags, want_pred, (what, value))
    # the status word itself
    t = torch.from_numpy(table).to(hip_device)
    st = torch.zeros(1, dtype=torch.int32, device=hip_device)
    ws = nodeclf.softmax_workspace(n, d, K, hip_device)
    out = torch.zeros(K * (d + 1) + 2, dtype=torch.float64, device=hip_device)
    i_dev = torch.from_numpy(ids).to(hip_device)
    l_dev = torch.from_numpy(y.astype(np.int32)).to(hip_device)
    c_dev = torch.from_numpy(coef).to(hip_device)
    _native.call('dw_node_softmax', _native.ptr(t), V, d, _native.ptr(i_dev), _native.ptr(l_dev),
                 n, K, _native.ptr(c_dev), _native.ptr(out), None, _native.ptr(ws),
                 ws.numel() * 8, _native.ptr(st), _native.stream(hip_device))
    assert int(st.item()) == _native.DW_S_BAD_INDEX
    np.testing.assert_array_equal(out.cpu().numpy(), got)   # pred = NULL changes no sum


# ---- NodeLogisticRegression -------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k2', 'k7'])
def test_fit_on_device_reaches_sklearns_objective(name, hip_device):
    """The CPU test's problems with the kernel as the closure: the objective may not exceed
    sklearn's (margin 0), and predict at sklearn's own coefficients equals sklearn.predict on
    every sample, so score equals sklearn's."""
    n, d, K = ref.PROBLEMS[name]
    table, ids, y = ref.problem(name)
    X = table[ids].astype(np.float64)
    t_dev = torch.from_numpy(table.copy()).to(hip_device)
    i_dev = torch.from_numpy(ids.copy()).to(hip_device)
    clf = nodeclf.NodeLogisticRegression().fit(t_dev, i_dev, y)
    free = np.concatenate([clf.coef_, clf.intercept_[:, None]], axis=1)
    ours = ref.objective(X, y, free)
    sk, theirs = ref.sklearn_fit(name)
    print(f'{name}: objective {ours!r} vs sklearn {theirs!r}, gap '
          f'{(ours - theirs) / theirs:.3g}, {clf.n_iter_} iterations')
    assert ours <= theirs
    assert abs(clf.objective_ - ours) <= 1e-10 * ours
    assert list(clf.classes_) == list(range(K))
    # sklearn's own coefficients through the kernel
    at = nodeclf.NodeLogisticRegression()
    at.coef_, at.intercept_ = sk.coef_.copy(), sk.intercept_.copy()
    at.n_classes_, at.classes_ = K, np.arange(K)
    _, _, _, (gap, scale) = ref.softmax_sums(table, ids, y, at.full_coef(), K)
    assert gap > 1e-9 * scale
    np.testing.assert_array_equal(at.predict(t_dev, i_dev).cpu().numpy(), sk.predict(X))
    assert at.score(t_dev, i_dev, y) == sk.score(X, y)


def test_fit_maps_the_classes_present(hip_device):
    """As sklearn does, the fitted classes are those of the training labels."""
    table, ids, y = ref.problem('k7')
    keep = np.isin(y, (1, 4, 6))
    t_dev = torch.from_numpy(table.copy()).to(hip_device)
    i_dev = torch.from_numpy(ids[keep]).to(hip_device)
    clf = nodeclf.NodeLogisticRegression().fit(t_dev, i_dev, y[keep])
    assert list(clf.classes_) == [1, 4, 6] and clf.coef_.shape == (3, 16)
    pred = clf.predict(t_dev, i_dev).cpu().numpy()
    assert set(pred) <= {1, 4, 6} and (pred == y[keep]).mean() > 0.9
    with pytest.raises(ValueError, match='at least 2 classes'):
        clf.fit(t_dev, i_dev[:5], np.ones(5))


# ---- the experiment loop ----------------------------------------------------------------------
def _graph_labels(which):
    """(itos, labels) of the karate club and the triplets datasets (graph/datasets.py)."""
    if which == 'karate':
        import networkx as nx
        g = nx.karate_club_graph()
        labels = {f'n{v + 1:02d}': ('1' if g.nodes[v]['club'] == 'Mr. Hi' else '2') for v in g}
    else:
        labels = {f'{p}{s}': str(i) for i, p in enumerate('abc') for s in '123'}
    return ['<unk>'] + sorted(labels), labels


@pytest.mark.parametrize('which', ['karate', 'triplets'])
def test_experiment_loop_agrees_with_the_sklearn_path(which, hip_device):
    """A fixed random table of d = 8, 100 experiments per backend on identical partitions: the
    mean accuracies agree within 4 standard errors of their paired difference."""
    from shallow_encoders.split.core import TrainTestRatioSplit
    from tools.graph_model_downstream_classification import (fit_and_score, labels_to_integers,
                                                             node_classification)
    itos, labels = _graph_labels(which)
    n_nodes = len(itos) - 1
    assert n_nodes == (34 if which == 'karate' else 9)
    emb = np.random.default_rng(4).normal(size=(n_nodes + 1, 8)).astype(np.float32)
    y = np.asarray(labels_to_integers([labels[v] for v in itos[1:]]), dtype=np.float32)
    assert len(set(y)) == (2 if which == 'karate' else 3)
    n_exp = 100
    split = TrainTestRatioSplit(0.5, stratify=True)
    X = emb.astype(np.float64)[1:]
    host = []
    for i in range(n_exp):
        split.random_state = i
        sp = split(X, y)
        host.append(fit_and_score(sp['X_train'], sp['y_train'], sp['X_test'], sp['y_test'])[1])
    host = np.asarray(host)
    assert node_classification(emb, itos, labels, split, n_exp)[0] == pytest.approx(host.mean())
    table = torch.from_numpy(emb).to(hip_device)
    mean, best, conf, accs = nodeclf.node_classification_device(
        table, np.arange(1, n_nodes + 1), y, split, n_exp, device=hip_device,
        return_accuracies=True)
    accs = np.asarray(accs)
    assert len(accs) == n_exp and mean == pytest.approx(accs.mean()) and best == accs.max()
    K = len(set(y))
    assert conf.shape == (K, K) and conf.sum() == len(split(X, y)['y_test'])
    assert np.trace(conf) / conf.sum() == pytest.approx(best)
    diff = accs - host
    se = float(diff.std(ddof=1) / np.sqrt(n_exp))
    print(f'{which}: device {accs.mean():.4f} vs sklearn {host.mean():.4f}: paired difference '
          f'{diff.mean():+.5f}, standard error {se:.5f}, {int((diff != 0).sum())} of {n_exp} '
          f'experiments differ')
    assert abs(float(diff.mean())) <= 4.0 * se


# ---- end to end -------------------------------------------------------------------------------
def test_train_and_downstream_tools_on_a_labelled_edge_list(tmp_path, hip_device):
    """A planted-partition graph (4 communities x 40 nodes) as an edge list plus a label file
    with 10 labels withheld: tools/train.py, then the downstream tool with the node task on the
    device. Its accuracy over the 150 labelled nodes is above 0.5 (twice chance) and within 4
    standard errors of the sklearn backend's on the same checkpoint over 20 experiments."""
    import networkx as nx
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    g = nx.planted_partition_graph(4, 40, 0.3, 0.01, seed=7)
    assert min(dict(g.degree).values()) > 0
    edges = tmp_path / 'edges.txt'
    edges.write_text(''.join(f'{u} {v}\n' for u, v in g.edges()))
    withheld = set(np.random.default_rng(0).choice(160, 10, replace=False).tolist())
    labels = tmp_path / 'labels.csv'
    labels.write_text('node,community\n' + ''.join(
        f'{u},c{u // 40}\n' for u in range(160) if u not in withheld))
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_edge_list', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=nc', f'datamodule.additional_parameters.path={edges}',
            f'datamodule.additional_parameters.labels_path={labels}',
            'datamodule.additional_parameters.labels_skip_rows=1',
            'datamodule.additional_parameters.walks_per_node=10',
            'datamodule.additional_parameters.walk_length=40',
            'datamodule.batch_size=64', 'model.embedding_size=16', 'train.optimizer.lr=0.05',
            'train.max_epochs=3',
            'downstream.edge_classification.enable=false',
            'downstream.node_classification.enable=true',
            'downstream.node_classification.visualize=false',
            'downstream.node_classification.n_experiments=20']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_edge_list', 'nc', 'checkpoints', 'last.ckpt'))
    dev = downstream.main(base + ['downstream.node_classification.backend=device'])
    assert set(dev) == {'node_accuracy', 'node_best', 'node_macro_f1'}
    host = downstream.main(base)
    assert set(host) == {'node_accuracy', 'node_best'}
    assert dev['node_accuracy'] > 0.5

    # the per-experiment accuracies behind the two means, on the same partitions
    from shallow_encoders.common.path import CONFIG_PATH
    from shallow_encoders.config_parser import load_config_dict
    from tools.utils import setup_pipeline
    cfg = setup_pipeline(load_config_dict('sge_sg_edge_list', CONFIG_PATH, base[2:]),
                         task='downstream-classification')
    random.seed(0)
    dataset = cfg.datamodule.instantiate_dataset()
    rows, y, classes = dataset.dataset.label_arrays()
    assert len(rows) == 150 and classes == ['c0', 'c1', 'c2', 'c3']
    emb = downstream.load_input_embeddings(
        cfg, dataset, os.path.join(out, 'graph_edge_list', 'nc', 'checkpoints', 'last.ckpt'))
    nc = cfg.downstream.node_classification
    split = nc.instantiate_split_algorithm()
    yf = y.astype(np.float32)
    X = emb.astype(np.float64)[rows]
    h = []
    for i in range(20):
        split.random_state = i
        sp = split(X, yf)
        h.append(downstream.fit_and_score(sp['X_train'], sp['y_train'], sp['X_test'],
                                          sp['y_test'], nc.classifier_params)[1])
    _, _, _, d = nodeclf.node_classification_device(
        torch.from_numpy(emb).to(hip_device), rows, yf, nc.instantiate_split_algorithm(), 20,
        classifier_params=nc.classifier_params, device=hip_device, return_accuracies=True)
    h, d = np.asarray(h), np.asarray(d)
    assert h.mean() == pytest.approx(host['node_accuracy'])
    assert d.mean() == pytest.approx(dev['node_accuracy'])
    diff = d - h
    se = float(diff.std(ddof=1) / np.sqrt(20))
    print(f'device {d.mean():.4f} vs sklearn {h.mean():.4f}: paired difference '
          f'{diff.mean():+.5f}, standard error {se:.5f}')
    assert abs(float(diff.mean())) <= 4.0 * se
