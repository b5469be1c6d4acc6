"""Multi-label node classification on the GPU (csrc/dw_nodeclf.hip, graph/nodeclf.py): dw_node_ovr
against the float64 restatement over every instantiation and tail under both decision rules, the
mask's edge cases (bit 63, mask 0, the full mask, ties, padded classes, large logits), the joint
one-vs-rest fit against sklearn class by class, the experiment loop against sklearn on identical
partitions, and train + downstream tools on a multi-label edge list.

The bound: every float entry within 1e-10 * sum |terms| (test_gpu_nodeclf.py's bar), the 3 K
counts and the predictions exact, a rerun byte-identical."""
import os
import random

import numpy as np
import pytest
import torch

import nodeclf_ovr_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import nodeclf

pytestmark = pytest.mark.gpu

V = 50          # table rows: ids repeat
BOUND = 1e-10
RULES = {ref.THRESHOLD: 'threshold', ref.TOP_K: 'top_k'}


def _inputs(d, K, n, seed=0):
    """Random rows, ids, masks of 0 .. K labels (about two a sample) and coefficients."""
    rng = np.random.default_rng(1000 * d + 10 * K + seed)
    table = rng.normal(size=(V, d)).astype(np.float32)
    ids = rng.integers(0, V, n)
    Y = rng.random((n, K)) < min(2.0 / K, 0.5)
    coef = rng.normal(size=(K, d + 1)) / np.sqrt(d)
    return table, ids, ref.to_masks(Y), coef


def _run(table, ids, masks, coef, K, rule, dev, check=True, table_dev=None):
    t = torch.from_numpy(table).to(dev) if table_dev is None else table_dev
    i = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dev)
    m = torch.from_numpy(np.asarray(masks, dtype=np.int64)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).to(dev)
    pred = torch.full((len(ids),), -7, dtype=torch.int64, device=dev)
    out = nodeclf.ovr_sums(t, i, m, c, K, RULES[rule], pred=pred, check=check)
    return out.cpu().numpy(), pred.cpu().numpy()


def _assert_equal(got, pred, want, rule, what):
    """The float entries within the bound, the counts and the predictions exact."""
    f, sums = want.floats, want.sums[rule]
    err = np.abs(got[:f] - sums[:f])
    worst = float((err / np.maximum(want.mags[:f], 1e-300)).max())
    print(f'{what} {RULES[rule]}: worst |error| / sum|terms| {worst:.3g}')
    assert (err <= BOUND * want.mags[:f]).all(), what
    np.testing.assert_array_equal(got[f:], sums[f:], err_msg=str(what))
    np.testing.assert_array_equal(pred, want.pred[rule], err_msg=str(what))


def _check(table, ids, masks, coef, K, dev, what, margins=True, **kw):
    """Both rules against the restatement; returns {rule: (sums, pred)}."""
    want = ref.ovr_sums(table, ids, masks, coef, K)
    out = {}
    for rule in RULES:
        if margins:
            assert want.margin[rule] > 1e-9 * want.scale, (what, rule, want.margin, want.scale)
        out[rule] = _run(table, ids, masks, coef, K, rule, dev, **kw)
        _assert_equal(*out[rule], want, rule, what)
    return out


# ---- dw_node_ovr ------------------------------------------------------------------------------
@pytest.mark.parametrize('d,K', [(2, 1), (3, 3), (96, 7), (128, 16), (128, 17), (128, 47),
                                 (256, 64), (512, 5), (512, 64)])
def test_sums_and_predictions_equal_restatement(d, K, hip_device):
    for n in (1, 15, 17, 1000, 10_007):
        table, ids, masks, coef = _inputs(d, K, n)
        first = _check(table, ids, masks, coef, K, hip_device, (d, K, n))
        for rule, (got, pred) in first.items():
            again, pred2 = _run(table, ids, masks, coef, K, rule, hip_device)
            assert got.tobytes() == again.tobytes() and pred.tobytes() == pred2.tobytes()


def test_empty_input_writes_nothing(hip_device):
    table, ids, masks, coef = _inputs(8, 3, 0)
    got, pred = _run(table, ids, masks, coef, 3, ref.TOP_K, hip_device)
    assert got.shape == (3 * 9 + 1 + 9,) and not got.any() and pred.shape == (0,)


def test_bit_63_is_a_label_at_64_classes_and_out_of_range_at_63(hip_device):
    """Bit 63 is the sign bit of the int64 the mask travels in, and K = 64 leaves nothing to
    shift out: with 64 classes sample 7's bit 63 is counted and (its intercept is +50)
    predicted; with 63 the same mask is dropped and reported, the rest unchanged."""
    d, n = 20, 100
    table, ids, masks, coef = _inputs(d, 64, n)
    masks = masks & ((1 << 63) - 1)       # nobody has label 63 ...
    masks[7] |= -(1 << 63)                # ... but sample 7
    assert masks[7] < 0
    coef[63, d] = 50.0
    out = _check(table, ids, masks, coef, 64, hip_device, 'K = 64')
    for rule, (got, pred) in out.items():
        tp, n_pred, n_true = got[-3 * 64:].reshape(3, 64)
        assert n_true[63] == 1 and tp[63] == 1 and pred[7] < 0
        # above every other logit: predicted for everybody, or for everybody with a label
        assert n_pred[63] == (n if rule == ref.THRESHOLD else np.count_nonzero(masks))
    keep = np.arange(n) != 7
    want = ref.ovr_sums(table, ids[keep], masks[keep], coef[:63], 63)
    assert ref.ovr_sums(table, ids, masks, coef[:63], 63).sums[0].tobytes() == \
        want.sums[0].tobytes()
    for rule in RULES:
        with pytest.raises(IndexError):
            _run(table, ids, masks, coef[:63], 63, rule, hip_device)
        got, pred = _run(table, ids, masks, coef[:63], 63, rule, hip_device, check=False)
        assert pred[7] == 0
        _assert_equal(got, pred[keep], want, rule, 'K = 63')


@pytest.mark.parametrize('value', [-1, V, 2 ** 40])
def test_bad_id_is_dropped_and_reported(value, hip_device):
    d, K, n = 20, 4, 100
    table, ids, masks, coef = _inputs(d, K, n)
    ids = ids.copy()
    ids[7] = value
    keep = np.arange(n) != 7
    want = ref.ovr_sums(table, ids[keep], masks[keep], coef, K)
    for rule in RULES:
        with pytest.raises(IndexError):
            _run(table, ids, masks, coef, K, rule, hip_device)
        got, pred = _run(table, ids, masks, coef, K, rule, hip_device, check=False)
        assert pred[7] == 0
        _assert_equal(got, pred[keep], want, rule, ('id', value))
        # the status word itself, and pred = NULL
        t = torch.from_numpy(table).to(hip_device)
        st = torch.zeros(1, dtype=torch.int32, device=hip_device)
        ws = nodeclf.ovr_workspace(n, d, K, hip_device)
        out = torch.zeros(K * (d + 1) + 1 + 3 * K, dtype=torch.float64, device=hip_device)
        i_dev = torch.from_numpy(ids).to(hip_device)
        m_dev = torch.from_numpy(masks).to(hip_device)
        c_dev = torch.from_numpy(coef).to(hip_device)
        _native.call('dw_node_ovr', _native.ptr(t), V, d, _native.ptr(i_dev), _native.ptr(m_dev),
                     n, K, _native.ptr(c_dev), rule, _native.ptr(out), None, _native.ptr(ws),
                     ws.numel() * 8, _native.ptr(st), _native.stream(hip_device))
        assert int(st.item()) == _native.DW_S_BAD_INDEX
        np.testing.assert_array_equal(out.cpu().numpy(), got)   # pred = NULL changes no sum


@pytest.mark.parametrize('K', [5, 64])
def test_mask_0_predicts_nothing_and_the_full_mask_everything_under_top_k(K, hip_device):
    d, n = 24, 300
    table, ids, masks, coef = _inputs(d, K, n)
    masks[0::3] = 0
    masks[1::3] = -1 if K == 64 else (1 << K) - 1
    out = _check(table, ids, masks, coef, K, hip_device, ('empty and full', K))
    pred = out[ref.TOP_K][1]
    assert not pred[0::3].any() and (pred[1::3] == masks[1]).all()
    tp, n_pred, n_true = out[ref.TOP_K][0][-3 * K:].reshape(3, K)
    assert n_pred.sum() == n_true.sum() and (n_true >= 100).all()


def test_ties_go_to_the_lowest_class(hip_device):
    """Rows 0 and 1 identical, row 2 their negative, one label per sample: the top-1 class is 0
    or 2, never 1."""
    d, n = 16, 400
    table, ids, masks, coef = _inputs(d, 3, n)
    masks[:] = 1 << (np.arange(n) % 3)
    coef[1] = coef[0]
    coef[2] = -coef[0]
    out = _check(table, ids, masks, coef, 3, hip_device, 'ties', margins=False)
    z0 = table[ids].astype(np.float64) @ coef[0, :d] + coef[0, d]
    assert np.abs(z0).min() > 1e-9
    pred = out[ref.TOP_K][1]
    np.testing.assert_array_equal(pred, np.where(z0 > 0, 0b001, 0b100))
    assert (pred == 1).any() and (pred == 4).any()


@pytest.mark.parametrize('K', [3, 17])
def test_padded_classes_take_no_part(K, hip_device):
    """Every intercept -50: a padded logit of 0 would be above every class's, so it would be
    predicted by the threshold's neighbour z >= 0 and push real classes out of the top k."""
    d, n = 24, 300
    table, ids, masks, coef = _inputs(d, K, n)
    coef[:, d] = -50.0
    out = _check(table, ids, masks, coef, K, hip_device, ('padded', K))
    assert not out[ref.THRESHOLD][1].any()
    top = out[ref.TOP_K][1]
    assert (top >> K == 0).all()
    np.testing.assert_array_equal(ref.bits(top, K).sum(axis=1), ref.bits(masks, K).sum(axis=1))


def test_large_logits_stay_finite(hip_device):
    d, K, n = 32, 5, 500
    table, ids, masks, coef = _inputs(d, K, n)
    z = table[ids].astype(np.float64) @ coef[:, :d].T + coef[:, d]
    coef *= 1000.0 / np.abs(z).max()
    want = ref.ovr_sums(table, ids, masks, coef, K)
    assert want.scale >= 1000.0
    out = _check(table, ids, masks, coef, K, hip_device, 'range')
    got = out[ref.THRESHOLD][0]
    assert np.isfinite(got).all() and got[K * (d + 1)] > 1000.0


@pytest.mark.parametrize('d', [7, 128, 130])
def test_unaligned_table_and_odd_dim(d, hip_device):
    """A table view offset by one float (4-B aligned only) gives the sums of the aligned copy's
    restatement; d = 7 and 130 are no multiples of 4."""
    K, n = 6, 700
    table, ids, masks, coef = _inputs(d, K, n)
    buf = torch.zeros(V * d + 1, dtype=torch.float32, device=hip_device)
    view = buf[1:].view(V, d)
    view.copy_(torch.from_numpy(table))
    assert view.data_ptr() % 16 == 4
    _check(table, ids, masks, coef, K, hip_device, ('offset', d), table_dev=view)
    _check(table, ids, masks, coef, K, hip_device, ('aligned', d))


# ---- NodeOvRLogisticRegression ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['m3', 'm7'])
def test_fit_on_device_reaches_sklearns_objective_in_every_class(name, hip_device):
    """The CPU test's problems with the kernel as the closure: no class's objective may exceed
    sklearn's (margin 0), and predict under the threshold rule at sklearn's own coefficients
    equals OneVsRestClassifier.predict entry for entry."""
    n, d, K = ref.PROBLEMS[name]
    table, ids, masks = ref.problem(name)
    X, Y = table[ids].astype(np.float64), ref.bits(masks, K)
    t_dev = torch.from_numpy(table.copy()).to(hip_device)
    i_dev = torch.from_numpy(ids.copy()).to(hip_device)
    clf = nodeclf.NodeOvRLogisticRegression().fit(t_dev, i_dev, masks, K)
    assert list(clf.classes_) == list(range(K)) and clf.n_labels_ == K
    ours = ref.class_objectives(X, Y, clf.full_coef())
    sk, rows, theirs = ref.sklearn_fit(name)
    gap = (ours - theirs) / theirs
    print(f'{name}: worst class gap {gap.max():.3g}, {clf.n_iter_} iterations')
    assert (ours <= theirs).all(), gap
    assert abs(clf.objective_ - ours.sum()) <= 1e-10 * ours.sum()
    # sklearn's own coefficients through the kernel
    at = nodeclf.NodeOvRLogisticRegression()
    at.coef_, at.intercept_ = rows[:, :d].copy(), rows[:, d].copy()
    at.classes_, at.n_labels_ = np.arange(K), K
    want = ref.ovr_sums(table, ids, masks, at.full_coef(), K)
    assert want.margin[ref.THRESHOLD] > 1e-9 * want.scale
    pred = at.predict(t_dev, i_dev, rule='threshold').cpu().numpy()
    np.testing.assert_array_equal(ref.bits(pred, K), sk.predict(X).astype(bool))
    with pytest.raises(ValueError, match='top-k rule needs'):
        at.predict(t_dev, i_dev)


def test_fit_leaves_constant_classes_out(hip_device):
    """Classes 1 and 4 of m7 emptied: they are not fitted and never predicted; their true labels
    at prediction time are false negatives of their class and do not count towards k."""
    n, d, K = ref.PROBLEMS['m7']
    table, ids, masks = ref.problem('m7')
    gone = (1 << 1) | (1 << 4)
    train = masks & ~gone
    t_dev = torch.from_numpy(table.copy()).to(hip_device)
    i_dev = torch.from_numpy(ids.copy()).to(hip_device)
    clf = nodeclf.NodeOvRLogisticRegression().fit(t_dev, i_dev, train, K)
    assert list(clf.classes_) == [0, 2, 3, 5, 6] and clf.coef_.shape == (5, d)
    for rule in ('threshold', 'top_k'):
        pred = clf.predict(t_dev, i_dev, masks, rule).cpu().numpy()
        assert not (pred & gone).any() and (pred & ~gone).any()
        tp, n_pred, n_true = clf.counts(t_dev, i_dev, masks, rule)
        P, Y = ref.bits(pred, K), ref.bits(masks, K)
        np.testing.assert_array_equal([tp, n_pred, n_true], [(P & Y).sum(0), P.sum(0), Y.sum(0)])
        assert n_true[1] > 0 and n_pred[1] == 0 and n_pred[4] == 0
        if rule == 'top_k':
            np.testing.assert_array_equal(P.sum(axis=1), ref.bits(train, K).sum(axis=1))
    with pytest.raises(ValueError, match='every training node has label 0'):
        clf.fit(t_dev, i_dev, masks | 1, K)


# ---- the experiment loop ----------------------------------------------------------------------
def _sklearn_scores(X, Y, split, n_exp, classifier_params=None):
    """Per experiment (micro, macro) F1 of OneVsRestClassifier(LogisticRegression()) with the
    top-k rule in numpy, on the partitions the device loop gets."""
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import f1_score
    from sklearn.multiclass import OneVsRestClassifier
    index, opaque = np.arange(len(X))[:, None], ref.to_masks(Y)
    scores = []
    for i in range(n_exp):
        split.random_state = i
        sp = split(index, opaque)
        tr, te = sp['X_train'][:, 0], sp['X_test'][:, 0]
        assert Y[tr].any(axis=0).all() and not Y[tr].all(axis=0).any()
        clf = OneVsRestClassifier(LogisticRegression(**(classifier_params or {})))
        clf.fit(X[tr], Y[tr].astype(np.int64))
        P = ref.top_k(clf.decision_function(X[te]).reshape(len(te), -1), Y[te].sum(axis=1))
        scores.append((f1_score(Y[te], P, average='micro', zero_division=0),
                       f1_score(Y[te], P, average='macro', zero_division=0)))
    return np.asarray(scores)


def _assert_paired(dev, host, what):
    for col, name in enumerate(('micro', 'macro')):
        diff = dev[:, col] - host[:, col]
        se = float(diff.std(ddof=1) / np.sqrt(len(diff)))
        print(f'{what} {name}-F1: device {dev[:, col].mean():.4f} vs sklearn '
              f'{host[:, col].mean():.4f}: paired difference {diff.mean():+.6f}, standard error '
              f'{se:.6f}, {int((diff != 0).sum())} of {len(diff)} experiments differ')
        assert abs(float(diff.mean())) <= 4.0 * se


def test_experiment_loop_agrees_with_sklearn_one_vs_rest(hip_device):
    """m7's table, 50 experiments per side on identical partitions: the mean micro-F1 and the
    mean macro-F1 each agree within 4 standard errors of the paired difference."""
    from shallow_encoders.split.core import TrainTestRatioSplit
    n, d, K = ref.PROBLEMS['m7']
    table, ids, masks = ref.problem('m7')
    n_exp = 50
    split = TrainTestRatioSplit(0.5)
    host = _sklearn_scores(table[ids].astype(np.float64), ref.bits(masks, K), split, n_exp)
    micro, macro, best, scores = nodeclf.node_multilabel_device(
        torch.from_numpy(table.copy()).to(hip_device), ids, masks, split, n_exp,
        device=hip_device, return_scores=True, n_classes=K)
    scores = np.asarray(scores)
    assert scores.shape == (n_exp, 2) and best == scores[:, 0].max()
    assert micro == pytest.approx(scores[:, 0].mean()) and macro == pytest.approx(
        scores[:, 1].mean())
    _assert_paired(scores, host, 'm7')


# ---- end to end -------------------------------------------------------------------------------
def test_train_and_downstream_tools_on_a_multilabel_edge_list(tmp_path, hip_device):
    """A planted-partition graph (4 communities x 40 nodes), node u labelled with its community
    and, when u is odd, with `odd`; the label file in the repeated-line form with 10 nodes
    withheld: tools/train.py, then the downstream tool with multilabel=true on the device. Its
    micro-F1 is above the prior-only classifier's (every node gets its k most frequent labels
    overall) and within 4 standard errors of sklearn one-vs-rest's on the same checkpoint and
    partitions over 20 experiments."""
    import networkx as nx
    from sklearn.metrics import f1_score
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    g = nx.planted_partition_graph(4, 40, 0.3, 0.01, seed=7)
    assert min(dict(g.degree).values()) > 0
    edges = tmp_path / 'edges.txt'
    edges.write_text(''.join(f'{u} {v}\n' for u, v in g.edges()))
    withheld = set(np.random.default_rng(0).choice(160, 10, replace=False).tolist())
    labels = tmp_path / 'group-edges.csv'
    labels.write_text('node,group\n' + ''.join(
        f'{u},c{u // 40}\n' + (f'{u},odd\n' if u % 2 else '')
        for u in range(160) if u not in withheld))
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_edge_list', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=ml', f'datamodule.additional_parameters.path={edges}',
            f'datamodule.additional_parameters.labels_path={labels}',
            'datamodule.additional_parameters.labels_skip_rows=1',
            'datamodule.additional_parameters.multilabel=true',
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
    ckpt = os.path.join(out, 'graph_edge_list', 'ml', 'checkpoints', 'last.ckpt')
    assert os.path.exists(ckpt)
    with pytest.raises(ValueError, match='backend=device'):
        downstream.main(base)
    dev = downstream.main(base + ['downstream.node_classification.backend=device'])
    assert set(dev) == {'node_micro_f1', 'node_macro_f1', 'node_best_micro_f1'}

    from shallow_encoders.common.path import CONFIG_PATH
    from shallow_encoders.config_parser import load_config_dict
    from tools.utils import setup_pipeline
    cfg = setup_pipeline(load_config_dict('sge_sg_edge_list', CONFIG_PATH, base[2:]),
                         task='downstream-classification')
    random.seed(0)
    dataset = cfg.datamodule.instantiate_dataset()
    rows, masks, classes = dataset.dataset.label_arrays()
    assert len(rows) == 150 and classes == ['c0', 'c1', 'c2', 'c3', 'odd']
    Y = ref.bits(masks, 5)
    assert set(Y.sum(axis=1)) == {1, 2}
    emb = downstream.load_input_embeddings(cfg, dataset, ckpt)
    nc = cfg.downstream.node_classification
    assert nc.prediction == 'top_k'
    split = nc.instantiate_split_algorithm()
    host = _sklearn_scores(emb.astype(np.float64)[rows], Y, split, 20, nc.classifier_params)
    _, _, _, scores = nodeclf.node_multilabel_device(
        torch.from_numpy(emb).to(hip_device), rows, masks, nc.instantiate_split_algorithm(), 20,
        classifier_params=nc.classifier_params, device=hip_device, return_scores=True,
        n_classes=5)
    scores = np.asarray(scores)
    assert scores[:, 0].mean() == pytest.approx(dev['node_micro_f1'])
    assert scores[:, 1].mean() == pytest.approx(dev['node_macro_f1'])
    assert scores[:, 0].max() == dev['node_best_micro_f1']
    _assert_paired(scores, host, 'planted partition')

    # the prior alone: every test node gets its k most frequent labels overall
    prior = []
    freq = np.broadcast_to(Y.sum(axis=0).astype(np.float64), Y.shape)
    index, opaque = np.arange(len(rows))[:, None], ref.to_masks(Y)
    for i in range(20):
        split.random_state = i
        te = split(index, opaque)['X_test'][:, 0]
        prior.append(f1_score(Y[te], ref.top_k(freq[te], Y[te].sum(axis=1)), average='micro',
                              zero_division=0))
    print(f'micro-F1 {dev["node_micro_f1"]:.4f} vs the prior alone {np.mean(prior):.4f}')
    assert dev['node_micro_f1'] > np.mean(prior)
