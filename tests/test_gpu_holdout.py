"""Held-out link prediction on the GPU (csrc/dw_holdout.hip, dw_edge_scores and dw_roc_auc in
csrc/dw_linkpred.hip): the device split against the host path bit for bit, the scores against a
float64 numpy restatement at the project's 1e-10 * sum |terms| bound, the AUC counts against the
integer restatement exactly, the protocol's guarantees, and both tools on a tiny graph."""
import os
import random

import numpy as np
import pytest
import torch

import holdout_ref as ref
import linkpred_ref as lref
from shallow_encoders import _native
from shallow_encoders.graph import linkpred
from shallow_encoders.graph.holdout import split_edges

pytestmark = pytest.mark.gpu

OPERATORS = ('average', 'hadamard', 'weighted_l1', 'weighted_l2')


# ---- 1. the split --------------------------------------------------------------------------------
GRAPHS = {'karate': lambda: ref.karate(False), 'karate_weighted': lambda: ref.karate(True),
          'rmat12': ref.rmat12, 'self_loops': ref.self_loops, 'star': ref.star, 'path': ref.path}


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_device_split_equals_host_split(name, hip_device):
    g = GRAPHS[name]()
    for ratio, seed in ((0.1, 0), (0.5, 1), (0.9, 2)):
        want, held_w, info_w = split_edges(g, ratio, seed)
        got, held, info = split_edges(g, ratio, seed, device=hip_device)
        again, held2, info2 = split_edges(g, ratio, seed, device=hip_device)
        assert info == info_w == info2
        assert held.dtype == torch.int64 and held.shape == (info['n_hold'], 2)
        np.testing.assert_array_equal(held.cpu().numpy(), held_w)
        np.testing.assert_array_equal(got.row_ptr, want.row_ptr)
        np.testing.assert_array_equal(got.host_col(), want.col)
        assert got.host_col().dtype == np.int32
        if want.weights is None:
            assert got.weights is None
        else:
            np.testing.assert_array_equal(got.weights.view(np.uint64),
                                          want.weights.view(np.uint64))
        assert torch.equal(held, held2) and np.array_equal(again.row_ptr, got.row_ptr)
        assert np.array_equal(again.host_col(), got.host_col())
    if name == 'star':
        assert info['n_hold'] == 0
    if name == 'path':
        assert 0 < info['n_hold'] < info['n_want']


def test_device_split_refuses_a_repeated_neighbour(hip_device):
    from shallow_encoders.graph.csr import CSRGraph
    dup = CSRGraph.from_arrays([0, 0, 2, 3, 4], [2, 2, 1, 1])
    with pytest.raises(ValueError, match='twice'):
        split_edges(dup, 0.5, 0, device=hip_device)


# ---- 2. dw_edge_scores ---------------------------------------------------------------------------
def _scores_ref(table, op, pairs, coef):
    """(z, sum |terms|) in float64 from the float32 operator values (linkpred_ref.features)."""
    x = lref.features(table, op, pairs).astype(np.float64)
    d = table.shape[1]
    w, b = (np.ones(d), 0.0) if coef is None else (coef[:d], coef[d])
    return x @ w + b, np.abs(x * w).sum(axis=1) + abs(b)


def _table_pairs(V, d, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((V, d)).astype(np.float32),
            rng.integers(0, V, size=(n, 2)).astype(np.int64))


@pytest.mark.parametrize('d', [1, 2, 3, 8, 128, 130, 512])
def test_edge_scores_equal_restatement(d, hip_device):
    worst = 0.0
    for n in (1, 5, 1003):
        table, pairs = _table_pairs(50, d, n, seed=7 * d + n)
        t_dev, p_dev = torch.from_numpy(table).to(hip_device), torch.from_numpy(pairs).to(hip_device)
        coef = np.random.default_rng(d + n).normal(size=d + 1) / np.sqrt(d)
        for op, name in enumerate(OPERATORS):
            for c in (None, coef):
                got = linkpred.edge_scores(t_dev, p_dev, name, c)
                assert got.dtype == torch.float64 and got.shape == (n,)
                assert torch.equal(got, linkpred.edge_scores(t_dev, p_dev, name, c))
                want, mag = _scores_ref(table, op, pairs, c)
                err = np.abs(got.cpu().numpy() - want)
                worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
                assert (err <= 1e-10 * mag).all()
    print(f'd = {d}: worst score error {worst:.3g} of sum |terms| (bound 1e-10)')


def test_edge_scores_unaligned_table_and_bad_id(hip_device):
    d, n = 128, 1003
    table, pairs = _table_pairs(50, d, n, seed=3)
    buf = torch.zeros(50 * d + 1, dtype=torch.float32, device=hip_device)
    view = buf[1:].view(50, d)
    view.copy_(torch.from_numpy(table))
    assert view.data_ptr() % 16 == 4
    p_dev = torch.from_numpy(pairs).to(hip_device)
    coef = np.random.default_rng(9).normal(size=d + 1) / np.sqrt(d)
    for op, name in enumerate(OPERATORS):
        want, mag = _scores_ref(table, op, pairs, coef)
        got = linkpred.edge_scores(view, p_dev, name, coef).cpu().numpy()
        assert (np.abs(got - want) <= 1e-10 * mag).all()
    # an id outside [0, V): the status bit, and the pair scores as x = 0 (the intercept alone)
    p_bad = pairs.copy()
    p_bad[7, 0] = 50
    pb_dev = torch.from_numpy(p_bad).to(hip_device)
    t_dev = torch.from_numpy(table).to(hip_device)
    with pytest.raises(IndexError):
        linkpred.edge_scores(t_dev, pb_dev, 'hadamard', coef)
    c_dev = torch.from_numpy(coef).to(hip_device)
    z = torch.full((n,), 7.0, dtype=torch.float64, device=hip_device)
    st = torch.zeros(1, dtype=torch.int32, device=hip_device)
    _native.call('dw_edge_scores', _native.ptr(t_dev), 50, d, 1, _native.ptr(pb_dev), n,
                 _native.ptr(c_dev), _native.ptr(z), _native.ptr(st), _native.stream(hip_device))
    assert int(st.item()) == _native.DW_S_BAD_INDEX
    want, mag = _scores_ref(table, 1, pairs, coef)
    want[7], mag[7] = coef[d], abs(coef[d])
    assert (np.abs(z.cpu().numpy() - want) <= 1e-10 * mag).all()
    assert float(z[7]) == coef[d]


# ---- 3. dw_roc_auc -------------------------------------------------------------------------------
def _auc_case(scores, labels, dev):
    s_dev = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64)).to(dev)
    l_dev = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)).to(dev)
    got = linkpred.roc_auc_counts(s_dev, l_dev)
    assert got == linkpred.roc_auc_counts(s_dev, l_dev)
    assert got == ref.u2_counts(scores, labels)
    return s_dev, l_dev, got


@pytest.mark.parametrize('n_pos,n_neg', [(1, 1), (3, 1000), (4097, 5000)])
def test_roc_auc_counts_equal_restatement(n_pos, n_neg, hip_device):
    rng = np.random.default_rng(n_pos + n_neg)
    labels = rng.permutation(np.r_[np.ones(n_pos), np.zeros(n_neg)]).astype(np.uint8)
    cont = rng.standard_normal(n_pos + n_neg) + labels
    for scores in (cont, np.round(2 * cont) / 2):     # continuous, and a few values with ties
        s_dev, l_dev, (u2, p, q) = _auc_case(scores, labels, hip_device)
        assert (p, q) == (n_pos, n_neg)
        assert linkpred.roc_auc(s_dev, l_dev) == u2 / (2 * p * q)


@pytest.mark.parametrize('case', ref.auc_cases(), ids=lambda c: c[0])
def test_roc_auc_tie_cases(case, hip_device):
    name, scores, labels = case
    s_dev, l_dev, _ = _auc_case(scores, labels, hip_device)
    auc = linkpred.roc_auc(s_dev, l_dev)
    if name in ('all_equal', 'signed_zeros'):
        assert auc == 0.5
    if name == 'separated':
        assert auc == 1.0
    if name == 'separated_reversed':
        assert auc == 0.0


def test_roc_auc_refusals(hip_device):
    s = torch.tensor([0.5, float('nan'), 1.0], dtype=torch.float64, device=hip_device)
    y = torch.tensor([1, 0, 0], dtype=torch.uint8, device=hip_device)
    with pytest.raises(ValueError, match='NaN'):
        linkpred.roc_auc(s, y)
    out = torch.zeros(3, dtype=torch.int64, device=hip_device)
    st = torch.zeros(1, dtype=torch.int32, device=hip_device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=hip_device)
    _native.call('dw_roc_auc', _native.ptr(s), _native.ptr(y), 3, _native.ptr(out),
                 _native.ptr(st), _native.ptr(ws), ws.numel(), _native.stream(hip_device))
    assert int(st.item()) == _native.DW_S_NAN_SCORE
    s = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64, device=hip_device)
    for labels in ([1, 1, 1], [0, 0, 0]):
        with pytest.raises(ValueError, match='at least one'):
            linkpred.roc_auc(s, torch.tensor(labels, dtype=torch.uint8, device=hip_device))


def test_roc_auc_of_device_scores_agrees_with_sklearn(hip_device):
    from sklearn.metrics import roc_auc_score
    table, pairs = _table_pairs(50, 16, 1003, seed=1)
    labels = np.random.default_rng(2).integers(0, 2, size=1003).astype(np.uint8)
    z = linkpred.edge_scores(torch.from_numpy(table).to(hip_device),
                             torch.from_numpy(pairs).to(hip_device), 'hadamard', None)
    got = linkpred.roc_auc(z, torch.from_numpy(labels).to(hip_device))
    assert abs(got - roc_auc_score(labels, z.cpu().numpy())) <= 1e-12


# ---- 4. the protocol -----------------------------------------------------------------------------
def test_heldout_protocol_on_rmat12(hip_device):
    full = ref.rmat12()
    train, held, info = split_edges(full, 0.5, 0)
    V = full.vocab_size
    table = torch.from_numpy(np.random.default_rng(0).standard_normal((V, 16)).astype(
        np.float32)).to(hip_device)
    rows = np.repeat(np.arange(V), np.diff(full.row_ptr))
    edge_keys = set((rows * V + full.col).tolist())
    t_rows = np.repeat(np.arange(V), np.diff(train.row_ptr))
    train_keys = set((t_rows * V + train.col).tolist())
    assert not train_keys & set((held[:, 0] * V + held[:, 1]).tolist())
    assert not train_keys & set((held[:, 1] * V + held[:, 0]).tolist())

    held_dev = torch.from_numpy(held).to(hip_device)
    train_pos = linkpred.positive_edges(train, hip_device, loops=False)
    n_train, n_test = train_pos.shape[0], held.shape[0]
    assert n_train == info['n_edges'] - info['n_hold'] and n_test == info['n_hold']
    ranges = []
    for i in range(2):
        x_tr, y_tr, x_te, y_te = linkpred.heldout_pairs(full, train_pos, held_dev, i, 0,
                                                        hip_device)
        assert int(y_te.sum()) == n_test and y_te.shape[0] == 2 * n_test     # balanced
        assert int(y_tr.sum()) == n_train and y_tr.shape[0] == 2 * n_train
        assert torch.equal(x_te[:n_test], held_dev) and torch.equal(x_tr[:n_train], train_pos)
        for neg in (x_tr[n_train:].cpu().numpy(), x_te[n_test:].cpu().numpy()):
            assert not edge_keys & set((neg[:, 0] * V + neg[:, 1]).tolist())
        a, b = linkpred.heldout_negative_offsets(i, n_train, n_test)
        np.testing.assert_array_equal(
            x_te[n_test:].cpu().numpy(),
            linkpred.negative_edges(full, n_test, 0, offset=b, device=hip_device).cpu().numpy())
        ranges += [(a, a + n_train), (b, b + n_test)]
    ranges.sort()
    assert all(r[1] <= s[0] for r, s in zip(ranges, ranges[1:]))             # disjoint offsets

    args = (table, full, train, held, 2, 'hadamard')
    res, aucs, accs = linkpred.heldout_edge_classification(
        *args, classifier_params={'max_iter': 20}, seed=0, return_experiments=True)
    again = linkpred.heldout_edge_classification(*args, classifier_params={'max_iter': 20},
                                                 seed=0)
    assert res == again
    assert set(res) == {'edge_auc', 'edge_auc_std', 'edge_accuracy', 'edge_best'}
    assert all(0.0 <= a <= 1.0 for a in aucs + accs) and res['edge_best'] == max(accs)
    dot, dot_aucs, _ = linkpred.heldout_edge_classification(*args, scorer='dot', seed=0,
                                                            return_experiments=True)
    for i in range(2):
        _, _, x_te, y_te = linkpred.heldout_pairs(full, train_pos, held_dev, i, 0, hip_device)
        assert dot_aucs[i] == linkpred.roc_auc(
            linkpred.edge_scores(table, x_te, 'hadamard', None), y_te)
    assert dot['edge_auc'] == float(np.mean(dot_aucs))
    with pytest.raises(ValueError, match='scorer'):
        linkpred.heldout_edge_classification(*args, scorer='cosine')


# ---- 5. the tools --------------------------------------------------------------------------------
def test_tools_on_a_graph_rmat_dataset_with_a_holdout(tmp_path, hip_device):
    """tools/train.py then the downstream tool on a tiny graph_rmat with holdout_ratio=0.3: both
    build the same split, the walks never step along a held edge, and protocol=heldout reports
    the four held-out keys."""
    from shallow_encoders.config_parser import load_config_dict
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    from tools.utils import setup_pipeline
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_cora', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=lp', 'datamodule.dataset_name=graph_rmat',
            'datamodule.additional_parameters.scale=8',
            'datamodule.additional_parameters.n_edges=2000',
            'datamodule.additional_parameters.graph_seed=0',
            'datamodule.additional_parameters.walks_per_node=1',
            'datamodule.additional_parameters.method_params.q=1',
            'datamodule.additional_parameters.rng=philox', 'train.noise=device',
            'model.embedding_size=128', 'train.optimizer.lr=0.01', 'train.max_epochs=1',
            'downstream.node_classification.enable=false',
            'downstream.edge_classification.n_experiments=2',
            'datamodule.additional_parameters.holdout_ratio=0.3']
    heldout = base + ['downstream.edge_classification.protocol=heldout',
                      'downstream.edge_classification.backend=device']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_rmat', 'lp', 'checkpoints', 'last.ckpt'))
    res = downstream.main(heldout)
    assert set(res) == {'edge_auc', 'edge_auc_std', 'edge_accuracy', 'edge_best'}
    assert 0.0 <= res['edge_auc'] <= 1.0 and 0.0 <= res['edge_accuracy'] <= res['edge_best'] <= 1.0

    def dataset(overrides):
        from shallow_encoders.common.path import CONFIG_PATH
        cfg = setup_pipeline(load_config_dict('sge_sg_cora', CONFIG_PATH, overrides[2:]),
                             task='downstream-classification')
        return cfg.datamodule.instantiate_dataset().dataset
    a, b = dataset(base), dataset(heldout)
    held = np.asarray(a.heldout_edges)
    assert len(held) == a.holdout_info['n_hold'] > 0
    np.testing.assert_array_equal(held, np.asarray(b.heldout_edges))
    np.testing.assert_array_equal(a.csr.row_ptr, b.csr.row_ptr)
    assert a.csr.vocab_size == a.full_csr.vocab_size and a.csr.nnz == a.full_csr.nnz - 2 * len(held)
    # one batch of walks against the held set
    V = a.csr.vocab_size
    walks = a.next_walk_batch(256).cpu().numpy().astype(np.int64)
    steps = np.stack([walks[:, :-1].ravel(), walks[:, 1:].ravel()], axis=1)
    keys = np.minimum(steps[:, 0], steps[:, 1]) * V + np.maximum(steps[:, 0], steps[:, 1])
    assert len(keys) > 0 and not set(keys.tolist()) & set((held[:, 0] * V + held[:, 1]).tolist())
    # without a holdout the protocol names the override to set
    plain = [o for o in heldout if 'holdout_ratio' not in o]
    with pytest.raises(ValueError, match='holdout_ratio'):
        downstream.main(plain)
