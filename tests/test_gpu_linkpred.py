"""Device link prediction on the GPU (csrc/dw_linkpred.hip, shallow_encoders/graph/linkpred.py):
the sampler against its restatement bit for bit, dw_edge_features against numpy float32 bit for
bit, dw_edge_logreg against the float64 restatement at a derived bound, the fitted classifier
against sklearn, the experiment loop against the sklearn path, and the downstream tool on a
``graph_rmat`` dataset."""
import os
import random

import numpy as np
import pytest
import torch

import linkpred_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import linkpred
from shallow_encoders.graph.csr import CSRGraph

pytestmark = pytest.mark.gpu


def _karate_csr():
    g, row_ptr, col, cs = ref.karate()
    return g, CSRGraph.from_networkx(g), row_ptr, cs


# ---- dw_negative_edges ------------------------------------------------------------------------
def _check_sampler(csr, row_ptr, cs, n, dev):
    V = len(row_ptr) - 1
    adj = np.zeros((V, V), dtype=bool)
    rows = np.repeat(np.arange(V), np.diff(row_ptr))
    adj[rows, cs] = True
    for seed, off in ((3, 0), (3, 2 ** 32 + 5)):
        got = linkpred.negative_edges(csr, n, seed, offset=off, device=dev)
        again = linkpred.negative_edges(csr, n, seed, offset=off, device=dev)
        assert got.dtype == torch.int64 and got.shape == (n, 2)
        assert torch.equal(got, again)
        got = got.cpu().numpy()
        np.testing.assert_array_equal(got, ref.negative_edges_fast(row_ptr, cs, 1, n, seed, off))
        assert got.min() >= 1 and got.max() < V
        assert not adj[got[:, 0], got[:, 1]].any()


def test_sampler_equals_restatement_on_karate(hip_device):
    _, csr, row_ptr, cs = _karate_csr()
    np.testing.assert_array_equal(csr.row_ptr, row_ptr)
    _check_sampler(csr, row_ptr, cs, 1000, hip_device)
    assert linkpred.negative_edges(csr, 0, 1, device=hip_device).shape == (0, 2)


def test_sampler_equals_restatement_on_rmat12(hip_device):
    from shallow_encoders.graph.rmat import rmat_graph
    csr = rmat_graph(12, 40_000, 0, device=hip_device)
    cs = ref.sorted_rows(csr.row_ptr, csr.host_col())
    _check_sampler(csr, csr.row_ptr, cs, 100_000, hip_device)


def test_sampler_refuses_a_repeated_neighbour(hip_device):
    dup = CSRGraph.from_arrays([0, 0, 2, 4, 4, 4], [2, 2, 1, 1])
    with pytest.raises(ValueError, match='same neighbour twice'):
        linkpred.negative_edges(dup, 4, 0, device=hip_device)


# ---- dw_edge_features -------------------------------------------------------------------------
def _table_pairs(V, d, n, seed):
    rng = np.random.default_rng(seed)
    table = rng.normal(size=(V, d)).astype(np.float32)
    pairs = rng.integers(0, V, size=(n, 2))
    return table, pairs


@pytest.mark.parametrize('d', [2, 3, 96, 128, 256, 512])
def test_edge_features_bit_for_bit(d, hip_device):
    for n in (1, 63, 1000):
        table, pairs = _table_pairs(50, d, n, seed=d + n)
        t_dev = torch.from_numpy(table).to(hip_device)
        p_dev = torch.from_numpy(pairs).to(hip_device)
        for op, name in enumerate(ref.OPS):
            got = linkpred.edge_embeddings_device(t_dev, p_dev, name).cpu().numpy()
            want = ref.features(table, op, pairs)
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_edge_features_misaligned_out_and_bad_id(hip_device):
    table, pairs = _table_pairs(50, 128, 63, seed=9)
    t_dev = torch.from_numpy(table).to(hip_device)
    p_dev = torch.from_numpy(pairs).to(hip_device)
    buf = torch.full((63 * 128 + 2,), -7.0, dtype=torch.float32, device=hip_device)
    out = buf[1:-1].view(63, 128)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    linkpred.edge_embeddings_device(t_dev, p_dev, 'weighted_l2', out=out)
    want = ref.features(table, 3, pairs)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert buf[0].item() == -7.0 and buf[-1].item() == -7.0
    # an id outside [0, V): DW_S_BAD_INDEX, that row zeros, the others untouched by it
    for bad in (50, -1, 2 ** 40):
        p_bad = pairs.copy()
        p_bad[5, 1] = bad
        p_bad_dev = torch.from_numpy(p_bad).to(hip_device)
        res = torch.full((63, 128), 3.0, dtype=torch.float32, device=hip_device)
        st = torch.zeros(1, dtype=torch.int32, device=hip_device)
        _native.call('dw_edge_features', _native.ptr(t_dev), 50, 128, 1, _native.ptr(p_bad_dev),
                     63, _native.ptr(res), _native.ptr(st), _native.stream(hip_device))
        assert int(st.item()) == _native.DW_S_BAD_INDEX
        res = res.cpu().numpy()
        want = ref.features(table, 1, pairs)
        want[5] = 0.0
        np.testing.assert_array_equal(res.view(np.uint32), want.view(np.uint32))
        with pytest.raises(IndexError):
            linkpred.edge_embeddings_device(t_dev, p_bad_dev, 'hadamard')


# ---- dw_edge_logreg ---------------------------------------------------------------------------
def _logreg_case(table, pairs, labels, op, coef, dev):
    """Device sums against the restatement: every sum within 1e-10 * sum |terms| (taken from the
    reference), the correct-count equal, two runs bit-identical."""
    want, mag, (min_z, max_wx) = ref.logreg_sums(table, op, pairs, labels, coef)
    assert min_z > 1e-9 * max_wx, 'a sample too close to z = 0 for an exact count'
    args = (torch.from_numpy(table).to(dev), op, torch.from_numpy(pairs).to(dev),
            torch.from_numpy(labels).to(dev), torch.from_numpy(coef).to(dev))
    a = linkpred.edge_logreg_sums(*args)
    b = linkpred.edge_logreg_sums(*args)
    assert torch.equal(a, b)
    got = a.cpu().numpy()
    d = table.shape[1]
    err = np.abs(got[:d + 2] - want[:d + 2])
    worst = float((err / np.maximum(mag[:d + 2], 1e-300)).max())
    assert (err <= 1e-10 * mag[:d + 2]).all(), f'relative error {worst:.3g} of sum |terms|'
    assert got[d + 2] == want[d + 2]
    return worst


@pytest.mark.parametrize('d', [2, 96, 128, 256])
def test_edge_logreg_equals_restatement(d, hip_device):
    worst = 0.0
    for n in (1, 65, 10_007):
        rng = np.random.default_rng(100 * d + n)
        table, pairs = _table_pairs(50, d, n, seed=d + n)   # 50 rows: ids repeat
        labels = rng.integers(0, 2, size=n).astype(np.uint8)
        coef = rng.normal(size=d + 1) / np.sqrt(d)
        for op in range(4):
            worst = max(worst, _logreg_case(table, pairs, labels, op, coef, hip_device))
    print(f'd = {d}: worst error {worst:.3g} of sum |terms| (bound 1e-10)')


@pytest.mark.parametrize('d', [64, 255, 511, 512])
def test_edge_logreg_other_launch_shapes(d, hip_device):
    """The launch shapes the issue's sizes do not reach: 16 lanes per sample (d <= 64), two 16-B
    chunks per lane (d > 256), and the scalar-row kernel's 4 and 8 chunks (d % 4 != 0)."""
    for n in (65, 1031):
        rng = np.random.default_rng(100 * d + n)
        table, pairs = _table_pairs(50, d, n, seed=d + n)
        labels = rng.integers(0, 2, size=n).astype(np.uint8)
        coef = rng.normal(size=d + 1) / np.sqrt(d)
        for op in range(4):
            _logreg_case(table, pairs, labels, op, coef, hip_device)


def test_edge_logreg_stable_at_large_z(hip_device):
    """coef scaled so that |z| reaches about 50: exp(-|z|), log1p and the two-sided sigmoid."""
    d, n = 128, 10_007
    rng = np.random.default_rng(1)
    table, pairs = _table_pairs(50, d, n, seed=2)
    labels = rng.integers(0, 2, size=n).astype(np.uint8)
    coef = rng.normal(size=d + 1)
    z = ref.features(table, 1, pairs).astype(np.float64) @ coef[:d] + coef[d]
    coef *= 50.0 / np.abs(z).max()
    z = ref.features(table, 1, pairs).astype(np.float64) @ coef[:d] + coef[d]
    assert 45.0 < np.abs(z).max() < 55.0
    _logreg_case(table, pairs, labels, 1, coef, hip_device)


def test_edge_logreg_unaligned_table_and_bad_id(hip_device):
    """A table view off the 16-B grid takes the scalar-row kernel (same contract); an id outside
    [0, V) sets DW_S_BAD_INDEX and counts as x = 0."""
    d, n = 96, 65
    rng = np.random.default_rng(4)
    table, pairs = _table_pairs(50, d, n, seed=5)
    labels = rng.integers(0, 2, size=n).astype(np.uint8)
    coef = rng.normal(size=d + 1) / np.sqrt(d)
    want, mag, _ = ref.logreg_sums(table, 2, pairs, labels, coef)
    buf = torch.zeros(50 * d + 1, dtype=torch.float32, device=hip_device)
    view = buf[1:].view(50, d)
    view.copy_(torch.from_numpy(table))
    assert view.data_ptr() % 16 == 4
    p_dev = torch.from_numpy(pairs).to(hip_device)
    l_dev = torch.from_numpy(labels).to(hip_device)
    c_dev = torch.from_numpy(coef).to(hip_device)
    got = linkpred.edge_logreg_sums(view, 2, p_dev, l_dev, c_dev).cpu().numpy()
    assert (np.abs(got[:d + 2] - want[:d + 2]) <= 1e-10 * mag[:d + 2]).all()
    assert got[d + 2] == want[d + 2]
    p_bad = pairs.copy()
    p_bad[7, 0] = 50
    zeroed = np.concatenate([table, np.zeros((1, d), np.float32)])
    p_ref = p_bad.copy()
    p_ref[7] = (50, 50)     # x = op(0, 0) = 0 for every operator
    want, mag, _ = ref.logreg_sums(zeroed, 2, p_ref, labels, coef)
    t_dev = torch.from_numpy(table).to(hip_device)
    pb_dev = torch.from_numpy(p_bad).to(hip_device)
    with pytest.raises(IndexError):
        linkpred.edge_logreg_sums(t_dev, 2, pb_dev, l_dev, c_dev)
    got = linkpred.edge_logreg_sums(t_dev, 2, pb_dev, l_dev, c_dev, check=False).cpu().numpy()
    assert (np.abs(got[:d + 2] - want[:d + 2]) <= 1e-10 * mag[:d + 2]).all()
    assert got[d + 2] == want[d + 2]


# ---- EdgeLogisticRegression -------------------------------------------------------------------
@pytest.mark.parametrize('op', range(4))
def test_fit_on_device_reaches_sklearns_objective(op, hip_device):
    """The CPU test's karate inputs and its one-sided bar (tests/test_linkpred.py:
    SKLEARN_MARGIN, set from the gap measured with the numpy closure), with the kernel as the
    closure; score() equals the float64 reference's correct-count at the fitted coefficients."""
    from test_linkpred import SKLEARN_MARGIN, sklearn_objective
    table, pairs, labels = ref.karate_problem()
    t32 = table.astype(np.float32)
    x64 = ref.features(t32, op, pairs).astype(np.float64)
    y = labels.astype(np.float64)
    t_dev = torch.from_numpy(t32).to(hip_device)
    p_dev = torch.from_numpy(pairs).to(hip_device)
    l_dev = torch.from_numpy(labels).to(hip_device)
    clf = linkpred.EdgeLogisticRegression(ref.OPS[op]).fit(t_dev, p_dev, l_dev)
    ours = ref.objective(x64, y, clf.full_coef())
    theirs = sklearn_objective(x64, y)
    print(f'{ref.OPS[op]}: objective {ours!r} vs sklearn {theirs!r}, gap '
          f'{(ours - theirs) / theirs:.3g}, {clf.n_iter_} iterations')
    assert ours <= theirs * (1.0 + SKLEARN_MARGIN)
    assert abs(clf.objective_ - ours) <= 1e-10 * ours
    want, _, (min_z, max_wx) = ref.logreg_sums(t32, op, pairs, labels, clf.full_coef())
    assert min_z > 1e-9 * max_wx
    assert clf.score(t_dev, p_dev, l_dev) == want[-1] / len(pairs)


# ---- the experiment loop and the tool ---------------------------------------------------------
def test_edge_classification_device_agrees_with_the_sklearn_path(hip_device):
    """Karate, test_downstream.py's random embeddings, 100 experiments each way: the two mean
    accuracies differ by at most 4 standard errors of their difference (computed from the two
    sets of per-experiment accuracies)."""
    from tools.graph_model_downstream_classification import edge_classification
    g, csr, _, _ = _karate_csr()
    stoi = {v: i + 1 for i, v in enumerate(sorted(g.nodes))}
    emb = np.random.default_rng(2).normal(size=(35, 8))
    n_exp = 100
    host = np.asarray([edge_classification(emb, g, stoi, 0.5, 1, 'hadamard', seed=s)[0]
                       for s in range(n_exp)])
    table = torch.from_numpy(emb.astype(np.float32)).to(hip_device)
    mean, best, accs = linkpred.edge_classification_device(
        table, csr, 0.5, n_exp, 'hadamard', seed=0, device=hip_device, return_accuracies=True)
    accs = np.asarray(accs)
    assert len(accs) == n_exp and mean == pytest.approx(accs.mean()) and best == accs.max()
    assert 0.0 <= mean <= best <= 1.0
    se = float(np.sqrt(host.var(ddof=1) / n_exp + accs.var(ddof=1) / n_exp))
    diff = float(accs.mean() - host.mean())
    print(f'device {accs.mean():.4f} vs sklearn {host.mean():.4f}: difference {diff:+.4f}, '
          f'standard error {se:.4f}')
    assert abs(diff) <= 4.0 * se
    # the same seed gives the same experiments
    again = linkpred.edge_classification_device(table, csr, 0.5, 3, 'hadamard', seed=0,
                                                device=hip_device, return_accuracies=True)[2]
    assert again == list(accs[:3])


def test_downstream_tool_on_a_graph_rmat_dataset(tmp_path, hip_device):
    """tools/train.py then the downstream tool on a tiny graph_rmat (scale 8, 2,000 edge draws,
    one epoch): backend=device gives an edge accuracy; the default backend cannot read a CSR
    graph at all, which is why the device path exists."""
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
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
            'downstream.edge_classification.n_experiments=2']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_rmat', 'lp', 'checkpoints', 'last.ckpt'))
    res = downstream.main(base + ['downstream.edge_classification.backend=device'])
    assert set(res) == {'edge_accuracy', 'edge_best'}
    assert 0.0 <= res['edge_accuracy'] <= res['edge_best'] <= 1.0
    with pytest.raises(AttributeError):
        downstream.main(base)
