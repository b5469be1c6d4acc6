"""Device node classification without a device (DESIGN.md "Device node classification"): the
restatement against its own finite differences, the L-BFGS driver on the restatement against
sklearn, the label files, the index-column split, the entry points' argument checks through
ctypes, and the config and tool wiring."""
import ctypes

import numpy as np
import pytest

import nodeclf_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import nodeclf
from shallow_encoders.graph.edge_list import read_node_labels


# ---- the restatement --------------------------------------------------------------------------
def test_restated_gradient_agrees_with_central_differences_of_its_loss():
    rng = np.random.default_rng(0)
    V, d, K, n = 20, 5, 4, 60
    table = rng.normal(size=(V, d)).astype(np.float32)
    ids = rng.integers(0, V, n)
    y = rng.integers(0, K, n)
    coef = rng.normal(size=(K, d + 1))
    sums, mags, pred, _ = ref.softmax_sums(table, ids, y, coef, K)
    grad = sums[:K * (d + 1)].reshape(K, d + 1)
    h = 1e-6
    for k in range(K):
        for j in range(d + 1):
            up, down = coef.copy(), coef.copy()
            up[k, j] += h
            down[k, j] -= h
            fd = (ref.softmax_sums(table, ids, y, up, K)[0][-2]
                  - ref.softmax_sums(table, ids, y, down, K)[0][-2]) / (2 * h)
            assert abs(fd - grad[k, j]) <= 1e-6 * max(1.0, mags[k * (d + 1) + j]), (k, j)
    X = table[ids].astype(np.float64)
    assert sums[-2] == pytest.approx(ref.loss_only(X, y, coef), rel=1e-14)
    np.testing.assert_array_equal(pred, (X @ coef[:, :d].T + coef[:, d]).argmax(axis=1))
    assert sums[-1] == (pred == y).sum()


def test_restatement_drops_a_sample_with_a_bad_id_or_label():
    rng = np.random.default_rng(1)
    table = rng.normal(size=(10, 3)).astype(np.float32)
    ids = np.asarray([1, 2, -1, 10, 3, 4])
    y = np.asarray([0, 1, 0, 1, 2, -1])
    coef = rng.normal(size=(2, 4))
    sums, _, pred, _ = ref.softmax_sums(table, ids, y, coef, 2)
    want, _, p2, _ = ref.softmax_sums(table, ids[:2], y[:2], coef, 2)
    np.testing.assert_array_equal(sums, want)
    assert list(pred[2:]) == [-1, -1, -1, -1] and list(pred[:2]) == list(p2)


# ---- the driver -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k2', 'k3', 'k7', 'k40'])
def test_driver_reaches_sklearns_objective(name):
    """fit_closure on the restatement against LogisticRegression() at its defaults; the final
    objective, recomputed in float64, may not exceed sklearn's (margin 0: the driver ends below
    sklearn's own stopping point on every problem). Measured (ours - sklearn) / sklearn:
    k2 (34, 8, 2) -5.2e-07, k3 (300, 8, 3) -2.9e-05, k7 (1000, 16, 7) -1.7e-03 and
    k40 (600, 128, 40) -6.6e-03 (sklearn stops at its 100 iterations on the last two)."""
    n, d, K = ref.PROBLEMS[name]
    table, ids, y = ref.problem(name)
    X = table[ids].astype(np.float64)
    clf = nodeclf.NodeLogisticRegression().fit_closure(ref.closure(name), d, K)
    rows = 1 if K == 2 else K
    assert clf.coef_.shape == (rows, d) and clf.intercept_.shape == (rows,)
    free = np.concatenate([clf.coef_, clf.intercept_[:, None]], axis=1)
    ours = ref.objective(X, y, free)
    sk, theirs = ref.sklearn_fit(name)
    assert sk.coef_.shape == clf.coef_.shape
    print(f'{name}: objective {ours!r} vs sklearn {theirs!r}, gap '
          f'{(ours - theirs) / theirs:.3g}, {clf.n_iter_} iterations')
    assert ours <= theirs
    assert abs(clf.objective_ - ours) <= 1e-10 * ours
    assert clf.full_coef().shape == (K, d + 1)
    if K == 2:
        assert not clf.full_coef()[0].any()


def test_driver_without_intercept_and_with_a_short_budget():
    n, d, K = ref.PROBLEMS['k3']
    table, ids, y = ref.problem('k3')
    X = table[ids].astype(np.float64)
    full = nodeclf.NodeLogisticRegression().fit_closure(ref.closure('k3'), d, K)
    flat = nodeclf.NodeLogisticRegression(fit_intercept=False).fit_closure(ref.closure('k3'), d, K)
    assert not flat.intercept_.any() and flat.coef_.any()
    assert flat.objective_ >= full.objective_
    short = nodeclf.NodeLogisticRegression(max_iter=2).fit_closure(ref.closure('k3'), d, K)
    assert short.n_iter_ <= 2 and short.objective_ > full.objective_
    two = nodeclf.NodeLogisticRegression(fit_intercept=False).fit_closure(ref.closure('k2'), 8, 2)
    assert two.intercept_.shape == (1,) and two.intercept_[0] == 0.0


def test_classifier_params_are_checked():
    clf = nodeclf.NodeLogisticRegression.from_params({'C': 2.0, 'max_iter': 7})
    assert clf.C == 2.0 and clf.max_iter == 7 and clf.fit_intercept and clf.tol == 1e-4
    with pytest.raises(ValueError, match=r"classifier_params \['penalty'\] are not supported by "
                                         r"the device backend"):
        nodeclf.NodeLogisticRegression.from_params({'penalty': 'l1'})
    with pytest.raises(ValueError, match='C must be positive'):
        nodeclf.NodeLogisticRegression(C=0)
    with pytest.raises(RuntimeError, match='fit first'):
        nodeclf.NodeLogisticRegression().full_coef()
    with pytest.raises(ValueError, match='n_classes'):
        nodeclf.NodeLogisticRegression().fit_closure(lambda c: c, 4, 65)


def test_macro_f1_equals_sklearns():
    from sklearn.metrics import confusion_matrix, f1_score
    rng = np.random.default_rng(3)
    t, p = rng.integers(0, 5, 200), rng.integers(0, 5, 200)
    assert nodeclf.macro_f1(confusion_matrix(t, p, labels=range(5))) == pytest.approx(
        f1_score(t, p, average='macro'))


# ---- label files ------------------------------------------------------------------------------
def _write(tmp_path, data: bytes, name='labels.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_label_lines(tmp_path):
    text = (b'node label\n'            # header, skipped by skip_rows
            b'# a comment\n'
            b'\n'
            b'   \t\n'
            b'% another\n'
            b'3 red\n'
            b'  17\t\tblue extra columns, ignored\r\n'
            b'000000000000000005,,green\n'
            b'2 7\n'
            b'999999999999999999 x,\n'
            b'4 a-b/c')                # no last newline
    ids, tokens = read_node_labels(_write(tmp_path, text), skip_rows=1)
    assert ids.dtype == np.int64
    assert list(ids) == [3, 17, 5, 2, 999999999999999999, 4]
    assert tokens == ['red', 'blue', 'green', '7', 'x', 'a-b/c']
    assert read_node_labels(_write(tmp_path, b'# nothing\n'))[1] == []


@pytest.mark.parametrize('bad', [b'-3 red', b'+3 red', b'3', b'3 ', b'3,,', b'red 3', b'3red x',
                                 b'1234567890123456789 x', b'3 re\rd', b'3.5 x'])
def test_label_file_names_the_malformed_line(tmp_path, bad):
    text = b'# head\n1 a\n\n' + bad + b'\n2 b\n'
    with pytest.raises(ValueError, match=r'line 4 is not a node label'):
        read_node_labels(_write(tmp_path, text))
    with pytest.raises(ValueError, match=r'line 4 '):   # CRLF and no last newline: same line
        read_node_labels(_write(tmp_path, b'# head\r\n1 a\r\n\r\n' + bad))


def test_label_file_refuses_a_repeated_id(tmp_path):
    with pytest.raises(ValueError, match=r'line 3 labels node 7 a second time'):
        read_node_labels(_write(tmp_path, b'7 a\n8 b\n007 a\n'))
    np.savez(tmp_path / 'dup.npz', node=np.asarray([4, 5, 4]), label=np.asarray([0, 1, 0]))
    with pytest.raises(ValueError, match='node 4 is labelled twice'):
        read_node_labels(str(tmp_path / 'dup.npz'))


def test_label_npz(tmp_path):
    np.savez(tmp_path / 'l.npz', node=np.asarray([9, 2, 5], dtype=np.int32),
             label=np.asarray([10, 2, 10]))
    ids, tokens = read_node_labels(str(tmp_path / 'l.npz'))
    assert list(ids) == [9, 2, 5] and ids.dtype == np.int64 and tokens == ['10', '2', '10']
    np.savez(tmp_path / 'f.npz', node=np.asarray([1, 2]), label=np.asarray([0.5, 1.0]))
    with pytest.raises(ValueError, match='integer arrays'):
        read_node_labels(str(tmp_path / 'f.npz'))


def test_edge_list_dataset_labels(tmp_path, caplog):
    """Partial labels, dropped non-node ids, the dict form, and label_arrays() numbered as
    labels_to_integers numbers the dict form."""
    import logging
    from shallow_encoders.graph.datasets import EdgeListDataset
    from tools.graph_model_downstream_classification import labels_to_integers
    edges = _write(tmp_path, b'1 2\n2 3\n3 10\n10 40\n40 1\n5 3\n', 'edges.txt')
    labels = _write(tmp_path, b'id,label\n40,b\n2,10\n77,b\n3,9\n1,b\n0,zz\n')
    kw = dict(walks_per_node=1, walk_length=4, path=edges, build='host', rng='philox')
    with caplog.at_level(logging.INFO):
        ds = EdgeListDataset(labels_path=labels, labels_skip_rows=1, **kw)
    assert ds.has_labels and ds.n_labels_dropped == 2
    assert sum('dropped 2 labelled ids' in r.getMessage() for r in caplog.records) == 1
    rows, y, classes = ds.label_arrays()
    # nodes 1 2 3 5 10 40 -> rows 1 .. 6; 5 and 10 carry no label
    assert rows.dtype == np.int64 and list(rows) == [1, 2, 3, 6]
    assert classes == ['10', '9', 'b'] and y.dtype == np.int32 and list(y) == [2, 0, 1, 2]
    assert ds.labels == {'n0000001': 'b', 'n0000002': '10', 'n0000003': '9', 'n0000040': 'b'}
    itos = ds.csr.itos
    vertices = [v for v in itos[1:] if v in ds.labels]
    assert [itos.index(v) for v in vertices] == list(rows)
    assert labels_to_integers([ds.labels[v] for v in vertices]) == list(y)
    plain = EdgeListDataset(**kw)
    assert not plain.has_labels and plain.n_labels_dropped == 0
    with pytest.raises(AssertionError):
        plain.labels


def test_host_node_classification_takes_the_labelled_vertices_only():
    from shallow_encoders.split.core import TrainTestRatioSplit
    from tools.graph_model_downstream_classification import node_classification
    rng = np.random.default_rng(0)
    itos = ['<unk>'] + [f'v{i:02d}' for i in range(30)]
    emb = rng.normal(size=(31, 4))
    emb[1:16] += 3.0
    labels = {v: ('a' if i < 15 else 'b') for i, v in enumerate(itos[1:])}
    split = TrainTestRatioSplit(0.5, stratify=True)
    full = node_classification(emb, itos, labels, split, 3)
    # unlabelled extra vertices (with misleading embeddings) change nothing
    itos2 = itos + ['w0', 'w1']
    emb2 = np.concatenate([emb, -50 * np.ones((2, 4))])
    assert node_classification(emb2, itos2, labels, split, 3) == full


# ---- the split --------------------------------------------------------------------------------
def test_index_column_split_equals_the_feature_split():
    from shallow_encoders.split.core import (TrainTestRatioSplit, TrainValTestRatioSplit,
                                             TrainValTestStratifiedNSamplesSplit)
    rng = np.random.default_rng(5)
    n = 90
    X = rng.normal(size=(n, 6))
    y = (np.arange(n) % 3).astype(np.float32)
    index = np.arange(n)[:, None]
    algos = [TrainTestRatioSplit(0.6, stratify=True), TrainTestRatioSplit(0.5, test_all=True),
             TrainValTestRatioSplit(0.5, 0.7), TrainValTestStratifiedNSamplesSplit(5, 3),
             TrainValTestStratifiedNSamplesSplit(4, 2, 6)]
    for algo in algos:
        for seed in range(5):
            algo.random_state = seed
            a = algo(X, y)
            algo.random_state = seed
            b = algo(index, y)
            assert set(a) == set(b)
            for part in ('train', 'val', 'test'):
                if f'X_{part}' not in a:
                    continue
                ix = b[f'X_{part}'][:, 0]
                np.testing.assert_array_equal(a[f'X_{part}'], X[ix])
                np.testing.assert_array_equal(a[f'y_{part}'], b[f'y_{part}'])
                np.testing.assert_array_equal(y[ix], b[f'y_{part}'])


# ---- the entry points' argument checks (no device call is made) -------------------------------
def _softmax(d=8, K=3, n=4, V=10, fake=None, ws_bytes=0):
    lib = _native.load()
    p = fake
    rc = lib.dw_node_softmax(p, V, d, p, p, n, K, p, p, None, p, ws_bytes, None, None)
    return rc, lib.dw_last_error_string()


def _workspace(n, d, K):
    lib = _native.load()
    nb = ctypes.c_size_t(0)
    rc = lib.dw_node_softmax_workspace_bytes(n, d, K, ctypes.byref(nb))
    return rc, int(nb.value)


@pytest.mark.parametrize('kw', [dict(d=0), dict(d=513), dict(K=1), dict(K=65), dict(n=-1),
                                dict(V=0), dict(V=2 ** 31)])
def test_abi_refuses_bad_sizes_before_the_pointers(kw):
    rc, err = _softmax(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert b'bad sizes' in err and b'null pointer' not in err, err
    if 'V' not in kw:
        args = dict(n=4, d=8, K=3)
        args.update(kw)
        assert _workspace(**args)[0] == _native.DW_E_INVALID_ARG


def test_abi_takes_the_limits_up_to_the_pointers():
    for kw in (dict(), dict(d=1, K=2), dict(d=512, K=64), dict(V=2 ** 31 - 1)):
        rc, err = _softmax(**kw)
        assert rc == _native.DW_E_INVALID_ARG and b'null pointer' in err, (kw, err)
        assert _softmax(n=0, **kw)[0] == _native.DW_OK
    assert _native.load().dw_node_softmax_workspace_bytes(4, 8, 3, None) == \
        _native.DW_E_INVALID_ARG


def test_abi_refuses_a_short_workspace():
    """Never-dereferenced non-null pointers: the size check comes before any launch."""
    rc, need = _workspace(1000, 128, 47)
    assert rc == _native.DW_OK
    # one partial row of K (d + 1) + 2 doubles per block, 64 samples a block at this dim
    assert need == 16 * (47 * 129 + 2) * 8
    assert _workspace(10 ** 6, 128, 47)[1] == 256 * (47 * 129 + 2) * 8
    assert _workspace(10 ** 6, 512, 64)[1] == 256 * (64 * 513 + 2) * 8
    assert _workspace(33, 512, 2)[1] == 2 * (2 * 513 + 2) * 8
    assert _workspace(0, 8, 2) == (_native.DW_OK, 1 * (2 * 9 + 2) * 8)
    rc, err = _softmax(d=128, K=47, n=1000, fake=64, ws_bytes=need - 8)
    assert rc == _native.DW_E_INVALID_ARG and b'workspace too small' in err, err


def test_wrapper_refuses_host_and_malformed_tensors():
    import torch
    table = torch.zeros(10, 8)
    ids = torch.zeros(4, dtype=torch.int64)
    y = torch.zeros(4, dtype=torch.int32)
    coef = torch.zeros(3, 9, dtype=torch.float64)
    with pytest.raises(ValueError, match='float32'):
        nodeclf.softmax_sums(table.double(), ids, y, coef, 3)
    with pytest.raises(ValueError, match='outside'):
        nodeclf.softmax_sums(torch.zeros(10, 513), ids, y, coef, 3)
    with pytest.raises(ValueError, match='n_classes'):
        nodeclf.softmax_sums(table, ids, y, coef, 1)
    with pytest.raises(ValueError, match='int64'):
        nodeclf.softmax_sums(table, ids.int(), y, coef, 3)
    with pytest.raises(ValueError, match='labels'):
        nodeclf.softmax_sums(table, ids, y.long(), coef, 3)
    with pytest.raises(ValueError, match='coef'):
        nodeclf.softmax_sums(table, ids, y, coef[:2], 3)
    with pytest.raises(ValueError, match='pred'):
        nodeclf.softmax_sums(table, ids, y, coef, 3, pred=torch.zeros(4))
    # host tensors never reach a kernel: no CPU fallback
    with pytest.raises((ValueError, _native.NativeLibraryError, _native.DWError)):
        nodeclf.softmax_sums(table, ids, y, coef, 3, workspace=torch.zeros(64, dtype=torch.float64))


# ---- config and tool --------------------------------------------------------------------------
def test_config_backend_is_validated():
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.config_parser.core import GraphDownstreamNodeClassificationConfig
    assert GraphDownstreamNodeClassificationConfig().backend == 'sklearn'
    assert GraphDownstreamNodeClassificationConfig(backend='device').backend == 'device'
    with pytest.raises(ValueError, match='node_classification.backend'):
        GraphDownstreamNodeClassificationConfig(backend='gpu')
    assert load_config('sge_sg_karate_club').downstream.node_classification.backend == 'sklearn'
    c = load_config('sge_sg_karate_club',
                    overrides=['downstream.node_classification.backend=device'])
    assert c.downstream.node_classification.backend == 'device'


def test_edge_list_config_carries_the_label_keys(tmp_path):
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.graph.datasets import EdgeListDataset
    c = load_config('sge_sg_edge_list')
    params = dict(c.datamodule.additional_parameters)
    assert params['labels_path'] is None and params['labels_skip_rows'] == 0
    assert not c.downstream.node_classification.enable
    assert c.downstream.node_classification.backend == 'sklearn'
    with pytest.raises(ValueError, match='additional_parameters.path'):   # the one required key
        EdgeListDataset(**params)
    edges = _write(tmp_path, b'1 2\n2 3\n3 1\n3 4\n', 'e.txt')
    labels = _write(tmp_path, b'1 x\n4 y\n')
    c = load_config('sge_sg_edge_list',
                    overrides=[f'datamodule.additional_parameters.path={edges}',
                               'datamodule.additional_parameters.build=host',
                               'datamodule.additional_parameters.rng=python'])
    assert not c.datamodule.instantiate_dataset().has_labels
    c = load_config('sge_sg_edge_list',
                    overrides=[f'datamodule.additional_parameters.path={edges}',
                               f'datamodule.additional_parameters.labels_path={labels}',
                               'datamodule.additional_parameters.build=host',
                               'datamodule.additional_parameters.rng=python',
                               'downstream.node_classification.enable=true',
                               'downstream.node_classification.backend=device'])
    built = c.datamodule.instantiate_dataset()
    assert built.has_labels and built.labels == {'n0000001': 'x', 'n0000004': 'y'}
    assert list(built.dataset.label_arrays()[0]) == [1, 4]
    assert c.downstream.node_classification.enable


def test_tool_refuses_features_on_the_device_backend():
    from tools.graph_model_downstream_classification import node_classification_on_device

    class WithFeatures:
        has_features = True
    with pytest.raises(ValueError, match='node features'):
        node_classification_on_device(np.zeros((3, 2), np.float32), WithFeatures(), None)
