"""Multi-label node classification without a device (DESIGN.md "Device node classification"):
the one-vs-rest restatement against its own finite differences, the joint L-BFGS driver on the
restatement against sklearn's OneVsRestClassifier class by class, constant classes, the F1
metrics, the multi-label label files, the dataset's masks, dw_node_ovr's argument checks through
ctypes, and the config and tool wiring."""
import ctypes

import numpy as np
import pytest

import nodeclf_ovr_ref as ref
from shallow_encoders import _native
from shallow_encoders.graph import nodeclf
from shallow_encoders.graph.edge_list import read_node_label_sets, read_node_labels


# ---- the restatement --------------------------------------------------------------------------
def test_restated_gradient_agrees_with_central_differences_of_its_loss():
    rng = np.random.default_rng(0)
    V, d, K, n = 20, 5, 4, 60
    table = rng.normal(size=(V, d)).astype(np.float32)
    ids = rng.integers(0, V, n)
    masks = rng.integers(0, 1 << K, n)
    coef = rng.normal(size=(K, d + 1))
    got = ref.ovr_sums(table, ids, masks, coef, K)
    sums = got.sums[ref.THRESHOLD]
    grad = sums[:K * (d + 1)].reshape(K, d + 1)
    h = 1e-6
    at = K * (d + 1)
    for k in range(K):
        for j in range(d + 1):
            up, down = coef.copy(), coef.copy()
            up[k, j] += h
            down[k, j] -= h
            fd = (ref.ovr_sums(table, ids, masks, up, K).sums[0][at]
                  - ref.ovr_sums(table, ids, masks, down, K).sums[0][at]) / (2 * h)
            assert abs(fd - grad[k, j]) <= 1e-6 * max(1.0, got.mags[k * (d + 1) + j]), (k, j)
    X, Y = table[ids].astype(np.float64), ref.bits(masks, K)
    assert sums[at] == pytest.approx(ref.class_objectives(X, Y, coef, C=1.0).sum()
                                     - 0.5 * (coef[:, :d] ** 2).sum(), rel=1e-13)
    # the counts under both rules, and the rules themselves
    Z = X @ coef[:, :d].T + coef[:, d]
    np.testing.assert_array_equal(ref.bits(got.pred[ref.THRESHOLD], K), Z > 0)
    top = ref.bits(got.pred[ref.TOP_K], K)
    np.testing.assert_array_equal(top.sum(axis=1), Y.sum(axis=1))
    for i in range(n):   # every predicted logit is above every logit that is not
        assert not top[i].any() or not (~top[i]).any() or Z[i][top[i]].min() > Z[i][~top[i]].max()
    for rule, P in ((ref.THRESHOLD, Z > 0), (ref.TOP_K, top)):
        tail = got.sums[rule][at + 1:].reshape(3, K)
        np.testing.assert_array_equal(tail, [(P & Y).sum(0), P.sum(0), Y.sum(0)])


def test_restatement_drops_a_bad_id_or_a_mask_bit_past_the_classes():
    rng = np.random.default_rng(1)
    table = rng.normal(size=(10, 3)).astype(np.float32)
    ids = np.asarray([1, 2, -1, 10, 3, 4])
    masks = np.asarray([0, 3, 1, 1, 4, -1])   # K = 2: bit 2 and the sign bit are out of range
    coef = rng.normal(size=(2, 4))
    got = ref.ovr_sums(table, ids, masks, coef, 2)
    want = ref.ovr_sums(table, ids[:2], masks[:2], coef, 2)
    for rule in (ref.THRESHOLD, ref.TOP_K):
        np.testing.assert_array_equal(got.sums[rule], want.sums[rule])
        assert not got.pred[rule][2:].any()
        assert list(got.pred[rule][:2]) == list(want.pred[rule])
    # at K = 64 every bit is a label
    assert ref.valid(table, ids[:2], np.asarray([-1, 1 << 62]), 64).all()


def test_top_k_ties_go_to_the_lowest_column():
    Z = np.asarray([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0]])
    np.testing.assert_array_equal(ref.top_k(Z, [1, 1, 2]),
                                  [[True, False, False], [False, True, False],
                                   [True, True, False]])
    assert not ref.top_k(Z, [0, 0, 0]).any() and ref.top_k(Z, [3, 3, 3]).all()


# ---- the driver -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['m3', 'm7', 'm40'])
def test_joint_driver_reaches_sklearns_objective_in_every_class(name):
    """fit_closure on the restatement against OneVsRestClassifier(LogisticRegression()) at its
    defaults: the objective is separable, so the joint minimiser is every class's own, and no
    class's objective, recomputed in float64, may exceed sklearn's (margin 0)."""
    n, d, K = ref.PROBLEMS[name]
    table, ids, masks = ref.problem(name)
    X, Y = table[ids].astype(np.float64), ref.bits(masks, K)
    assert Y.sum(axis=1).min() >= 1 and Y.sum(axis=1).max() <= 3
    clf = nodeclf.NodeOvRLogisticRegression().fit_closure(ref.closure(name), d, K)
    assert clf.coef_.shape == (K, d) and clf.intercept_.shape == (K,)
    assert clf.full_coef().shape == (K, d + 1) and list(clf.classes_) == list(range(K))
    ours = ref.class_objectives(X, Y, clf.full_coef())
    _, _, theirs = ref.sklearn_fit(name)
    gap = (ours - theirs) / theirs
    print(f'{name}: worst class gap {gap.max():.3g} (sum {ours.sum()!r} vs sklearn '
          f'{theirs.sum()!r}), {clf.n_iter_} iterations')
    assert (ours <= theirs).all(), gap
    assert abs(clf.objective_ - ours.sum()) <= 1e-10 * ours.sum()


def test_driver_without_intercept_and_one_class():
    n, d, K = ref.PROBLEMS['m3']
    full = nodeclf.NodeOvRLogisticRegression().fit_closure(ref.closure('m3'), d, K)
    flat = nodeclf.NodeOvRLogisticRegression(fit_intercept=False).fit_closure(
        ref.closure('m3'), d, K)
    assert not flat.intercept_.any() and flat.coef_.any()
    assert flat.objective_ >= full.objective_
    # K = 1 is a legal one-vs-rest problem: class 0 of m3 alone
    table, ids, masks = ref.problem('m3')
    one = nodeclf.NodeOvRLogisticRegression().fit_closure(
        lambda coef: ref.ovr_sums(table, ids, masks & 1, coef, 1).sums[0], d, 1)
    X, Y = table[ids].astype(np.float64), ref.bits(masks, K)
    assert one.coef_.shape == (1, d)
    assert ref.class_objectives(X, Y[:, :1], one.full_coef())[0] <= ref.sklearn_fit('m3')[2][0]
    with pytest.raises(ValueError, match='n_classes'):
        nodeclf.NodeOvRLogisticRegression().fit_closure(lambda c: c, 4, 65)
    with pytest.raises(ValueError, match=r"classifier_params \['penalty'\]"):
        nodeclf.NodeOvRLogisticRegression.from_params({'penalty': 'l1'})
    assert nodeclf.NodeOvRLogisticRegression.from_params({'C': 2.0}).C == 2.0


def test_constant_classes_are_not_fitted():
    """A class no training node has is left out (and so never predicted); a class every
    training node has raises; the compacted masks map back through classes_."""
    clf = nodeclf.NodeOvRLogisticRegression()
    masks = np.asarray([0b00101, 0b10001, 0b00100, 0b10000])   # classes 1 and 3 are empty
    assert list(clf.fitted_classes(masks, 5)) == [0, 2, 4]
    clf.classes_, clf.n_labels_ = np.asarray([0, 2, 4]), 5
    assert list(clf.compact(masks)) == [0b011, 0b101, 0b010, 0b100]
    assert list(clf.compact(np.asarray([0b01010]))) == [0]   # unfitted labels give k = 0
    with pytest.raises(ValueError, match='every training node has label 2'):
        clf.fitted_classes(np.asarray([0b101, 0b100, 0b110]), 3)
    with pytest.raises(ValueError, match='at or above n_classes'):
        clf.fitted_classes(np.asarray([0b1000]), 3)
    # bit 63 is a label like any other
    top = np.asarray([-2, 1], dtype=np.int64)   # bits 1 .. 63, and bit 0
    assert list(clf.fitted_classes(top, 64)) == list(range(64))
    np.testing.assert_array_equal(nodeclf.bits_mask(nodeclf.mask_bits(top, 64)), top)


def test_micro_macro_f1_equals_sklearns():
    from sklearn.metrics import f1_score
    rng = np.random.default_rng(3)
    Y = rng.random((200, 6)) < 0.3
    P = rng.random((200, 6)) < 0.3
    Y[:, 4] = P[:, 4] = False   # neither present nor predicted
    P[:, 5] = False             # present, never predicted
    micro, macro = nodeclf.micro_macro_f1((Y & P).sum(0), P.sum(0), Y.sum(0))
    assert micro == pytest.approx(f1_score(Y, P, average='micro', zero_division=0), rel=1e-14)
    assert macro == pytest.approx(f1_score(Y, P, average='macro', zero_division=0), rel=1e-14)
    assert nodeclf.micro_macro_f1([0, 0], [0, 0], [0, 0]) == (0.0, 0.0)


# ---- label files ------------------------------------------------------------------------------
def _write(tmp_path, data: bytes, name='labels.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_label_set_lines(tmp_path):
    text = (b'node,group\n'            # header, skipped by skip_rows
            b'# a comment\n'
            b'\n'
            b'7,g1\n'                  # a repeated node: its sets are unioned
            b'  3 red blue\tgreen \r\n'   # several labels on one line, CRLF
            b'7,g2\r\n'
            b'% another\n'
            b'7,g1\n'                  # a repeated pair counts once
            b'3,,blue,\n'
            b'000000000000000005 x')   # no last newline
    ids, sets = read_node_label_sets(_write(tmp_path, text), skip_rows=1)
    assert ids.dtype == np.int64 and list(ids) == [7, 3, 5]
    assert sets == [['g1', 'g2'], ['red', 'blue', 'green'], ['x']]
    ids, sets = read_node_label_sets(_write(tmp_path, b'# nothing\n'))
    assert ids.dtype == np.int64 and len(ids) == 0 and sets == []


@pytest.mark.parametrize('bad', [b'-3 red', b'3', b'3 ', b'3,,', b'red 3', b'3red x',
                                 b'1234567890123456789 x', b'3 re\rd', b'3.5 x'])
def test_label_set_file_names_the_malformed_line(tmp_path, bad):
    with pytest.raises(ValueError, match=r'line 4 is not a node and its labels'):
        read_node_label_sets(_write(tmp_path, b'# head\n1 a\n\n' + bad + b'\n2 b\n'))
    with pytest.raises(ValueError, match=r'line 4 '):
        read_node_label_sets(_write(tmp_path, b'# head\r\n1 a\r\n\r\n' + bad))


def test_label_set_npz_and_the_single_label_reader_still_refuses(tmp_path):
    np.savez(tmp_path / 'l.npz', node=np.asarray([9, 2, 9, 9], dtype=np.int32),
             label=np.asarray([10, 2, 3, 10]))
    ids, sets = read_node_label_sets(str(tmp_path / 'l.npz'))
    assert list(ids) == [9, 2] and ids.dtype == np.int64 and sets == [['10', '3'], ['2']]
    np.savez(tmp_path / 'f.npz', node=np.asarray([1, 2]), label=np.asarray([0.5, 1.0]))
    with pytest.raises(ValueError, match='integer arrays'):
        read_node_label_sets(str(tmp_path / 'f.npz'))
    with pytest.raises(ValueError, match='node 9 is labelled twice'):
        read_node_labels(str(tmp_path / 'l.npz'))
    with pytest.raises(ValueError, match=r'line 3 labels node 7 a second time'):
        read_node_labels(_write(tmp_path, b'7 a\n8 b\n7 c\n'))


# ---- the dataset ------------------------------------------------------------------------------
EDGES = b'1 2\n2 3\n3 10\n10 40\n40 1\n5 3\n'
KW = dict(walks_per_node=1, walk_length=4, build='host', rng='philox')


def test_edge_list_dataset_masks(tmp_path):
    from shallow_encoders.graph.datasets import EdgeListDataset
    edges = _write(tmp_path, EDGES, 'edges.txt')
    labels = _write(tmp_path, b'id,label\n40,b\n2,10 b\n77,zz\n3,9\n40,9\n1,b\n2,b\n')
    ds = EdgeListDataset(path=edges, labels_path=labels, labels_skip_rows=1, multilabel=True,
                         **KW)
    assert ds.has_labels and ds.is_multilabel and ds.n_labels_dropped == 1
    rows, masks, classes = ds.label_arrays()
    # nodes 1 2 3 5 10 40 -> rows 1 .. 6; 5 and 10 carry no label; 77's label zz is dropped
    assert rows.dtype == np.int64 and list(rows) == [1, 2, 3, 6]
    assert classes == ['10', '9', 'b'] and masks.dtype == np.int64
    assert list(masks) == [0b100, 0b101, 0b010, 0b110]
    assert ds.labels == {'n0000001': ('b',), 'n0000002': ('10', 'b'), 'n0000003': ('9',),
                         'n0000040': ('9', 'b')}
    single = EdgeListDataset(path=edges, labels_path=_write(tmp_path, b'1 a\n2 b\n', 's.txt'),
                             **KW)
    assert single.has_labels and not single.is_multilabel
    assert single.label_arrays()[1].dtype == np.int32


def test_edge_list_dataset_takes_64_labels_and_refuses_65(tmp_path):
    from shallow_encoders.graph.datasets import EdgeListDataset
    edges = _write(tmp_path, EDGES, 'edges.txt')
    lab64 = _write(tmp_path, b'1 ' + b' '.join(b'l%02d' % i for i in range(64)) + b'\n', 'a.txt')
    rows, masks, classes = EdgeListDataset(path=edges, labels_path=lab64, multilabel=True,
                                           **KW).label_arrays()
    assert len(classes) == 64 and list(masks) == [-1]   # bit 63 set: the int64 is negative
    lab65 = _write(tmp_path, b'1 ' + b' '.join(b'l%02d' % i for i in range(65)) + b'\n', 'b.txt')
    with pytest.raises(ValueError, match='65 distinct labels.*at most 64'):
        EdgeListDataset(path=edges, labels_path=lab65, multilabel=True, **KW)


# ---- the entry points' argument checks (no device call is made) -------------------------------
def _ovr(d=8, K=3, n=4, V=10, rule=1, fake=None, ws_bytes=0):
    lib = _native.load()
    p = fake
    rc = lib.dw_node_ovr(p, V, d, p, p, n, K, p, rule, p, None, p, ws_bytes, None, None)
    return rc, lib.dw_last_error_string()


def _workspace(n, d, K):
    nb = ctypes.c_size_t(0)
    rc = _native.load().dw_node_ovr_workspace_bytes(n, d, K, ctypes.byref(nb))
    return rc, int(nb.value)


@pytest.mark.parametrize('kw', [dict(d=0), dict(d=513), dict(K=0), dict(K=65), dict(n=-1),
                                dict(V=0), dict(V=2 ** 31)])
def test_abi_refuses_bad_sizes_before_the_pointers(kw):
    rc, err = _ovr(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert b'dw_node_ovr' in err and b'bad sizes' in err and b'null pointer' not in err, err
    if 'V' not in kw:
        args = dict(n=4, d=8, K=3)
        args.update(kw)
        assert _workspace(**args)[0] == _native.DW_E_INVALID_ARG


@pytest.mark.parametrize('rule', [-1, 2])
def test_abi_refuses_a_bad_rule_before_the_pointers(rule):
    rc, err = _ovr(rule=rule)
    assert rc == _native.DW_E_INVALID_ARG and b'bad rule' in err, err
    assert _ovr(rule=rule, n=0)[0] == _native.DW_E_INVALID_ARG


def test_abi_takes_the_limits_up_to_the_pointers():
    for kw in (dict(), dict(d=1, K=1), dict(d=512, K=64), dict(V=2 ** 31 - 1), dict(rule=0)):
        rc, err = _ovr(**kw)
        assert rc == _native.DW_E_INVALID_ARG and b'null pointer' in err, (kw, err)
        assert _ovr(n=0, **kw)[0] == _native.DW_OK
    assert _native.load().dw_node_ovr_workspace_bytes(4, 8, 3, None) == _native.DW_E_INVALID_ARG


def test_abi_refuses_a_short_workspace():
    """Never-dereferenced non-null pointers: the size check comes before any launch."""
    rc, need = _workspace(1000, 128, 47)
    assert rc == _native.DW_OK
    # one partial row of K (d + 1) + 1 + 3 K doubles per block, 64 samples a block at this dim
    assert need == 16 * (47 * 129 + 1 + 3 * 47) * 8
    assert _workspace(10 ** 6, 512, 64)[1] == 256 * (64 * 513 + 1 + 3 * 64) * 8
    assert _workspace(33, 512, 1)[1] == 2 * (513 + 4) * 8
    rc, err = _ovr(d=128, K=47, n=1000, fake=64, ws_bytes=need - 8)
    assert rc == _native.DW_E_INVALID_ARG and b'workspace too small' in err, err
    # the softmax entry point keeps its own lower limit and row length
    nb = ctypes.c_size_t(0)
    lib = _native.load()
    assert lib.dw_node_softmax_workspace_bytes(4, 8, 1, ctypes.byref(nb)) == \
        _native.DW_E_INVALID_ARG
    assert lib.dw_node_softmax_workspace_bytes(4, 8, 2, ctypes.byref(nb)) == _native.DW_OK
    assert nb.value == (2 * 9 + 2) * 8


def test_wrapper_refuses_host_and_malformed_tensors():
    import torch
    table = torch.zeros(10, 8)
    ids = torch.zeros(4, dtype=torch.int64)
    m = torch.zeros(4, dtype=torch.int64)
    coef = torch.zeros(3, 9, dtype=torch.float64)
    with pytest.raises(ValueError, match='n_classes'):
        nodeclf.ovr_sums(table, ids, m, coef, 0)
    with pytest.raises(ValueError, match='n_classes'):
        nodeclf.ovr_sums(table, ids, m, coef, 65)
    with pytest.raises(ValueError, match='rule'):
        nodeclf.ovr_sums(table, ids, m, coef, 3, rule='argmax')
    with pytest.raises(ValueError, match='masks'):
        nodeclf.ovr_sums(table, ids, m.int(), coef, 3)
    with pytest.raises(ValueError, match='coef'):
        nodeclf.ovr_sums(table, ids, m, coef[:2], 3)
    with pytest.raises(ValueError, match='pred'):
        nodeclf.ovr_sums(table, ids, m, coef, 3, pred=torch.zeros(4, dtype=torch.int32))
    # host tensors never reach a kernel: no CPU fallback
    with pytest.raises((ValueError, _native.NativeLibraryError, _native.DWError)):
        nodeclf.ovr_sums(table, ids, m, coef, 3, workspace=torch.zeros(64, dtype=torch.float64))


# ---- config and tool --------------------------------------------------------------------------
def test_config_keys():
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.config_parser.core import GraphDownstreamNodeClassificationConfig
    assert GraphDownstreamNodeClassificationConfig().prediction == 'top_k'
    assert GraphDownstreamNodeClassificationConfig(prediction='threshold').prediction == \
        'threshold'
    with pytest.raises(ValueError, match='node_classification.prediction'):
        GraphDownstreamNodeClassificationConfig(prediction='argmax')
    c = load_config('sge_sg_edge_list')
    assert dict(c.datamodule.additional_parameters)['multilabel'] is False
    assert c.downstream.node_classification.prediction == 'top_k'
    c = load_config('sge_sg_edge_list',
                    overrides=['datamodule.additional_parameters.multilabel=true',
                               'downstream.node_classification.prediction=threshold'])
    assert dict(c.datamodule.additional_parameters)['multilabel'] is True
    assert c.downstream.node_classification.prediction == 'threshold'


def test_tool_refuses_a_multilabel_dataset_on_the_sklearn_backend():
    from shallow_encoders.config_parser.core import GraphDownstreamNodeClassificationConfig
    from tools.graph_model_downstream_classification import check_node_backend

    class Inner:
        is_multilabel = True

    class Wrapped:
        dataset = Inner()
    with pytest.raises(ValueError, match='backend=device'):
        check_node_backend(Wrapped(), GraphDownstreamNodeClassificationConfig())
    check_node_backend(Wrapped(), GraphDownstreamNodeClassificationConfig(backend='device'))
    Inner.is_multilabel = False
    check_node_backend(Wrapped(), GraphDownstreamNodeClassificationConfig())
