"""The connected held-out edge split on the GPU (dw_edge_forest, dw_edge_holdout_count_protected
and dw_edge_holdout_protected in csrc/dw_holdout.hip): the device split against the host path bit
for bit, the forest's flags, labels and counts against the Kruskal / breadth-first restatement
tests/holdout_connected_ref.py, the refusals and empty inputs, and both tools on a tiny graph."""
import ctypes
import functools
import math
import os
import random

import numpy as np
import pytest
import torch

import holdout_connected_ref as cref
from shallow_encoders import _native
from shallow_encoders.graph.csr import CSRGraph
from shallow_encoders.graph.holdout import connected_components, split_edges

pytestmark = pytest.mark.gpu

GRAPHS = cref.graphs()


@functools.lru_cache(maxsize=None)
def built(name):
    return GRAPHS[name]()


def _forest(csr, seed, dev):
    """dw_edge_forest through the ABI: (flags uint8[nnz], labels int32[V], counts [4], status)."""
    d = csr.device_tensors(dev)
    V, nnz = csr.vocab_size, csr.nnz
    nb = ctypes.c_size_t(0)
    _native.call('dw_edge_forest_workspace_bytes', V, nnz, ctypes.byref(nb))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    flags = torch.full((max(nnz, 1),), 7, dtype=torch.uint8, device=dev)
    labels = torch.full((V,), -5, dtype=torch.int32, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call('dw_edge_forest', _native.ptr(d['row_ptr']),
                 _native.ptr(d['col']) if nnz else None, V, nnz, seed, _native.ptr(flags),
                 _native.ptr(labels), _native.ptr(counts), _native.ptr(status), _native.ptr(ws),
                 ws.numel(), _native.stream(dev))
    return flags[:nnz].cpu().numpy(), labels.cpu().numpy(), counts.tolist(), int(status.item())


# ---- 1. the split --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_device_connected_split_equals_host_split(name, hip_device):
    g = built(name)
    for ratio, seed in ((0.1, 0), (0.5, 7), (0.9, 2)):
        want, held_w, info_w = split_edges(g, ratio, seed, protect='connected')
        got, held, info = split_edges(g, ratio, seed, device=hip_device, protect='connected')
        again, held2, info2 = split_edges(g, ratio, seed, device=hip_device, protect='connected')
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
        if again.weights is not None:
            assert np.array_equal(again.weights.view(np.uint64), got.weights.view(np.uint64))
    if name in ('star', 'path', 'triplets'):
        assert info['n_hold'] == 0
    if name == 'bridge':
        assert cref.BRIDGE not in {(int(a), int(b)) for a, b in held.cpu().numpy()}


def test_device_degree_split_is_unchanged_by_the_argument(hip_device):
    g = built('self_loops')
    a, held_a, info_a = split_edges(g, 0.5, 3, device=hip_device)
    b, held_b, info_b = split_edges(g, 0.5, 3, device=hip_device, protect='degree')
    assert info_a == info_b and set(info_a) == {'n_edges', 'n_want', 'n_candidates', 'n_hold'}
    assert torch.equal(held_a, held_b) and np.array_equal(a.host_col(), b.host_col())
    assert np.array_equal(a.row_ptr, b.row_ptr)


# ---- 2. dw_edge_forest ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_edge_forest_equals_the_kruskal_restatement(name, hip_device):
    g = built(name)
    row_ptr, col = g.row_ptr, g.host_col()
    V = g.vocab_size
    rows = np.repeat(np.arange(V), np.diff(row_ptr))
    labels_ref = cref.components(row_ptr, col)
    edges = cref.csr_edges(row_ptr, col)
    touched = {n for e in edges for n in e}
    for seed in (0, 7):
        forest = cref.forest(row_ptr, col, seed)
        want = np.asarray([(min(x, y), max(x, y)) in forest
                           for x, y in zip(rows.tolist(), col.tolist())], dtype=np.uint8)
        flags, labels, counts, status = _forest(g, seed, hip_device)
        assert status == 0
        np.testing.assert_array_equal(flags, want.reshape(-1))
        np.testing.assert_array_equal(labels, labels_ref)
        n_comp = len({int(labels_ref[n]) for n in touched})
        assert counts[:3] == [len(edges), len(forest), n_comp]
        assert len(forest) == len(touched) - n_comp
        assert 0 <= counts[3] <= math.ceil(math.log2(V))
        again = _forest(g, seed, hip_device)
        assert np.array_equal(again[0], flags) and np.array_equal(again[1], labels)
        assert again[2] == counts
        if name in ('karate', 'rmat12', 'self_loops'):
            assert counts[3] == {'karate': 2, 'rmat12': 4, 'self_loops': 3}[name]
    got, n = connected_components(g, device=hip_device)
    assert got.dtype == torch.int32 and n == len(set(labels_ref[1:].tolist()))
    np.testing.assert_array_equal(got.cpu().numpy(), labels_ref)


# ---- 3. refusals and empty inputs ----------------------------------------------------------------
def test_device_connected_split_refuses_a_repeated_neighbour(hip_device):
    dup = CSRGraph.from_arrays([0, 0, 2, 3, 4], [2, 2, 1, 1])
    with pytest.raises(ValueError, match='twice'):
        split_edges(dup, 0.5, 0, device=hip_device, protect='connected')
    with pytest.raises(ValueError, match='twice'):
        connected_components(dup, device=hip_device)


def test_empty_and_loops_only_graphs_come_back_unchanged(hip_device):
    empty = CSRGraph.from_arrays([0, 0, 0, 0], [])
    loops = CSRGraph.from_arrays([0, 0, 1, 2, 3], [1, 2, 3])
    for g in (empty, loops):
        V = g.vocab_size
        train, held, info = split_edges(g, 0.5, 0, device=hip_device, protect='connected')
        assert info == {'n_edges': 0, 'n_want': 0, 'n_candidates': 0, 'n_hold': 0,
                        'n_forest': 0, 'n_components': 0}
        assert info == split_edges(g, 0.5, 0, protect='connected')[2]
        assert held.shape == (0, 2)
        np.testing.assert_array_equal(train.row_ptr, g.row_ptr)
        np.testing.assert_array_equal(train.host_col(), g.col)
        flags, labels, counts, status = _forest(g, 0, hip_device)
        assert status == 0 and counts == [0, 0, 0, 0] and not flags.any()
        np.testing.assert_array_equal(labels, np.arange(V))
        labels, n = connected_components(g, device=hip_device)
        assert n == V - 1 and labels.cpu().tolist() == list(range(V))


# ---- 4. the tools --------------------------------------------------------------------------------
def test_tools_on_a_graph_rmat_dataset_with_a_connected_holdout(tmp_path, hip_device):
    """tools/train.py then the downstream tool on a scale-12 graph_rmat with holdout_ratio=0.5 and
    holdout_protect=connected: both build the same split, the residual graph keeps the full
    graph's components, and protocol=heldout reports a finite AUC."""
    from shallow_encoders.common.path import CONFIG_PATH
    from shallow_encoders.config_parser import load_config_dict
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    from tools.utils import setup_pipeline
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_cora', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=lpc', 'datamodule.dataset_name=graph_rmat',
            'datamodule.additional_parameters.scale=12',
            'datamodule.additional_parameters.n_edges=40000',
            'datamodule.additional_parameters.graph_seed=0',
            'datamodule.additional_parameters.walks_per_node=1',
            'datamodule.additional_parameters.method_params.q=1',
            'datamodule.additional_parameters.rng=philox', 'train.noise=device',
            'model.embedding_size=128', 'train.optimizer.lr=0.01', 'train.max_epochs=1',
            'downstream.node_classification.enable=false',
            'downstream.edge_classification.n_experiments=2',
            'datamodule.additional_parameters.holdout_ratio=0.5',
            'datamodule.additional_parameters.holdout_protect=connected']
    heldout = base + ['downstream.edge_classification.protocol=heldout',
                      'downstream.edge_classification.backend=device']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_rmat', 'lpc', 'checkpoints', 'last.ckpt'))
    res = downstream.main(heldout)
    assert set(res) == {'edge_auc', 'edge_auc_std', 'edge_accuracy', 'edge_best'}
    assert math.isfinite(res['edge_auc']) and 0.0 <= res['edge_auc'] <= 1.0

    def dataset(overrides):
        cfg = setup_pipeline(load_config_dict('sge_sg_cora', CONFIG_PATH, overrides[2:]),
                             task='downstream-classification')
        return cfg.datamodule.instantiate_dataset().dataset
    a, b = dataset(base), dataset(heldout)
    held = np.asarray(a.heldout_edges)
    assert a.holdout_info == {'n_edges': 32749, 'n_want': 16374, 'n_candidates': 28655,
                              'n_hold': 16374, 'n_forest': 4094, 'n_components': 2}
    np.testing.assert_array_equal(held, np.asarray(b.heldout_edges))
    np.testing.assert_array_equal(a.csr.row_ptr, b.csr.row_ptr)
    np.testing.assert_array_equal(connected_components(a.csr)[0],
                                  connected_components(a.full_csr)[0])
