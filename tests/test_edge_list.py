"""Edge-list ingestion, host path (shallow_encoders/graph/edge_list.py) against the restatement
in tests/edgelist_ref.py: networkx + CSRGraph.from_networkx, and a pure-Python line parser.
Every comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgelist_ref as ref  # noqa: E402

from shallow_encoders.graph.csr import CSRGraph, IdNames  # noqa: E402
from shallow_encoders.graph.edge_list import (edge_list_csr, read_edge_arrays,  # noqa: E402
                                              read_edge_list)


def _write(tmp_path, data, name='edges.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize('case', sorted(ref.ARRAY_CASES))
def test_host_path_equals_networkx(case):
    src, dst, w = ref.ARRAY_CASES[case]()
    got = edge_list_csr(src, dst, w)
    ref.assert_same_graph(got, ref.networkx_csr(src, dst, w))
    assert isinstance(got.itos, IdNames) and got.names is got.itos


def test_sparse_case_has_the_duplicates_it_claims():
    src, dst, _ = ref.sparse_weighted_edges()
    pairs = [tuple(sorted(p)) for p in zip(src.tolist(), dst.tolist())]
    assert len(pairs) - len(set(pairs)) >= 8 and sum(a == b for a, b in pairs) >= 3
    assert max(src.max(), dst.max()) == 10 ** 17


def test_host_text_parser_equals_python_parser(tmp_path):
    path = _write(tmp_path, ref.FORMAT_TEXT)
    want = ref.parse_text(ref.FORMAT_TEXT)
    assert len(want[0]) == 10 and want[0][-3] == 10 ** 17 and want[1][-3] == 10 ** 18 - 1
    for chunk in (1 << 20, 64, 40):   # one chunk; cut chunks (the longest line has 39 bytes)
        src, dst = read_edge_arrays(path, chunk_bytes=chunk)
        assert src.dtype == np.int64 and dst.dtype == np.int64
        assert (src.tolist(), dst.tolist()) == want, chunk
    ref.assert_same_graph(read_edge_list(path), ref.networkx_csr(*want))


def test_host_text_parser_equals_read_edgelist(tmp_path):
    import networkx as nx
    rng = np.random.default_rng(5)
    e = rng.integers(0, 50, size=(300, 2))
    text = '# header comment\n' + ''.join(f'{u} {v}\n' if i % 3 else f'{u}\t{v}  7\n'
                                          for i, (u, v) in enumerate(e.tolist()))
    path = _write(tmp_path, text.encode())
    g = nx.read_edgelist(path, nodetype=int, data=False)
    src, dst = read_edge_arrays(path)
    assert (src.tolist(), dst.tolist()) == (e[:, 0].tolist(), e[:, 1].tolist())
    assert sorted(g) == sorted(set(e.ravel().tolist()))
    # the same reader naming the nodes as it goes (a relabel afterwards would reorder the rows)
    named = nx.read_edgelist(path, nodetype=lambda s: f'n{int(s):07d}', data=False)
    ref.assert_same_graph(read_edge_list(path), CSRGraph.from_networkx(named))


def _line_of(exc):
    m = re.search(r'line (\d+)', str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


@pytest.mark.parametrize('bad', ref.BAD_LINES)
def test_errors_name_the_line(tmp_path, bad):
    data = b'# c\n1 2\n\n' + bad + b'\n3 4\n' + bad + b'\n'
    with pytest.raises(ref.BadLine) as e0:
        ref.parse_text(data)
    assert e0.value.line_no == 4
    path = _write(tmp_path, data)
    for chunk in (1 << 20, 32):
        with pytest.raises(ValueError) as e:
            read_edge_arrays(path, chunk_bytes=chunk)
        assert _line_of(e) == 4


def test_header_needs_skip_rows(tmp_path):
    data = b'source,target\n1,2\n2,3\n'
    path = _write(tmp_path, data, 'edges.csv')
    with pytest.raises(ValueError) as e:
        read_edge_list(path)
    assert _line_of(e) == 1
    src, dst = read_edge_arrays(path, skip_rows=1)
    assert (src.tolist(), dst.tolist()) == ([1, 2], [2, 3]) == ref.parse_text(data, 1)
    # skip_rows counts physical lines, across chunks
    src, dst = read_edge_arrays(path, skip_rows=2, chunk_bytes=16)
    assert (src.tolist(), dst.tolist()) == ([2], [3])
    ref.assert_same_graph(read_edge_list(path, skip_rows=1), ref.networkx_csr([1, 2], [2, 3]))


def test_line_longer_than_a_chunk(tmp_path):
    path = _write(tmp_path, b'1 2\n' + b'#' * 100 + b'\n3 4\n')
    with pytest.raises(ValueError, match='longer than chunk_bytes'):
        read_edge_arrays(path, chunk_bytes=32)


@pytest.mark.parametrize('data', [b'', b'# only\n% comments\n\n'])
def test_files_without_edges_are_refused(tmp_path, data):
    """A graph without nodes has no vocabulary and nothing to walk: a clear error, not an empty
    CSR (edge_list.py's docstring)."""
    path = _write(tmp_path, data)
    src, dst = read_edge_arrays(path)
    assert len(src) == 0 and len(dst) == 0
    with pytest.raises(ValueError, match='no edges'):
        read_edge_list(path)
    with pytest.raises(ValueError, match='no edges'):
        edge_list_csr(np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))


def test_npy_and_npz(tmp_path):
    src, dst, w = ref.sparse_weighted_edges()
    np.savez(tmp_path / 'g.npz', src=src, dst=dst, weight=w)
    np.savez(tmp_path / 'plain.npz', src=src, dst=dst)
    np.save(tmp_path / 'g.npy', np.stack([src, dst], axis=1))
    ref.assert_same_graph(read_edge_list(str(tmp_path / 'g.npz')), ref.networkx_csr(src, dst, w))
    plain = ref.networkx_csr(src, dst)
    ref.assert_same_graph(read_edge_list(str(tmp_path / 'plain.npz')), plain)
    ref.assert_same_graph(read_edge_list(str(tmp_path / 'g.npy')), plain)


def test_id_names():
    ids = np.array([3, 17, 123456789012], dtype=np.int64)
    names = IdNames(ids)
    assert len(names) == 4 and names.width == 12
    assert names[0] == '<unk>' and names[1] == 'n000000000003' and names[-1] == 'n123456789012'
    assert names[1:3] == ['n000000000003', 'n000000000017']
    assert list(names) == ['<unk>', 'n000000000003', 'n000000000017', 'n123456789012']
    with pytest.raises(IndexError):
        names[4]
    assert names.index('<unk>') == 0 and names.index('n000000000017') == 2
    for foreign in ('n000000000018', 'n17', 'x000000000017', 'n0000000000017', '17'):
        with pytest.raises(ValueError):
            names.index(foreign)
    assert IdNames(np.array([5])).width == 7
    with pytest.raises(ValueError):
        IdNames(np.array([2, 2]))
    g = edge_list_csr(ids[[0, 1]], ids[[2, 2]])
    assert g.node_id('n000000000017') == 2 and g.names[3] == 'n123456789012'


def test_limits():
    with pytest.raises(ValueError, match=r'10\^18'):
        edge_list_csr(np.array([1]), np.array([10 ** 18]))
    with pytest.raises(ValueError, match=r'10\^18'):
        edge_list_csr(np.array([-1]), np.array([2]))
    g = edge_list_csr(np.array([1]), np.array([10 ** 18 - 1]))
    assert g.itos[2] == 'n999999999999999999'
    with pytest.raises(ValueError, match='differ in length'):
        edge_list_csr(np.array([1, 2]), np.array([2]))


def test_dataset_host_build(tmp_path):
    import networkx as nx
    from shallow_encoders.graph.datasets import EdgeListDataset
    from shallow_encoders.word2vec.dataloader.registry import DATASET_REGISTRY
    assert DATASET_REGISTRY['graph_edge_list'] is EdgeListDataset
    e = list(nx.karate_club_graph().edges())
    path = _write(tmp_path, ''.join(f'{u} {v}\n' for u, v in e).encode())
    ds = EdgeListDataset(walks_per_node=2, walk_length=5, path=path, build='host')
    ref.assert_same_graph(ds.csr, ref.networkx_csr([u for u, _ in e], [v for _, v in e]))
    assert len(ds) == 68
    with pytest.raises(ValueError, match='build'):
        EdgeListDataset(walks_per_node=2, walk_length=5, path=path, build='gpu')


def test_config_loads(tmp_path):
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.graph.datasets import EdgeListDataset
    c = load_config('sge_sg_edge_list')
    assert c.datamodule.dataset_name == 'graph_edge_list' and c.datamodule.is_graph
    params = dict(c.datamodule.additional_parameters)
    assert params['path'] is None and params['build'] == 'auto' and params['skip_rows'] == 0
    with pytest.raises(ValueError, match='additional_parameters.path'):   # a required override
        EdgeListDataset(**params)
    c = load_config('sge_sg_edge_list',
                    overrides=['datamodule.additional_parameters.path=my/edges.txt'])
    assert c.datamodule.additional_parameters['path'] == 'my/edges.txt'
    path = _write(tmp_path, b'1 2\n2 3\n3 1\n3 4\n')
    c = load_config('sge_sg_edge_list',
                    overrides=[f'datamodule.additional_parameters.path={path}',
                               'datamodule.additional_parameters.build=host',
                               'datamodule.additional_parameters.rng=python'])
    built = c.datamodule.instantiate_dataset()
    assert built.vocab.get_itos() == ['<unk>', 'n0000001', 'n0000002', 'n0000003', 'n0000004']
    ref.assert_same_graph(built.dataset.csr, ref.networkx_csr([1, 2, 3, 3], [2, 3, 1, 4]))
