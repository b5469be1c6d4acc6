"""Edge-list ingestion on the device (csrc/dw_edgelist.hip through graph/edge_list.py): equal,
bit for bit, to the host path and to the restatement in tests/edgelist_ref.py, at the smallest
shapes that cross blocks, scan tiles, chunks and key widths."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgelist_ref as ref  # noqa: E402

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph.edge_list import (edge_list_csr, read_edge_arrays,  # noqa: E402
                                              read_edge_list)

pytestmark = pytest.mark.gpu


def _workspace(dev, n_bytes, m):
    nb = ctypes.c_size_t(0)
    _native.call('dw_edgelist_workspace_bytes', n_bytes, m, ctypes.byref(nb))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=dev)


def device_parse(data: bytes, dev, skip=0, misalign=0):
    """dw_edgelist_parse on its own: (src, dst, lines seen, bad line or -1, status).
    ``misalign``: the text starts that many bytes past a 16-byte boundary."""
    n = len(data)
    cap = (n + 1) // 4 + 1
    with torch.cuda.device(dev):
        text = None
        if n:
            buf = torch.frombuffer(bytearray(b'9' * misalign + data), dtype=torch.uint8).to(dev)
            text = buf[misalign:]
            assert text.data_ptr() % 16 == misalign
        ws = _workspace(dev, n, 0)
        src = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        dst = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        info = torch.zeros(3, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_edgelist_parse', _native.ptr(text), n, skip, _native.ptr(src),
                     _native.ptr(dst), cap, _native.ptr(info), _native.ptr(info[2:]),
                     _native.ptr(status), _native.ptr(ws), ws.numel(), _native.stream(dev))
        k, lines, bad = info.tolist()
    assert (src[k:] == -7).all() and (dst[k:] == -7).all()   # nothing written past the count
    return src[:k].tolist(), dst[:k].tolist(), lines, bad, int(status.item())


def _n_lines(data: bytes) -> int:
    return data.count(b'\n') + (0 if data.endswith(b'\n') or not data else 1)


def _check_parse(data: bytes, dev, skip=0):
    want = ref.parse_text(data, skip)
    got = device_parse(data, dev, skip)
    assert got[4] == 0 and got[3] == -1
    assert (got[0], got[1]) == want
    assert got[2] == _n_lines(data)
    assert device_parse(data, dev, skip) == got   # a rerun is bit-identical
    return want


def _write(tmp_path, data, name='edges.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _random_lines(n, seed, width=None):
    """n lines 'u v' of random ids; ``width``: every line padded with an extra column to exactly
    that many bytes (newline excluded)."""
    rng = np.random.default_rng(seed)
    out = []
    for u, v in rng.integers(0, 10 ** 6, size=(n, 2)).tolist():
        s = f'{u} {v}'
        if width is not None:
            s = (s + ' ' + 'x' * width)[:width]
        out.append(s)
    return ('\n'.join(out) + '\n').encode()


# ---- device against host: every input of the CPU test ------------------------------------------
@pytest.mark.parametrize('case', sorted(ref.ARRAY_CASES))
def test_device_equals_host(case, hip_device):
    src, dst, w = ref.ARRAY_CASES[case]()
    host = edge_list_csr(src, dst, w)
    dev = edge_list_csr(src, dst, w, device=hip_device)
    assert dev.col is None and dev.weighted == (w is not None)   # built and kept in HBM
    d = dev.device_tensors(hip_device)
    assert d['col'].is_cuda and (d['weights'] is None) == (w is None)
    ref.assert_same_graph(dev, host)
    again = edge_list_csr(torch.as_tensor(src).to(hip_device), torch.as_tensor(dst).to(hip_device),
                          None if w is None else torch.as_tensor(w).to(hip_device),
                          device=hip_device)
    assert torch.equal(again.device_tensors(hip_device)['col'], d['col'])
    assert torch.equal(again.device_tensors(hip_device)['row_ptr'], d['row_ptr'])
    if w is not None:
        assert torch.equal(again.device_tensors(hip_device)['weights'], d['weights'])
    np.testing.assert_array_equal(again.itos.ids, host.itos.ids)


def test_device_text_equals_host_and_networkx(tmp_path, hip_device):
    path = _write(tmp_path, ref.FORMAT_TEXT)
    want = ref.parse_text(ref.FORMAT_TEXT)
    for chunk in (1 << 20, 64, 40):
        src, dst = read_edge_arrays(path, device=hip_device, chunk_bytes=chunk)
        assert src.is_cuda and (src.tolist(), dst.tolist()) == want, chunk
    ref.assert_same_graph(read_edge_list(path, device=hip_device), ref.networkx_csr(*want))


def test_device_limits(hip_device):
    with pytest.raises(ValueError, match=r'10\^18'):
        edge_list_csr(np.array([1]), np.array([10 ** 18]), device=hip_device)
    with pytest.raises(ValueError, match=r'10\^18'):
        edge_list_csr(torch.tensor([-1]), torch.tensor([2]), device=hip_device)
    g = edge_list_csr(np.array([1]), np.array([10 ** 18 - 1]), device=hip_device)
    assert g.itos[2] == 'n999999999999999999'


# ---- dw_edgelist_parse on its own ----------------------------------------------------------------
def test_parse_format_file(hip_device):
    _check_parse(ref.FORMAT_TEXT, hip_device)
    _check_parse(ref.FORMAT_TEXT, hip_device, skip=5)
    _check_parse(b'', hip_device)
    _check_parse(b'\n', hip_device)
    _check_parse(b'# c', hip_device)


@pytest.mark.parametrize('n', [257, 65537])
def test_parse_many_lines(n, hip_device):
    want = _check_parse(_random_lines(n, seed=n), hip_device)
    assert len(want[0]) == n


@pytest.mark.parametrize('width', [3, 60])
def test_parse_line_lengths(width, hip_device):
    if width == 3:
        data = b'\n'.join(b'%d %d' % (i % 10, (7 * i) % 10) for i in range(1000)) + b'\n'
    else:
        data = _random_lines(1000, seed=60, width=60)
    assert all(len(x) == width for x in data.split(b'\n')[:-1])
    assert len(_check_parse(data, hip_device)[0]) == 1000


def test_parse_long_lines_and_unaligned_text(hip_device):
    """Lines that run past a lane's segment, past the bytes a block stages and past the block;
    and a text pointer off the 16-byte boundary (the staging loads bytes then)."""
    data = (b'1 2\n' + b'#' + b'c' * 1000 + b'\n' + b' ' * 300 + b'3\t4\n' + b'5 6 ' + b'x' * 700
            + b'\n' + _random_lines(1500, seed=8) + b'%' + b' 7 8' * 5000 + b'\n9 10\n'
            + b' ' * 17000 + b'11 12')
    want = _check_parse(data, hip_device)
    assert want[0][:3] == [1, 3, 5] and want[0][-2:] == [9, 11] and len(want[0]) == 1505
    for misalign in (1, 7, 8):
        got = device_parse(data, hip_device, misalign=misalign)
        assert (got[0], got[1]) == want and got[2:] == (_n_lines(data), -1, 0)
    bad = data + b'x'
    assert device_parse(bad, hip_device, misalign=3)[2:] == (_n_lines(bad), _n_lines(bad) - 1,
                                                             _native.DW_S_BAD_TEXT)


def test_parse_last_byte_is_a_digit(hip_device):
    for tail in (b'12 345', b'1 2', b'123456789012345678 9'):
        data = _random_lines(100, seed=1) + tail
        want = _check_parse(data, hip_device)
        assert (want[0][-1], want[1][-1]) == tuple(int(x) for x in tail.split())
    _check_parse(b'4 5', hip_device)


def test_parse_many_chunks(tmp_path, hip_device):
    data = b'# header\n' + _random_lines(5000, seed=5)
    path = _write(tmp_path, data)
    want = ref.parse_text(data)
    src, dst = read_edge_arrays(path, device=hip_device, chunk_bytes=64)
    assert (src.tolist(), dst.tolist()) == want
    hs, hd = read_edge_arrays(path, chunk_bytes=64)
    assert (hs.tolist(), hd.tolist()) == want
    src, dst = read_edge_arrays(path, device=hip_device, chunk_bytes=64, skip_rows=4001)
    assert (src.tolist(), dst.tolist()) == ref.parse_text(data, 4001)


def _line_of(exc):
    m = re.search(r'line (\d+)', str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


@pytest.mark.parametrize('bad', ref.BAD_LINES + [b'source,target'])
def test_parse_errors_name_the_line(tmp_path, bad, hip_device):
    data = b'# c\n1 2\n\n' + bad + b'\n3 4\n' + bad + b'\n'
    got = device_parse(data, hip_device)
    assert got[4] == _native.DW_S_BAD_TEXT and got[3] == 3   # 0-based; the first of the two
    path = _write(tmp_path, data)
    with pytest.raises(ValueError) as e:
        read_edge_arrays(path, device=hip_device)
    assert _line_of(e) == 4
    # the same line in the third chunk of a longer file: the number stays global. Lines of
    # exactly 14 bytes: a 64-byte chunk holds four, so chunk 3 starts at line 9.
    fixed = [b'%d %d\n' % (100000 + 7 * i, 999999 - 3 * i) for i in range(30)]
    assert all(len(x) == 14 for x in fixed)
    data = b''.join(fixed[:9]) + bad + b'\n' + b''.join(fixed[9:]) + bad + b'\n'
    path = _write(tmp_path, data, 'long.txt')
    with pytest.raises(ref.BadLine) as e0:
        ref.parse_text(data)
    assert e0.value.line_no == 10
    for device in (hip_device, None):
        with pytest.raises(ValueError) as e:
            read_edge_arrays(path, device=device, chunk_bytes=64)
        assert _line_of(e) == 10


def test_header_passes_with_skip_rows(tmp_path, hip_device):
    path = _write(tmp_path, b'source,target\n1,2\n2,3\n', 'edges.csv')
    with pytest.raises(ValueError) as e:
        read_edge_list(path, device=hip_device)
    assert _line_of(e) == 1
    g = read_edge_list(path, device=hip_device, skip_rows=1)
    ref.assert_same_graph(g, ref.networkx_csr([1, 2], [2, 3]))


@pytest.mark.parametrize('data', [b'', b'# only\n% comments\n\n'])
def test_files_without_edges_are_refused(tmp_path, data, hip_device):
    with pytest.raises(ValueError, match='no edges'):
        read_edge_list(_write(tmp_path, data), device=hip_device)


# ---- dw_edges_canonical ---------------------------------------------------------------------------
def canonical_ref(src, dst, w):
    ids = sorted(set(src) | set(dst))
    rank = {x: i for i, x in enumerate(ids)}
    at, edges = {}, []
    for i, (u, v) in enumerate(zip(src, dst)):
        key = (min(u, v), max(u, v))
        if key not in at:
            at[key] = len(edges)
            edges.append([(rank[u] << 32) | rank[v], None])
        edges[at[key]][1] = None if w is None else w[i]
    return ids, [e[0] for e in edges], None if w is None else [e[1] for e in edges]


def device_canonical(src, dst, w, dev):
    m = len(src)
    with torch.cuda.device(dev):
        s = torch.tensor(src, dtype=torch.int64, device=dev)
        d = torch.tensor(dst, dtype=torch.int64, device=dev)
        wt = None if w is None else torch.tensor(w, dtype=torch.float64, device=dev)
        ws = _workspace(dev, 0, m)
        ids = torch.full((2 * m,), -7, dtype=torch.int64, device=dev)
        edges = torch.full((m,), -7, dtype=torch.int64, device=dev)
        ew = None if w is None else torch.full((m,), -7.0, dtype=torch.float64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        bits = max(1, max(max(src), max(dst)).bit_length())
        _native.call('dw_edges_canonical', _native.ptr(s), _native.ptr(d), _native.ptr(wt), m,
                     bits, _native.ptr(ids), _native.ptr(edges), _native.ptr(ew),
                     _native.ptr(counts), _native.ptr(status), _native.ptr(ws), ws.numel(),
                     _native.stream(dev))
        n, e = counts.tolist()
    assert int(status.item()) == 0
    assert (ids[n:] == -7).all() and (edges[e:] == -7).all()
    return ids[:n].tolist(), edges[:e].tolist(), None if w is None else ew[:e].tolist()


def _canonical_cases():
    rng = np.random.default_rng(9)
    wide = rng.permutation(2 ** 16 + 1) * 3 + 5           # 2^16 + 1 distinct ids: 17 rank bits
    high = [(k << 33) | 5 for k in (3, 1, 2, 1, 3, 0)]     # equal below bit 32
    return {
        'm1': ([4], [2], [1.5]),
        'm1_loop': ([4], [4], None),
        'all_identical': ([7, 3, 7, 3, 7] * 60, [3, 7, 3, 7, 3] * 60, list(range(300))),
        'all_self_loops': ([5, 9, 5, 2, 9, 5] * 50, [5, 9, 5, 2, 9, 5] * 50, list(range(300))),
        'rank_17_bits': (wide.tolist(), np.roll(wide, 1).tolist(), None),
        'ids_above_bit_32': (high, high[1:] + high[:1], [float(i) for i in range(6)]),
        'first_ne_last': ([1, 2, 1, 9, 2], [2, 1, 2, 9, 1], [10.0, 20.0, 30.0, 1.0, 40.0]),
    }


@pytest.mark.parametrize('case', sorted(_canonical_cases()))
def test_canonical(case, hip_device):
    src, dst, w = _canonical_cases()[case]
    got = device_canonical(src, dst, w, hip_device)
    assert got == canonical_ref(src, dst, w)
    assert device_canonical(src, dst, w, hip_device) == got
    warr = None if w is None else np.asarray(w, dtype=np.float64)
    ref.assert_same_graph(edge_list_csr(np.asarray(src), np.asarray(dst), warr,
                                        device=hip_device),
                          edge_list_csr(np.asarray(src), np.asarray(dst), warr))
    if case == 'first_ne_last':
        assert got[2] == [40.0, 1.0]


# ---- a shuffled R-MAT 12 through text -------------------------------------------------------------
def test_shuffled_rmat12_text(tmp_path, hip_device):
    from shallow_encoders.graph.rmat import rmat_edges
    e, _ = rmat_edges(12, 30000, seed=1)
    e = e[np.random.default_rng(2).permutation(len(e))]
    path = _write(tmp_path, ''.join(f'{u}\t{v}\n' for u, v in e.tolist()).encode())
    host = read_edge_list(path)
    dev = read_edge_list(path, device=hip_device, chunk_bytes=1 << 16)
    ref.assert_same_graph(dev, host)
    d = dev.device_tensors(hip_device)
    st = torch.zeros(1, dtype=torch.int32, device=hip_device)
    _native.call('dw_csr_validate', _native.ptr(d['row_ptr']), _native.ptr(d['col']),
                 dev.vocab_size, dev.nnz, _native.ptr(st), _native.stream(hip_device))
    _native.check_status(st, 'CSR validation')
    assert dev.nnz == 2 * len(e) and dev.is_simple(hip_device)
    assert dev.require_n2v_index(hip_device)['n2v_rec'] is not None


# ---- end to end -------------------------------------------------------------------------------------
def test_dataset_walks_linkpred_and_config(tmp_path, hip_device):
    import networkx as nx
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.graph import linkpred
    from shallow_encoders.graph.datasets import EdgeListDataset, RandomWalkDataset
    path = _write(tmp_path, ''.join(f'{u} {v}\n' for u, v in nx.karate_club_graph().edges())
                  .encode())
    kw = dict(walks_per_node=2, walk_length=8, method='node2vec',
              method_params={'p': 0.5, 'q': 2}, rng='philox', seed=3)
    random.seed(0)
    ds = EdgeListDataset(path=path, build='device', **kw)
    assert ds.csr.col is None   # built in HBM
    random.seed(0)
    host = RandomWalkDataset(graph=read_edge_list(path), **kw)
    a, b = ds.next_walk_batch(40), host.next_walk_batch(40)
    assert a.shape == (40, 8) and torch.equal(a, b)

    table = torch.randn(ds.csr.vocab_size, 8, device=hip_device,
                        generator=torch.Generator(device=hip_device).manual_seed(0))
    mean, best = linkpred.edge_classification_device(table, ds.csr, 0.5, 1, 'hadamard', seed=0)
    assert np.isfinite(mean) and 0.0 <= mean <= 1.0 and best == mean

    c = load_config('sge_sg_edge_list',
                    overrides=[f'datamodule.additional_parameters.path={path}'])
    assert c.downstream.edge_classification.backend == 'device'
    random.seed(0)
    built = c.datamodule.instantiate_dataset()
    assert built.dataset.csr.col is None and len(built.vocab) == 35
    ref.assert_same_graph(built.dataset.csr, host.csr)


def test_train_and_downstream_tools_on_an_edge_list(tmp_path, hip_device):
    """tools/train.py --config-name=sge_sg_edge_list with the file as its one override (plus a
    smaller epoch), then the downstream tool: the config's device link prediction."""
    import networkx as nx
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    path = _write(tmp_path, b'source,target\n' + ''.join(
        f'{u},{v}\n' for u, v in nx.karate_club_graph().edges()).encode(), 'karate.csv')
    out = str(tmp_path / 'runs')
    base = ['--config-name', 'sge_sg_edge_list', f'path.output_dir={out}', f'output_dir={out}',
            'train.experiment=el', f'datamodule.additional_parameters.path={path}',
            'datamodule.additional_parameters.skip_rows=1',
            'datamodule.additional_parameters.walks_per_node=2',
            'datamodule.additional_parameters.walk_length=20',
            'downstream.edge_classification.n_experiments=2']
    torch.manual_seed(0)
    random.seed(0)
    train_tool.main(base)
    assert os.path.exists(os.path.join(out, 'graph_edge_list', 'el', 'checkpoints', 'last.ckpt'))
    res = downstream.main(base)
    assert set(res) == {'edge_accuracy', 'edge_best'}
    assert 0.0 <= res['edge_accuracy'] <= res['edge_best'] <= 1.0
