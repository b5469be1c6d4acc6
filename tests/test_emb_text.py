"""Embeddings as word2vec text on the host path (dw_embtext_host, the kernels' code compiled for
the CPU): tokens and files byte for byte against tests/embtext_ref.py (numpy's unique-mode digits
in CPython's repr layout), the loader, the key helper and tools/export_embeddings.py."""
import os
import re

import numpy as np
import pytest
import torch

import embtext_ref as ref
from shallow_encoders.word2vec.embeddings_io import load_word2vec_format, save_word2vec_format


@pytest.fixture(scope='module')
def corpus():
    """(bits, reference tokens) of the hard values and of every 4,099th bit pattern."""
    bits = np.concatenate([ref.hard_bits(), ref.strided_bits()])
    return bits, ref.tokens(bits.view(np.float32))


def _digits(tok: str) -> int:
    m = re.fullmatch(r'-?(\d+)(?:\.(\d+))?(?:e[-+]\d+)?', tok)
    return len((m.group(1) + (m.group(2) or '')).strip('0')) if m else 0


# ------------------------------------------------------------------------------------ tokens
def test_tokens_equal_the_reference(corpus):
    bits, want = corpus
    got = ref.host_tokens(bits)
    bad = [(hex(b), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])
    nd = np.asarray([_digits(t) for t in want])
    assert (nd == 9).sum() >= 1000 and (nd == 1).sum() >= 100
    assert max(len(t) for t in want) == ref.MAX_TOKEN
    assert want[list(bits).index(0x80000000)] == '-0.0'


def test_reference_examples():
    """The rule itself, on the issue's examples (repr's layout, not str(float32)'s)."""
    for x, t in [(1e-4, '0.0001'), (1e-5, '1e-05'), (1.0, '1.0'), (9999999e9, '9999999000000000.0'),
                 (1e16, '1e+16'), (1.1754944e-38, '1.1754944e-38'), (-0.0, '-0.0'),
                 (float('inf'), 'inf'), (float('-inf'), '-inf'), (float('nan'), 'nan'),
                 (16777216.0, '16777216.0'), (1e-45, '1e-45'), (3.4028235e38, '3.4028235e+38')]:
        assert ref.token(x) == t
        assert ref.host_tokens(np.float32(x).reshape(1).view(np.uint32)) == [t]


def test_tokens_round_trip(corpus):
    bits, want = corpus
    fin = (bits & 0x7F800000) != 0x7F800000
    back = np.asarray([float(t) for t in want], dtype=np.float64).astype(np.float32)
    np.testing.assert_array_equal(back.view(np.uint32)[fin], bits[fin])


# ------------------------------------------------------------------------------------ files
def _table(n, d, seed=0):
    """Hard values first, random bit patterns behind them; finite."""
    rng = np.random.default_rng(seed)
    bits = np.concatenate([ref.hard_bits(), rng.integers(0, 1 << 32, size=n * d, dtype=np.uint64)
                           .astype(np.uint32)])
    bits = bits[(bits & 0x7F800000) != 0x7F800000]
    rng.shuffle(bits)
    return bits[:n * d].view(np.float32).reshape(n, d).copy()


@pytest.mark.parametrize('n,d', [(1, 1), (2, 3), (65, 128)])
def test_files_equal_the_restatement(tmp_path, n, d):
    table = _table(n, d, seed=n)
    path = str(tmp_path / 'a.emb')
    size = save_word2vec_format(path, table)
    want = ref.file_bytes(range(n), table)
    data = open(path, 'rb').read()
    assert data == want and size == len(want)
    assert b'\r' not in data and b' \n' not in data and b'  ' not in data
    # a torch tensor, str keys with multibyte UTF-8, int64 keys with 0 and 10^18 - 1
    names = [f'nœud{i}√' for i in range(n)]
    save_word2vec_format(path, torch.from_numpy(table), keys=names)
    assert open(path, 'rb').read() == ref.file_bytes(names, table)
    ids = (np.arange(n, dtype=np.int64) * 7919) % (10 ** 18)
    ids[0], ids[-1] = 0, 10 ** 18 - 1
    save_word2vec_format(path, table, keys=ids)
    assert open(path, 'rb').read() == ref.file_bytes([int(i) for i in ids], table)
    save_word2vec_format(path, table, keys=torch.from_numpy(ids))
    assert open(path, 'rb').read() == ref.file_bytes([int(i) for i in ids], table)


def test_rows_chunks_and_unk(tmp_path):
    table = _table(65, 5, seed=3)
    rows = np.asarray([64, 0, 3, 3, 17, 64, 1, 0], dtype=np.int64)
    keys = [f'k{i}' for i in range(len(rows))]
    want = ref.file_bytes(keys, table[rows])
    path = str(tmp_path / 'r.emb')
    for chunk in (256 << 20, 1, 100, len(want) // 2):   # < one line, a few lines, mid-table
        save_word2vec_format(path, table, keys=keys, rows=rows, chunk_bytes=chunk)
        assert open(path, 'rb').read() == want, chunk
    # <unk> (row 0) skipped: rows 1 .. V - 1 under the graph's own keys
    from shallow_encoders.graph.csr import CSRGraph, IdNames, NodeNames
    ids = np.sort(np.random.default_rng(0).choice(10 ** 6, size=64, replace=False)).astype(np.int64)
    row_ptr = np.zeros(66, dtype=np.int64)
    g = CSRGraph.from_arrays(row_ptr, np.zeros(0, dtype=np.int32), itos=IdNames(ids))
    k = g.export_keys()
    assert k.dtype == np.int64 and list(k) == list(ids)
    assert g.export_keys('token')[:2] == [f'n{ids[0]:07d}', f'n{ids[1]:07d}']
    assert g.export_keys('id', include_unk=True)[:2] == ['<unk>', str(ids[0])]
    save_word2vec_format(path, table, keys=k, rows=np.arange(1, 65))
    assert open(path, 'rb').read() == ref.file_bytes([int(i) for i in ids], table[1:])
    g = CSRGraph.from_arrays(row_ptr, np.zeros(0, dtype=np.int32), itos=NodeNames(64, 7))
    assert list(g.export_keys()) == list(range(64))
    assert g.export_keys('token', include_unk=True)[:2] == ['<unk>', 'n0000000']
    import networkx as nx
    g = CSRGraph.from_networkx(nx.relabel_nodes(nx.path_graph(3), {0: 'B1', 1: 'a2', 2: 'c3'}))
    assert g.export_keys() == ['a2', 'B1', 'c3'] and g.export_keys('token') == ['a2', 'b1', 'c3']
    with pytest.raises(ValueError):
        g.export_keys('name')


def test_host_row_ranges_concatenate():
    table = _table(65, 3, seed=5)
    whole, line_off, st = ref.host_lines(table)
    assert st == 0 and whole == ref.file_bytes(range(65), table).split(b'\n', 1)[1]
    lens = [len(ln) + 1 for ln in whole.decode().split('\n')[:-1]]
    np.testing.assert_array_equal(line_off, np.concatenate([[0], np.cumsum(lens)]))
    for cut in range(66):
        a = ref.host_lines(table, r0=0, r1=cut)[0]
        b = ref.host_lines(table, r0=cut, r1=65)[0]
        assert a + b == whole


# ------------------------------------------------------------------------------------ round trip
def test_load_save_round_trip(tmp_path, corpus):
    bits, _ = corpus
    fin = bits[(bits & 0x7F800000) != 0x7F800000]
    fin = fin[:len(fin) // 128 * 128].view(np.float32).reshape(-1, 128)
    path = str(tmp_path / 'rt.emb')
    save_word2vec_format(path, fin, chunk_bytes=1 << 20)
    keys, back = load_word2vec_format(path)
    assert keys == [str(i) for i in range(len(fin))] and back.dtype == np.float32
    np.testing.assert_array_equal(back.view(np.uint32), fin.view(np.uint32))   # -0.0 stays -0.0
    assert (back.view(np.uint32) == 0x80000000).any()
    t = np.asarray([[np.nan, 1.5, -np.inf]], dtype=np.float32)
    save_word2vec_format(path, t, keys=['x'], nonfinite='write')
    assert open(path, 'rb').read() == b'1 3\nx nan 1.5 -inf\n'
    keys, back = load_word2vec_format(path)
    assert keys == ['x'] and np.isnan(back[0, 0]) and back[0, 1] == 1.5 and back[0, 2] == -np.inf


def test_loader_reads_other_writers(tmp_path):
    vals = np.random.default_rng(1).normal(0, 0.3, size=(7, 4)).astype(np.float32)
    path = str(tmp_path / 'f.emb')
    toks = [[f'{v:.6f}' for v in row] for row in vals]
    with open(path, 'w') as f:
        f.write('7 4\n' + ''.join(f'w{i} ' + ' '.join(r) + '\n' for i, r in enumerate(toks)))
    keys, back = load_word2vec_format(path)
    assert keys == [f'w{i}' for i in range(7)]
    want = np.asarray([[np.float32(float(t)) for t in r] for r in toks], dtype=np.float32)
    np.testing.assert_array_equal(back.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------ errors
def test_save_errors(tmp_path):
    path = str(tmp_path / 'e.emb')
    t = np.ones((4, 3), dtype=np.float32)
    t[2, 1] = np.inf
    t[3, 0] = np.nan
    with pytest.raises(ValueError, match=r'row 2, column 1'):
        save_word2vec_format(path, t)
    assert not os.path.exists(path)
    with pytest.raises(ValueError, match=r'row 3, column 0'):
        save_word2vec_format(path, t, rows=[3, 2])
    assert not os.path.exists(path)
    save_word2vec_format(path, t, rows=[0, 1])      # the bad rows are not written: no error
    t = np.ones((4, 3), dtype=np.float32)
    for bad in ('a b', 'a\tb', 'a\n', ''):
        with pytest.raises(ValueError, match='key 1'):
            save_word2vec_format(path, t, keys=['x', bad, 'y', 'z'])
    with pytest.raises(ValueError):
        save_word2vec_format(path, t, keys=['x'])
    with pytest.raises(ValueError):
        save_word2vec_format(path, t, keys=np.asarray([0, 1, -1, 2]))
    for rows in ([0, 4], [-1]):
        with pytest.raises(IndexError):
            save_word2vec_format(path, t, rows=rows)
    with pytest.raises(ValueError):
        save_word2vec_format(path, t.astype(np.float64))
    with pytest.raises(ValueError):
        save_word2vec_format(path, t, nonfinite='skip')


@pytest.mark.parametrize('text,line', [
    (b'3 2\na 1 2\nb 3 4\n', 1),              # fewer lines than announced
    (b'1 2\na 1 2\nb 3 4\n', 1),              # more
    (b'x 2\na 1 2\n', 1),
    (b'2 2\na 1 2\nb 3\n', 3),                # short
    (b'2 2\na 1 2 3\nb 3 4\n', 2),            # long
    (b'2 2\na 1 2\nb 3 4x\n', 3),             # unparsable
    (b'', 1),
])
def test_loader_errors_name_the_line(tmp_path, text, line):
    path = str(tmp_path / 'bad.emb')
    open(path, 'wb').write(text)
    with pytest.raises(ValueError, match=rf'line {line}\b'):
        load_word2vec_format(path)


def test_native_refusals():
    import ctypes
    from shallow_encoders import _native
    lib = _native.load()
    t = np.ones((2, 2), dtype=np.float32)
    lo = np.zeros(3, dtype=np.int64)
    k = np.arange(2, dtype=np.int64)
    st = ctypes.c_int32(0)
    out = np.full(64, 0xA5, dtype=np.uint8)
    args = (t.ctypes.data, 2, 2, None, 2, k.ctypes.data, None, None, lo.ctypes.data)
    assert lib.dw_embtext_host(*args, 0, 2, None, 0, ctypes.byref(st)) == 0
    assert lo[2] == len(b'0 1.0 1.0\n1 1.0 1.0\n')
    rc = lib.dw_embtext_host(*args, 0, 2, out.ctypes.data, int(lo[2]) - 1, ctypes.byref(st))
    assert rc == _native.DW_E_INVALID_ARG and (out == 0xA5).all()   # one byte short: no write
    assert b'need 20 bytes' in lib.dw_last_error_string()
    # the device entry points refuse dim > 512 before any launch (no device is touched)
    rc = lib.dw_embtext_sizes(1, 2, 513, None, 2, 1, None, None, 1, 1, 1, 1, 0, None)
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()
    rc = lib.dw_embtext_write(1, 2, 513, None, 2, 1, None, None, 1, 1, 0, 2, 1, 0, 1, None)
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()


# ------------------------------------------------------------------------------------ tool
def test_export_tool_on_a_karate_checkpoint(tmp_path):
    from shallow_encoders.config_parser import load_config
    from tools import conventions, export_embeddings
    out = str(tmp_path / 'runs')
    cfg = load_config('sge_sg_karate_club', overrides=[f'path.output_dir={out}'])
    assert cfg.export.table == 'input' and cfg.export.keys == 'id' and not cfg.export.include_unk
    assert cfg.export.nonfinite == 'error' and cfg.export.device == 'auto'
    assert cfg.export.path is None
    V = 35
    rng = np.random.default_rng(0)
    w_in = rng.normal(0, 0.3, size=(V, 4)).astype(np.float32)
    w_out = rng.normal(0, 0.3, size=(V, 4)).astype(np.float32)
    ck = conventions.get_checkpoint_path(out, cfg.datamodule.dataset_name, cfg.train.experiment,
                                         'last.ckpt')
    os.makedirs(os.path.dirname(ck))
    torch.save({'state_dict': {'_model._input_embedding.weight': torch.from_numpy(w_in),
                               '_model._output_embedding.weight': torch.from_numpy(w_out)}}, ck)
    argv = ['--config-name', 'sge_sg_karate_club', f'path.output_dir={out}', f'output_dir={out}',
            'export.device=cpu']
    path = export_embeddings.main(argv)
    assert path == os.path.join(out, cfg.datamodule.dataset_name, cfg.train.experiment, 'analysis',
                                'embeddings.emb')
    names = [f'n{i:02d}' for i in range(1, 35)]
    data = open(path, 'rb').read()
    assert data.count(b'\n') == 35 and data == ref.file_bytes(names, w_in[1:])
    keys, table = load_word2vec_format(path)
    assert keys == names
    np.testing.assert_array_equal(table, w_in[1:])
    other = str(tmp_path / 'o.emb')
    export_embeddings.main(argv + ['export.table=output', 'export.include_unk=true',
                                   f'export.path={other}'])
    keys, table = load_word2vec_format(other)
    assert keys == ['<unk>'] + names
    np.testing.assert_array_equal(table, w_out)
    with pytest.raises(ValueError):
        load_config('sge_sg_karate_club', overrides=['export.table=both'])
