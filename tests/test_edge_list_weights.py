"""Weighted text edge lists, CPU side: the integer restatement of the device's decimal-to-double
conversion (tests/strtod_ref.py) against ``float()``, the power-of-five table and the kernel's
own conversion code run on the host (dw_pow5_table, dw_weight_token_host) against the
restatement, and the host path of ``weighted=True`` against a byte-at-a-time parser and networkx.
Every comparison is exact."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgelist_ref as ref  # noqa: E402
import strtod_ref as sref  # noqa: E402

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph.edge_list import (parse_lines_host, read_edge_arrays,  # noqa: E402
                                              read_edge_list)

N_TOKENS = 100_000


def _write(tmp_path, data, name='edges.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _line_of(exc):
    m = re.search(r'line (\d+)', str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _restated(name):
    """(tokens, restatement's answer per token), computed once per corpus."""
    toks = sref.corpus(name, N_TOKENS)
    return toks, [sref.token_bits(t) for t in toks]


# ---- the restatement against float() ----------------------------------------------------------
@pytest.mark.parametrize('name', sorted(sref.CORPORA))
def test_restatement_equals_float(name):
    toks, got = _restated(name)
    assert len(toks) >= N_TOKENS
    undecided = 0
    for t, b in zip(toks, got):
        assert b != sref.BAD, t
        if b is sref.UNDECIDED:
            undecided += 1
        else:
            assert b == sref.float_bits(t), t
    print(f'{name}: {undecided} undecided of {len(toks)}')
    if name in sref.NO_UNDECIDED:
        assert undecided == 0
    elif name == 'digits25':
        assert undecided <= sref.DIGITS25_CAP * len(toks)
        assert undecided > 0   # the corpus does reach the hand-over


def test_restatement_special_tokens():
    assert sref.token_bits(b'-0') == 1 << 63 and sref.token_bits(b'0e999') == 0
    assert sref.token_bits(b'5.') == sref.token_bits(b'005.000') == sref.float_bits(b'5')
    assert sref.token_bits(b'9007199254740993') == sref.float_bits(b'9007199254740992')   # tie: even
    assert sref.token_bits(b'9007199254740995') == sref.float_bits(b'9007199254740996')
    for t in sref.BAD_TOKENS:
        assert sref.token_bits(t) == sref.BAD, t
    for t in sref.OVERFLOW_TOKENS + [b'4.9e-324', b'1e-400', b'1e-310']:
        assert sref.token_bits(t) is sref.UNDECIDED, t   # overflow, subnormal, underflow


# ---- the native table and the kernel's conversion code on the host ------------------------------
def test_pow5_table_equals_python_integers():
    out = np.zeros(2 * 651, dtype=np.uint64)
    _native.call('dw_pow5_table', out.ctypes.data)
    got = out.reshape(651, 2).tolist()
    for q in range(-342, 309):
        assert tuple(got[q + 342]) == sref.pow5_entry(q), q
    assert got[342] == [1 << 63, 0]   # 5^0


def _native_token(t):
    kind, bits = ctypes.c_int32(-1), ctypes.c_uint64(0)
    _native.call('dw_weight_token_host', t, len(t), ctypes.byref(kind), ctypes.byref(bits))
    return {0: sref.BAD, 2: sref.UNDECIDED}.get(kind.value, bits.value)


@pytest.mark.parametrize('name', sorted(sref.CORPORA))
def test_native_conversion_equals_restatement(name):
    toks, want = _restated(name)
    for t, w in zip(toks[:20_000], want):
        assert _native_token(t) == w, t


def test_native_conversion_bad_and_overflow_tokens():
    for t in sref.BAD_TOKENS + [b'', b'1 ', b' 1', b'1,']:
        assert _native_token(t) == sref.BAD, t
    for t in sref.OVERFLOW_TOKENS:
        assert _native_token(t) is sref.UNDECIDED, t
    assert _native_token(b'-0') == 1 << 63
    assert _native_token(b'0' * 64) == 0 and _native_token(b'0' * 65) == sref.BAD


# ---- the host parser ----------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def test_host_parser_equals_python_parser(tmp_path):
    data = sref.FORMAT_TEXT_WEIGHTED
    src, dst, toks, _ = sref.parse_text_weighted(data)
    assert len(src) == 11 and toks[-1] == b'3.' and data.endswith(b'3.')
    want_w = [sref.float_bits(t) for t in toks]
    path = _write(tmp_path, data)
    for chunk in (1 << 20, 64, 48):   # one chunk; cut chunks (the longest line has 44 bytes)
        s, d, w = read_edge_arrays(path, chunk_bytes=chunk, weighted=True)
        assert s.dtype == np.int64 and w.dtype == np.float64
        assert (s.tolist(), d.tolist(), _bits(w)) == (src, dst, want_w), chunk
    assert _bits(w)[8] == 1 << 63   # '-0'
    s, d, w = read_edge_arrays(path, weighted=True, skip_rows=6)
    want = sref.parse_text_weighted(data, 6)
    assert (s.tolist(), d.tolist(), _bits(w)) == (want[0], want[1],
                                                 [sref.float_bits(t) for t in want[2]])
    s, d, w, n_lines = parse_lines_host(data, weighted=True)
    assert n_lines == 17 and _bits(w) == want_w


@pytest.mark.parametrize('bad', sref.BAD_LINES_WEIGHTED + [b'1 2 ' + t
                                                           for t in sref.OVERFLOW_TOKENS])
def test_host_parser_errors_name_the_line(tmp_path, bad):
    data = b'# c\n1 2 0.5\n\n' + bad + b'\n3 4 1\n' + bad + b'\n'
    with pytest.raises(ref.BadLine) as e0:
        sref.parse_text_weighted(data)
    assert e0.value.line_no == 4
    path = _write(tmp_path, data)
    for chunk in (1 << 20, 100):
        with pytest.raises(ValueError) as e:
            read_edge_arrays(path, weighted=True, chunk_bytes=max(chunk, len(bad) + 2))
        assert _line_of(e) == 4


# ---- graphs -------------------------------------------------------------------------------------
def weighted_text(src, dst, w):
    return ''.join(f'{u} {v} {x!r}\n' for u, v, x in zip(src.tolist(), dst.tolist(),
                                                          w.tolist())).encode()


def test_weighted_graph_equals_networkx(tmp_path):
    src, dst, w = ref.sparse_weighted_edges()
    path = _write(tmp_path, weighted_text(src, dst, w))
    g = read_edge_list(path, weighted=True)
    ref.assert_same_graph(g, ref.networkx_csr(src, dst, w))
    assert g.weighted and g.weights.dtype == np.float64
    # the flag off: the third column is an extra column, the graph is unweighted
    off = read_edge_list(path)
    ref.assert_same_graph(off, ref.networkx_csr(src, dst))
    assert not off.weighted and len(read_edge_arrays(path)) == 2


def test_weighted_flag_and_array_files(tmp_path):
    src, dst, w = ref.sparse_weighted_edges()
    npy = str(tmp_path / 'e.npy')
    np.save(npy, np.stack([src, dst], axis=1))
    with pytest.raises(ValueError, match='npy'):
        read_edge_list(npy, weighted=True)
    assert not read_edge_list(npy).weighted
    npz = str(tmp_path / 'e.npz')
    np.savez(npz, src=src, dst=dst, weight=w)
    for flag in (False, True):
        ref.assert_same_graph(read_edge_list(npz, weighted=flag), ref.networkx_csr(src, dst, w))


def test_dataset_parameter_host_build(tmp_path):
    from shallow_encoders.graph.datasets import EdgeListDataset
    src, dst, w = ref.sparse_weighted_edges()
    path = _write(tmp_path, weighted_text(src, dst, w))
    kw = dict(path=path, build='host', walks_per_node=1, walk_length=4)
    ds = EdgeListDataset(weighted=True, **kw)
    ref.assert_same_graph(ds.csr, ref.networkx_csr(src, dst, w))
    assert not EdgeListDataset(**kw).csr.weighted
