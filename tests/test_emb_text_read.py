"""Word2vec text back into embeddings on the host path (dw_embread_host, the kernels' token code
compiled for the CPU): read_word2vec_format against the law numpy.float32(float(token)) and the
plain-Python restatement tests/embread_ref.py — round trips of the writer, other writers'
formats, rounding boundaries, layouts, chunking, errors by line — then align_word2vec and the
downstream tool's downstream.embeddings_path.

Two of the values the feature's description lists are stated as the law gives them, not as it
words them: ``7.006492321624086e-46`` lies 0.4 ulp of a double above 2^-150, so float() gives
2^-150 itself and the tie rounds to 0 — the law is double rounding; the next double up is the
first token that gives the smallest subnormal, and it is tested beside it. ``1e39`` is a normal
double, which the conversion decides and the float32 rounding turns into inf; only ``1e-400`` and
``1e999`` lie outside the double conversion's range and go to the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import embread_ref as er
import embtext_ref as tr
from shallow_encoders import _native
from shallow_encoders.word2vec.embeddings_io import (align_word2vec, load_word2vec_format,
                                                     read_word2vec_format, save_word2vec_format)


def _finite(bits):
    return bits[(bits & 0x7F800000) != 0x7F800000]


@pytest.fixture(scope='module')
def corpus():
    """Finite float32 bit patterns: the hard values and every 4,099th pattern, as [n, 128]."""
    bits = _finite(np.concatenate([tr.hard_bits(), tr.strided_bits(4099)]))
    return bits[:len(bits) // 128 * 128].reshape(-1, 128)


@pytest.fixture(scope='module')
def small():
    """67,731 patterns (the hard values and every 65,584th), finite ones, and their floats."""
    bits = _finite(np.concatenate([tr.hard_bits(), tr.strided_bits(65584)]))
    return bits, bits.view(np.float32)


def _write(tmp_path, data: bytes, name='f.emb') -> str:
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(data)
    return path


def _bits(result) -> np.ndarray:
    return np.asarray(result.table).view(np.uint32)


FORMATS = [('%.6f', lambda v: '%.6f' % v), ('%.9g', lambda v: '%.9g' % v),
           ('%.18e', lambda v: '%.18e' % v), ('repr', lambda v: repr(float(v)))]


# ------------------------------------------------------------------------------------ round trip
def test_round_trip_of_the_writer(tmp_path, corpus):
    path = str(tmp_path / 'rt.emb')
    table = corpus.view(np.float32)
    save_word2vec_format(path, table)
    back = read_word2vec_format(path, chunk_bytes=1 << 20)      # ~10 chunks
    assert (back.n, back.d) == table.shape and isinstance(back.table, np.ndarray)
    assert back.table.dtype == np.float32
    np.testing.assert_array_equal(_bits(back), corpus)
    assert (corpus == 0x80000000).any()                          # -0.0 stays -0.0
    np.testing.assert_array_equal(back.keys_i64, np.arange(len(table)))
    assert back.host_tokens == 0
    assert back.keys()[:3] == ['0', '1', '2']
    t = np.asarray([[np.nan, 1.5, -np.inf], [np.inf, -0.0, 0.0]], dtype=np.float32)
    save_word2vec_format(path, t, keys=['x', 'y'], nonfinite='write')
    back = read_word2vec_format(path)
    assert _bits(back).tolist() == [[0x7FC00000, 0x3FC00000, 0xFF800000],
                                    [0x7F800000, 0x80000000, 0]]
    assert back.keys() == ['x', 'y'] and back.keys_i64 is None


# ------------------------------------------------------------------------------------ the law
def test_tokens_against_the_law():
    """Per token through dw_f32_token_host: whatever the conversion decides is the law's."""
    bits = _finite(np.concatenate([tr.hard_bits(), tr.strided_bits(1048583)]))
    undecided = 0
    for v in bits.view(np.float32):
        toks = [f(v) for _, f in FORMATS]
        toks += [toks[1].upper()] + ([] if toks[1].startswith('-') else ['+' + toks[1]])
        for t in toks:
            kind, got = er.token(t)
            assert kind != er.TOKEN_BAD, t
            undecided += kind == er.TOKEN_UNDECIDED
            assert kind == er.TOKEN_UNDECIDED or got == er.law(t), (t, hex(got), hex(er.law(t)))
    assert undecided == 0


FLT_TIE_UP = 2.0 ** -126 - 2.0 ** -150     # halfway between the largest subnormal and FLT_MIN
OVERFLOW = 2.0 ** 128 - 2.0 ** 103         # halfway between FLT_MAX and 2^128
HALF_UNIT = 2.0 ** -150                    # half the smallest subnormal


def _around(x):
    return [repr(float(np.nextafter(x, 0.0))), repr(x), repr(float(np.nextafter(x, np.inf)))]


BOUNDARY = [
    # the float32 tie above 1.0, and a hair to either side: the double is the tie itself, so all
    # three round to even — double rounding is the law
    ('1.00000005960464477539062500000000001', 0x3F800000),
    ('1.000000059604644775390625', 0x3F800000),
    ('1.00000005960464477539062499999999999', 0x3F800000),
    ('1.0000000596046449', 0x3F800001),
    # its neighbours' ties: below 1.0 (up to the even 1.0), above 1 + 2^-23 (up to the even)
    ('0.9999999701976776123046875', 0x3F800000), ('0.9999999701976775', 0x3F7FFFFF),
    ('1.000000178813934326171875', 0x3F800002), ('1.0000001788139342', 0x3F800001),
    ('.5', 0x3F000000), ('5.', 0x40A00000), ('+5', 0x40A00000), ('1E5', 0x47C35000),
    ('-0.0', 0x80000000), ('0', 0), ('-0', 0x80000000), ('0e0', 0),
    ('7.006492321624085e-46', 0), ('1.4e-45', 1), ('1e-45', 1), ('2.1e-45', 1), ('2.2e-45', 2),
    ('3.4028235677973366e38', 0x7F800000), ('3.4028235e38', 0x7F7FFFFF),
    ('-3.4028235677973366e38', 0xFF800000), ('1e39', 0x7F800000), ('-1e39', 0xFF800000),
    ('nan', 0x7FC00000), ('-nan', 0xFFC00000), ('NaN', 0x7FC00000), ('+nan', 0x7FC00000),
    ('inf', 0x7F800000), ('-Infinity', 0xFF800000), ('+INF', 0x7F800000),
    ('iNfInItY', 0x7F800000),
] + list(zip(_around(HALF_UNIT), [0, 0, 1])) \
  + list(zip(_around(FLT_TIE_UP), [0x007FFFFF, 0x00800000, 0x00800000])) \
  + list(zip(_around(OVERFLOW), [0x7F7FFFFF, 0x7F800000, 0x7F800000])) \
  + list(zip(_around(1.5 * 2.0 ** -149), [1, 2, 2]))
HOST_TOKENS = ['1e-400', '1e999', '-1e999', '1_0', '1e12345', '0.' + '0' * 63 + '1', '0' * 300,
               '1' + '0' * 64, '0.' + '0' * 62 + '1']
REFUSED = ['١', '0x10', '1_0x', 'abc', '1e', '--1', 'nan0', 'infin', '1.5x', '.', 'e5', '+', '1e+']


def test_boundaries_per_token():
    for t, want in BOUNDARY:
        assert er.law(t) == want, (t, hex(er.law(t)))            # the table above is the law's
        assert er.token(t) == (er.TOKEN_DECIDED, want), (t, er.token(t))
    assert er.law('7.006492321624086e-46') == 0
    assert er.token('7.006492321624086e-46') == (er.TOKEN_DECIDED, 0)
    for t in HOST_TOKENS + REFUSED:
        assert er.token(t.encode('utf-8')) == (er.TOKEN_UNDECIDED, 0), t
    assert er.token('0.' + '0' * 61 + '1')[0] == er.TOKEN_DECIDED    # 64 bytes: in the kernel
    assert er.token('')[0] == er.TOKEN_BAD and er.token('1 2')[0] == er.TOKEN_BAD


def test_boundaries_per_file(tmp_path):
    toks = [t for t, _ in BOUNDARY] + HOST_TOKENS
    data = er.file_of(range(len(toks)), [[t, '1.5'] for t in toks])
    back = read_word2vec_format(_write(tmp_path, data))
    want = [[er.law(t.encode('utf-8')), 0x3FC00000] for t in toks]
    assert _bits(back).tolist() == want
    assert back.host_tokens == len(HOST_TOKENS)
    keys, table = load_word2vec_format(_write(tmp_path, data))
    np.testing.assert_array_equal(table.view(np.uint32), _bits(back))
    h = er.host_body(data.split(b'\n', 1)[1], 2)
    assert h['n_undecided'] == len(HOST_TOKENS) and h['status'] == 0
    assert [u[:2] for u in h['undecided']] == [(len(BOUNDARY) + i, 0)
                                               for i in range(len(HOST_TOKENS))]
    assert (h['table'][len(BOUNDARY):, 0] == 0).all()            # 0.0 until the host patches it


@pytest.mark.parametrize('name,fmt', FORMATS)
def test_other_writers_formats_per_file(tmp_path, small, name, fmt):
    _, vals = small
    vals = vals[:len(vals) // 64 * 64].reshape(-1, 64)
    rows = [[fmt(v) for v in r] for r in vals]
    path = _write(tmp_path, er.file_of([f'w{i}' for i in range(len(rows))], rows))
    back = read_word2vec_format(path, chunk_bytes=1 << 18)
    want = np.asarray([[er.law(t) for t in r] for r in rows], dtype=np.uint32)
    np.testing.assert_array_equal(_bits(back), want)
    assert back.keys()[-1] == f'w{len(rows) - 1}' and back.keys_i64 is None


# ------------------------------------------------------------------------------------ the cap
def test_real_corpora_leave_nothing_to_the_host(small):
    """The writer's shortest tokens and the %.6f / %.9g / %.18e forms of float32 values are all
    decided by the conversion itself: a reader that leans on the host's float() cannot pass."""
    bits, vals = small
    assert len(bits) == 67731
    rng = np.random.default_rng(0)
    normal = rng.normal(0, 0.3, size=20000).astype(np.float32)
    hard = _finite(tr.hard_bits()).view(np.float32)
    hard = hard[rng.permutation(len(hard))][:5000]
    corpora = [(tr.tokens(vals), bits)]
    corpora += [([f(v) for v in normal], None) for _, f in FORMATS[:3]]
    corpora += [(['%.18e' % v for v in hard], hard.view(np.uint32))]
    for toks, want in corpora:
        body = ''.join(f'{i} {t}\n' for i, t in enumerate(toks)).encode()
        h = er.host_body(body, 1)
        assert h['n_undecided'] == 0 and h['status'] == 0 and h['lines'] == len(toks)
        law = np.asarray([er.law(t) for t in toks], dtype=np.uint32)
        np.testing.assert_array_equal(h['table'][:, 0], law)
        if want is not None:
            np.testing.assert_array_equal(law, want)
        np.testing.assert_array_equal(h['key_i64'], np.arange(len(toks)))


# ------------------------------------------------------------------------------------ layouts
def _same(a, b):
    for k in ('table', 'key_off', 'key_len', 'key_i64'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ('lines', 'err_line', 'status'):
        assert a[k] == b[k], k


LAYOUTS = [
    b'a 1 2\r\nb 3 4\r\n',                       # CRLF
    b'a 1 2\nb 3 4',                             # no final newline
    b'a 1 2\r\nb 3 4\r',                         # ... and a bare \r at the end
    b'  a \t 1\t\t2  \n\tb   3 4\t \n',          # runs of blanks and tabs, trailing blanks
    'nœud√ 1 2\né 3 4\n'.encode('utf-8'),
    b'007 1 2\n+5 3 4\n1234567890123456789 5 6\n0 7 8\n123456789012345678 9 10\n00 1 1\n',
    b'a 1\x0b2\x0c\n',                           # \v and \f separate tokens, as bytes.split()
]


@pytest.mark.parametrize('case', range(len(LAYOUTS)))
def test_layouts(tmp_path, case):
    body = LAYOUTS[case]
    r, h = er.read_body(body, 2), er.host_body(body, 2)
    assert r['status'] & er.S_BAD_TEXT == 0 and h['n_undecided'] == 0
    _same(r, h)
    n = r['lines']
    back = read_word2vec_format(_write(tmp_path, f'{n} 2\n'.encode() + body))
    keys, table = load_word2vec_format(_write(tmp_path, f'{n} 2\n'.encode() + body))
    assert back.keys() == keys
    np.testing.assert_array_equal(_bits(back), table.view(np.uint32))
    if case == 5:
        assert h['key_i64'].tolist() == [-1, -1, -1, 0, 123456789012345678, -1]
        assert back.keys_i64 is None and h['status'] == er.S_TEXT_KEY
        assert back.keys()[:4] == ['007', '+5', '1234567890123456789', '0']
    elif case == 4:
        assert back.keys_i64 is None and back.keys() == ['nœud√', 'é']
    ints = read_word2vec_format(_write(tmp_path, b'3 1\n0 1\n10 2\n999999999999999999 3\n'))
    assert ints.keys_i64.tolist() == [0, 10, 10 ** 18 - 1]


@pytest.mark.parametrize('d', [1, 2, 63, 64, 65, 128, 512])
def test_one_line_of_d_values(tmp_path, d):
    vals = np.random.default_rng(d).normal(0, 0.3, size=d).astype(np.float32)
    path = str(tmp_path / 'one.emb')
    save_word2vec_format(path, vals.reshape(1, d), keys=[77])
    back = read_word2vec_format(path)
    np.testing.assert_array_equal(back.table, vals.reshape(1, d))
    assert back.keys_i64.tolist() == [77]
    body = open(path, 'rb').read().split(b'\n', 1)[1]
    _same(er.read_body(body, d), er.host_body(body, d))
    for other in (d - 1, d + 1):
        if 1 <= other <= 512:
            h = er.host_body(body, other)
            assert h['status'] == er.S_BAD_TEXT and h['err_line'] == 0
            assert not h['table'].any() and not h['key_len'].any()   # nothing of it is stored


def test_long_tokens(tmp_path):
    t64, t65, t300 = '1.' + '0' * 62, '1.' + '0' * 63, '0' * 300
    assert (len(t64), len(t65)) == (64, 65)
    body = f'k {t64} {t65} {t300} 2.5\n'.encode()
    r, h = er.read_body(body, 4), er.host_body(body, 4)
    assert [u[1:] for u in h['undecided']] == [(1, 2 + 65, 65), (2, 2 + 65 + 66, 300)]
    assert h['table'][0].tolist() == [0x3F800000, 0, 0, 0x40200000]
    back = read_word2vec_format(_write(tmp_path, b'1 4\n' + body))
    np.testing.assert_array_equal(_bits(back), r['table'])
    assert _bits(back)[0].tolist() == [0x3F800000, 0x3F800000, 0, 0x40200000]


def test_chunk_sizes_give_the_same_arrays(tmp_path):
    rng = np.random.default_rng(1)
    table = rng.normal(0, 0.3, size=(37, 5)).astype(np.float32)
    keys = [f'k{i}' if i % 3 else str(i) for i in range(37)]
    path = str(tmp_path / 'c.emb')
    save_word2vec_format(path, table, keys=keys)
    line = len(open(path, 'rb').read().split(b'\n')[1]) + 1
    whole = read_word2vec_format(path)
    np.testing.assert_array_equal(whole.table, table)
    assert whole.keys() == keys and whole.keys_i64 is None
    for chunk in (1, 64, line - 1, line, line + 1, 3 * line + 2):
        got = read_word2vec_format(path, chunk_bytes=chunk)
        np.testing.assert_array_equal(_bits(got), _bits(whole), err_msg=str(chunk))
        assert got.keys() == keys, chunk
    with pytest.raises(ValueError):
        read_word2vec_format(path, chunk_bytes=0)


# ------------------------------------------------------------------------------------ errors
ERRORS = [
    (b'3 2\na 1 2\nb 3 4\n', 1),              # fewer lines than announced
    (b'1 2\na 1 2\nb 3 4\n', 1),              # more
    (b'x 2\na 1 2\n', 1),
    (b'2 2\na 1 2\nb 3\n', 3),                # short
    (b'2 2\na 1 2 3\nb 3 4\n', 2),            # long
    (b'2 2\na 1 2\nb 3 4x\n', 3),             # unparsable
    (b'', 1),
    (b'3 2\na 1 2\n\nb 3 4\n', 3),            # an empty line in the middle
    (b'3 2\na 1 2\n \t \nb 3 4\n', 3),        # ... and an all-blank one
    (b'2 2\na 1_0x 2\nb 3 4\n', 2),           # a token outside every grammar
    (b'2 2\na 1 2\nb 3\nc 5 6\n', 1),         # a bad line, but the count is checked first
    (b'2 2\n\xff 1 2\nb 3 4\n', 2),           # a key that is not UTF-8
    (b'2 0\na\nb\n', 1), (b'-1 2\n', 1), (b'2\na 1\n', 1),
]


@pytest.mark.parametrize('case', range(len(ERRORS)))
def test_errors_name_the_line_the_loader_names(tmp_path, case):
    text, line = ERRORS[case]
    path = _write(tmp_path, text)
    with pytest.raises(ValueError, match=rf'line {line}\b'):
        load_word2vec_format(path)
    for chunk in (256 << 20, 1):
        with pytest.raises(ValueError, match=rf'line {line}\b'):
            read_word2vec_format(path, chunk_bytes=chunk)


def test_a_bad_line_in_the_second_chunk(tmp_path):
    good = ''.join(f'{i} 1.5 2.5\n' for i in range(40))
    text = ('42 2\n' + good + '40 1.5\n41 1 2\n').encode()
    path = _write(tmp_path, text)
    for chunk in (len(good) + 5, 100, 1):
        with pytest.raises(ValueError, match=r'line 42\b'):
            read_word2vec_format(path, chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r'line 42\b'):
        load_word2vec_format(path)
    text = ('42 2\n' + good + '40 1.5 zz\n41 1 2\n').encode()
    with pytest.raises(ValueError, match=r'line 42\b'):
        read_word2vec_format(_write(tmp_path, text), chunk_bytes=100)


def test_native_refusals_and_the_undecided_capacity():
    lib = _native.load()
    rc = lib.dw_embread_parse(1, 8, 1, 1, 513, 1, 1, 1, 0, 1, 1, 1, None, 0, 1, 1, 1, None)
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()
    rc = lib.dw_embread_host(1, 8, 513, 1, 1, 0, 1, 1, 1, None, 0, 1, 1, 1)
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()
    rc = lib.dw_embread_parse(1, 8, 1, 2, 4, 1, 1, 1, 0, 1, 1, 1, None, 0, 1, 1, 1, None)
    assert rc == _native.DW_E_INVALID_ARG                        # two lines, a table of one row
    body = b'a 1e999 1e-400\nb 1e999 2\n'
    full, short = er.host_body(body, 2), er.host_body(body, 2, undecided_capacity=2)
    assert full['n_undecided'] == short['n_undecided'] == 3      # dropped, but counted
    assert short['undecided'] == full['undecided'][:2]
    assert er.host_body(b'', 2)['lines'] == 0 and er.host_body(b'\n', 2)['err_line'] == 0
    # lines behind the table's last row are counted, not parsed
    h = er.host_body(b'a 1 2\nb 3 4\nc 5\n', 2, n_rows=2)
    assert h['lines'] == 3 and h['status'] == er.S_TEXT_KEY and h['err_line'] == -1


# ------------------------------------------------------------------------------------ alignment
def _edge_list_graph(ids):
    from shallow_encoders.graph.csr import CSRGraph, IdNames
    ids = np.sort(np.asarray(ids, dtype=np.int64))
    return CSRGraph.from_arrays(np.zeros(len(ids) + 2, dtype=np.int64),
                                np.zeros(0, dtype=np.int32), itos=IdNames(ids))


def test_align_integer_ids(tmp_path):
    rng = np.random.default_rng(0)
    ids = np.sort(rng.choice(10 ** 6, size=64, replace=False)).astype(np.int64)
    g = _edge_list_graph(ids)
    table = rng.normal(0, 0.3, size=(65, 5)).astype(np.float32)
    perm = rng.permutation(64)
    path = str(tmp_path / 'a.emb')
    save_word2vec_format(path, table, keys=ids[perm], rows=perm + 1)
    got = align_word2vec(read_word2vec_format(path), g)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (65, 5)
    np.testing.assert_array_equal(got[1:], table[1:])
    assert not got[0].any()
    # <unk> and string keys, and the token style: through the dict
    save_word2vec_format(path, table, keys=g.export_keys('id', include_unk=True))
    np.testing.assert_array_equal(align_word2vec(read_word2vec_format(path), g), table)
    save_word2vec_format(path, table, keys=g.export_keys('token', include_unk=True))
    np.testing.assert_array_equal(align_word2vec(read_word2vec_format(path), g, style='token'),
                                  table)
    with pytest.raises(ValueError, match='not in the vocabulary'):
        align_word2vec(read_word2vec_format(path), g)
    # a subset
    save_word2vec_format(path, table, keys=ids[perm[:40]], rows=perm[:40] + 1)
    sub = read_word2vec_format(path)
    with pytest.raises(ValueError, match='24 vocabulary rows'):
        align_word2vec(sub, g)
    got = align_word2vec(sub, g, missing='zero')
    want = np.zeros_like(table)
    want[perm[:40] + 1] = table[perm[:40] + 1]
    np.testing.assert_array_equal(got, want)
    # a duplicate and an unknown key name the key and its line
    keys = ids[perm].copy()
    keys[9] = keys[3]
    save_word2vec_format(path, table, keys=keys, rows=perm + 1)
    with pytest.raises(ValueError, match=rf"'{keys[3]}' \(line 11\) occurs twice"):
        align_word2vec(read_word2vec_format(path), g)
    unknown = next(i for i in range(10 ** 6) if i not in set(ids.tolist()))
    keys[9] = unknown
    save_word2vec_format(path, table, keys=keys, rows=perm + 1)
    with pytest.raises(ValueError, match=rf'key {unknown} \(line 11\) is not in the vocabulary'):
        align_word2vec(read_word2vec_format(path), g, missing='zero')
    with pytest.raises(ValueError):
        align_word2vec(sub, g, missing='skip')


def test_align_node_numbers_and_names(tmp_path):
    import networkx as nx
    from shallow_encoders.graph.csr import CSRGraph, NodeNames
    rng = np.random.default_rng(1)
    table = rng.normal(0, 0.3, size=(9, 3)).astype(np.float32)
    g = CSRGraph.from_arrays(np.zeros(10, dtype=np.int64), np.zeros(0, dtype=np.int32),
                             itos=NodeNames(8, 7))
    path = str(tmp_path / 'n.emb')
    perm = rng.permutation(8)
    save_word2vec_format(path, table, keys=perm, rows=perm + 1)
    np.testing.assert_array_equal(align_word2vec(read_word2vec_format(path), g)[1:], table[1:])
    save_word2vec_format(path, table, keys=[8], rows=[1])
    with pytest.raises(ValueError, match=r'key 8 \(line 2\)'):
        align_word2vec(read_word2vec_format(path), g, missing='zero')
    g = CSRGraph.from_networkx(nx.relabel_nodes(nx.path_graph(3), {0: 'B1', 1: 'a2', 2: 'c3'}))
    t = table[:4]
    save_word2vec_format(path, t, keys=['c3', 'B1', 'a2'], rows=[3, 2, 1])
    np.testing.assert_array_equal(align_word2vec(read_word2vec_format(path), g)[1:], t[1:])
    save_word2vec_format(path, t, keys=['c3', 'B1', 'c3'], rows=[3, 2, 1])
    with pytest.raises(ValueError, match=r"'c3' \(line 4\) occurs twice"):
        align_word2vec(read_word2vec_format(path), g)
    # a plain vocabulary: a list of tokens
    save_word2vec_format(path, t, keys=['<unk>', 'x', 'y', 'z'])
    np.testing.assert_array_equal(
        align_word2vec(read_word2vec_format(path), ['<unk>', 'z', 'y', 'x']), t[[0, 3, 2, 1]])


def karate_checkpoint(out):
    """The hand-made karate checkpoint of test_emb_text.py's export test; returns its input
    table and the tools' common arguments."""
    from shallow_encoders.config_parser import load_config
    from tools import conventions
    cfg = load_config('sge_sg_karate_club', overrides=[f'path.output_dir={out}'])
    assert cfg.downstream.embeddings_path is None and cfg.downstream.embeddings_missing == 'error'
    rng = np.random.default_rng(0)
    w_in = rng.normal(0, 0.3, size=(35, 4)).astype(np.float32)
    w_out = rng.normal(0, 0.3, size=(35, 4)).astype(np.float32)
    ck = conventions.get_checkpoint_path(out, cfg.datamodule.dataset_name, cfg.train.experiment,
                                         'last.ckpt')
    os.makedirs(os.path.dirname(ck))
    torch.save({'state_dict': {'_model._input_embedding.weight': torch.from_numpy(w_in),
                               '_model._output_embedding.weight': torch.from_numpy(w_out)}}, ck)
    return w_in, ['--config-name', 'sge_sg_karate_club', f'path.output_dir={out}',
                  f'output_dir={out}', 'downstream.node_classification.n_experiments=3',
                  'downstream.node_classification.visualize=false',
                  'downstream.edge_classification.n_experiments=3']


def test_downstream_tool_scores_the_exported_file(tmp_path):
    from shallow_encoders.config_parser import load_config
    from tools import export_embeddings
    from tools import graph_model_downstream_classification as downstream
    w_in, argv = karate_checkpoint(str(tmp_path / 'runs'))
    path = export_embeddings.main(argv + ['export.device=cpu'])
    from_checkpoint = downstream.main(argv)
    from_file = downstream.main(argv + [f'downstream.embeddings_path={path}'])
    assert set(from_file) == {'node_accuracy', 'node_best', 'edge_accuracy', 'edge_best'}
    assert from_file == from_checkpoint
    # a file that lacks nodes: refused, or scored with zero rows
    back = read_word2vec_format(path)
    np.testing.assert_array_equal(back.table, w_in[1:])
    part = str(tmp_path / 'part.emb')
    save_word2vec_format(part, back.table[:30], keys=back.keys()[:30])
    with pytest.raises(ValueError, match='4 vocabulary rows'):
        downstream.main(argv + [f'downstream.embeddings_path={part}'])
    res = downstream.main(argv + [f'downstream.embeddings_path={part}',
                                  'downstream.embeddings_missing=zero'])
    assert set(res) == set(from_file)
    with pytest.raises(ValueError):
        load_config('sge_sg_karate_club', overrides=['downstream.embeddings_missing=skip'])
