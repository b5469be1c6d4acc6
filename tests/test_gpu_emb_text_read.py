"""The embedding text reader's kernels (csrc/dw_embread.hip) against the host path
(dw_embread_host), which tests/test_emb_text_read.py pins to numpy.float32(float(token)): the
same table bits, key spans, integer keys, line count, error line, status and undecided set, on the
CPU tests' files and at the smallest shapes at which the kernels take another path — a line
shorter than a lane's 32 bytes, a line of exactly one 2 KiB tile and one byte more, tokens across
a tile's edge and across the end of the staged bytes, more tokens in a tile than lanes, every
alignment of the text's base, one line and 3,001 lines."""
import ctypes

import numpy as np
import pytest
import torch

import embread_ref as er
import embtext_ref as tr
import test_emb_text_read as cpu
from shallow_encoders import _native
from shallow_encoders.word2vec.embeddings_io import (pow5_table, read_word2vec_format,
                                                     save_word2vec_format)

pytestmark = pytest.mark.gpu

TILE, STAGED = 2048, 2128      # dw_embread.hip: TILE, TILE + OVER
GUARD = 3                      # sentinel rows in front of and behind every output
SENTINEL = 0x5A


def device_body(dev, body: bytes, d: int, n_rows=None, row0: int = 0, shift: int = 0,
                tail: bytes = b'', undecided_capacity: int = 4096, runs: int = 1):
    """host_body's dict from the two kernels. The text starts ``shift`` bytes behind a 256-byte
    boundary and has ``tail`` behind its n_bytes; every output lies between GUARD rows of a
    sentinel, which must come back untouched; ``runs`` > 1 repeats the parse into fresh outputs
    and requires the same bits."""
    n_bytes = len(body)
    if n_rows is None:
        n_rows = row0 + body.count(b'\n') + (1 if body and not body.endswith(b'\n') else 0)
    buf = torch.from_numpy(np.frombuffer(b'\xff' * shift + body + tail + b'\xff' * 16,
                                         dtype=np.uint8).copy()).to(dev)
    assert buf.data_ptr() % 256 == 0
    text = buf.data_ptr() + shift
    pow5 = pow5_table(dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_embread_workspace_bytes', n_bytes, ctypes.byref(nb))
    ws = torch.empty(max(1, nb.value), dtype=torch.uint8, device=dev)
    st = _native.stream(dev)
    first = None
    for _ in range(runs):
        def guarded(rows, width, dtype):
            t = torch.zeros((rows + 2 * GUARD) * width, dtype=dtype, device=dev)
            t.view(torch.uint8)[:GUARD * width * t.element_size()] = SENTINEL
            t.view(torch.uint8)[(GUARD + rows) * width * t.element_size():] = SENTINEL
            return t

        def inner(t, rows, width):
            a = t.cpu().numpy()
            lo, hi = GUARD * width, (GUARD + rows) * width
            assert (a[:lo].view(np.uint8) == SENTINEL).all(), 'a write in front of an output'
            assert (a[hi:].view(np.uint8) == SENTINEL).all(), 'a write behind an output'
            return a[lo:hi]
        table = guarded(n_rows, d, torch.float32)
        key_off, key_len, key_i64 = (guarded(n_rows, 1, torch.int64) for _ in range(3))
        und = guarded(undecided_capacity, 4, torch.int64)
        line_off = guarded(n_rows - row0 + 1, 1, torch.int64)
        counts = torch.full((2,), -5, dtype=torch.int64, device=dev)
        err = torch.full((1,), -7, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_embread_lines', text, n_bytes, line_off.data_ptr() + 8 * GUARD,
                     n_rows - row0, counts.data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel(),
                     st)
        lines = int(counts[0].item())
        parsed = min(lines, n_rows - row0)
        _native.call('dw_embread_parse', text, n_bytes, line_off.data_ptr() + 8 * GUARD, parsed,
                     d, pow5.data_ptr(), table.data_ptr() + 4 * GUARD * d, n_rows, row0,
                     key_off.data_ptr() + 8 * GUARD, key_len.data_ptr() + 8 * GUARD,
                     key_i64.data_ptr() + 8 * GUARD, und.data_ptr() + 32 * GUARD,
                     undecided_capacity, counts.data_ptr(), err.data_ptr(), status.data_ptr(), st)
        n_und = int(counts[1].item())
        kept = min(n_und, undecided_capacity)
        lo = inner(line_off, n_rows - row0 + 1, 1)
        out = dict(table=inner(table, n_rows, d).view(np.uint32).reshape(n_rows, d),
                   key_off=inner(key_off, n_rows, 1), key_len=inner(key_len, n_rows, 1),
                   key_i64=inner(key_i64, n_rows, 1), lines=lines, err_line=int(err.item()),
                   status=int(status.item()), n_undecided=n_und,
                   undecided=sorted(map(tuple, inner(und, undecided_capacity, 4)[:4 * kept]
                                        .reshape(-1, 4).tolist())),
                   line_off=lo[:parsed + 1].copy())
        if first is None:
            first = out
        else:
            _equal(first, out)
            np.testing.assert_array_equal(first['line_off'], out['line_off'])
    return first


def _equal(a, b):
    cpu._same(a, b)
    assert a['n_undecided'] == b['n_undecided'] and a['undecided'] == b['undecided']


def _check(dev, body, d, **kw):
    h = er.host_body(body, d, n_rows=kw.get('n_rows'), row0=kw.get('row0', 0),
                     undecided_capacity=kw.get('undecided_capacity', 4096))
    g = device_body(dev, body, d, **kw)
    _equal(h, g)
    starts = [0] + (np.flatnonzero(np.frombuffer(body, dtype=np.uint8) == 10) + 1).tolist()
    if starts[-1] != len(body):
        starts.append(len(body))
    np.testing.assert_array_equal(g['line_off'], starts[:len(g['line_off'])])
    return h


def _line(key: str, tokens, length=None) -> bytes:
    """'key tok tok ..' with the key padded to make the line ``length`` bytes (no line end)."""
    s = ' '.join([key] + list(tokens))
    if length is not None:
        assert length >= len(s)
        s = key + 'k' * (length - len(s)) + s[len(key):]
    return s.encode()


# ------------------------------------------------------------------------------------ files
@pytest.mark.parametrize('case', range(len(cpu.LAYOUTS)))
def test_layouts_equal_the_host_path(hip_device, case):
    _check(hip_device, cpu.LAYOUTS[case], 2)


def test_error_files_equal_the_host_path(hip_device):
    for text, _ in cpu.ERRORS:
        head, _, body = text.partition(b'\n')
        for d in (1, 2):
            _check(hip_device, body, d, shift=len(head) + 1)
    # lines behind the table's last row, rows behind an offset, a full undecided list
    _check(hip_device, b'a 1 2\nb 3 4\nc 5\n', 2, n_rows=2)
    h = _check(hip_device, b'a 1 2\nb 3 zz\n', 2, n_rows=7, row0=4)
    assert h['undecided'] == [(5, 1, 10, 2)] and not h['table'][:4].any()
    h = _check(hip_device, b'a 1e999 1e-400\nb 1e999 2\n', 2, undecided_capacity=0)
    assert h['n_undecided'] == 3
    assert device_body(hip_device, b'', 2)['lines'] == 0


def test_boundary_tokens_equal_the_host_path(hip_device):
    toks = [t for t, _ in cpu.BOUNDARY] + cpu.HOST_TOKENS + cpu.REFUSED
    body = er.file_of(range(len(toks)), [[t, '1.5'] for t in toks]).split(b'\n', 1)[1]
    h = _check(hip_device, body, 2, runs=2)
    assert h['n_undecided'] == len(cpu.HOST_TOKENS + cpu.REFUSED) and h['status'] == 0
    assert h['table'][:len(cpu.BOUNDARY), 0].tolist() == [w for _, w in cpu.BOUNDARY]


@pytest.mark.parametrize('name,fmt', cpu.FORMATS)
def test_formats_equal_the_law(hip_device, name, fmt):
    bits = cpu._finite(np.concatenate([tr.hard_bits(), tr.strided_bits(1048583)]))
    vals = bits.view(np.float32)
    vals = vals[:len(vals) // 128 * 128].reshape(-1, 128)
    rows = [[fmt(v) for v in r] for r in vals]
    body = er.file_of(range(len(rows)), rows).split(b'\n', 1)[1]
    g = device_body(hip_device, body, 128)
    want = np.asarray([[er.law(t) for t in r] for r in rows], dtype=np.uint32)
    np.testing.assert_array_equal(g['table'], want)
    assert g['n_undecided'] == 0 and g['status'] == 0


# ------------------------------------------------------------------------------------ shapes
def test_short_lines_and_one_line(hip_device):
    _check(hip_device, b'a 1\n', 1)                 # one line, shorter than a lane's bytes
    _check(hip_device, b'7 1', 1)
    _check(hip_device, b'a 1\nb 2\nc 3\nd 4\ne 5\n', 1)     # five lines in one lane's bytes
    for d in (1, 2, 63, 64, 65, 128, 512):
        toks = ['%.6f' % v for v in np.random.default_rng(d).normal(0, 0.3, size=d)]
        h = _check(hip_device, _line('12', toks) + b'\n', d)
        assert h['status'] == 0 and h['key_i64'].tolist() == [12]


def test_lines_around_one_tile(hip_device):
    """At shift 0 the first line's tile starts at its first byte."""
    toks = ['%.9g' % v for v in np.random.default_rng(0).normal(0, 0.3, size=140)]
    for length in (TILE - 1, TILE, TILE + 1, STAGED - 1, STAGED, STAGED + 1, 2 * TILE,
                   2 * TILE + 1):
        for eol in (b'\n', b'', b'\r\n'):
            h = _check(hip_device, _line('k', toks, length) + eol, 140)
            assert h['status'] == er.S_TEXT_KEY and h['n_undecided'] == 0
        _check(hip_device, _line('k', toks, length) + b'\n' + _line('9', toks) + b'\n', 140)


def test_tokens_across_the_tile_edge_and_the_staged_end(hip_device):
    """A token that starts at each of the tile's last bytes, one that ends just at, in front of
    and behind the end of the staged bytes, and long ones that are read on through memory."""
    for start in range(TILE - 12, TILE + 2):
        for tok in ('-1.2345678e-05', '1.' + '0' * 62, '1.' + '0' * (STAGED - TILE - 3),
                    '1.' + '0' * (STAGED - TILE - 2), '1.' + '0' * 200, 'x' * 90):
            line = _line('k', ['2.5'], start - 1) + b' ' + tok.encode() + b' 3.5 nan\n'
            assert line.index(tok.encode()) == start
            h = _check(hip_device, line + b'5 1 2 3 4\n', 4)
            assert h['status'] == er.S_TEXT_KEY and h['err_line'] == -1
            assert h['n_undecided'] == (len(tok) > 64)
    # keys across the edges too: a key of 3,000 digits and an 18-digit one at the tile's end
    _check(hip_device, b'1' * 3000 + b' 1 2\n' + b'7 3 4\n', 2)
    _check(hip_device, _line('k', ['1'] * 5, TILE - 9) + b' 123456789012345678 1\n', 7)


def test_more_tokens_in_a_tile_than_lanes(hip_device):
    body = (b'k' + b' 0' * 512 + b'\n') * 3 + b'k' + b' 0' * 511 + b'\n' + b'k' + b' 0' * 513
    h = _check(hip_device, body, 512)
    assert h['lines'] == 5 and h['err_line'] == 3 and not h['table'].any()
    _check(hip_device, b'k' + b'\t-0' * 512, 512)


def test_every_alignment_of_the_base(hip_device):
    toks = ['%.6f' % v for v in np.random.default_rng(3).normal(0, 0.3, size=3 * 128)]
    body = b''.join(_line(str(i), toks[128 * i:128 * (i + 1)]) + b'\n' for i in range(3))
    want = er.host_body(body, 128)
    for header in range(4, 12):                                # '<n> <d>\n' of 4 to 11 bytes
        for base in (0, 8):
            _equal(want, device_body(hip_device, body, 128, shift=base + header))


def test_3001_lines(hip_device):
    rng = np.random.default_rng(5)
    vals = rng.normal(0, 0.3, size=(3001, 24)).astype(np.float32)
    lines = []
    for i, r in enumerate(vals):
        sep = ('  ', ' ', '\t', ' \t ')[i % 4]
        lines.append((sep.join([str(i * 7919)] + tr.tokens(r)) + ('\r\n' if i % 5 == 0 else '\n'))
                     .encode())
    lines[1234] = b'1234 1 2 3\n'
    lines[2000] = b'\n'
    h = _check(hip_device, b''.join(lines), 24, runs=2)
    assert h['lines'] == 3001 and h['err_line'] == 1234 and h['status'] == er.S_BAD_TEXT
    ok = np.ones(3001, dtype=bool)
    ok[[1234, 2000]] = False
    np.testing.assert_array_equal(h['table'][ok], vals.view(np.uint32)[ok])
    np.testing.assert_array_equal(h['key_i64'][ok], (np.arange(3001) * 7919)[ok])


def test_no_read_past_the_end(hip_device):
    """The bytes behind n_bytes continue the last token with digits: the value is the short one."""
    for body in (b'a 1 2\nb 3 4', b'a 1 2\nb 3 1.5', _line('k', ['1'] * 3, TILE - 1) + b'1',
                 _line('k', ['1'] * 3, STAGED) + b'1'):
        d = 2 if body[:1] == b'a' else 3
        want = er.host_body(body, d)
        for shift in (0, 5, 11):
            for tail in (b'99999999', b'9' * 40 + b' 7 7\n'):
                _equal(want, device_body(hip_device, body, d, shift=shift, tail=tail))


# ------------------------------------------------------------------------------------ the reader
def test_device_round_trip(hip_device, tmp_path):
    bits = cpu._finite(np.concatenate([tr.hard_bits(), tr.strided_bits(11003)]))[:3001 * 128]
    table = torch.from_numpy(bits.view(np.float32).reshape(3001, 128).copy()).to(hip_device)
    keys = np.arange(3001, dtype=np.int64) * 1000003
    path = str(tmp_path / 'rt.emb')
    save_word2vec_format(path, table, keys=keys)
    for chunk in (256 << 20, 1 << 20, 1000):
        back = read_word2vec_format(path, device=hip_device, chunk_bytes=chunk)
        assert back.table.device == table.device and back.table.dtype == torch.float32
        assert torch.equal(back.table.view(torch.int32), table.view(torch.int32)), chunk
        np.testing.assert_array_equal(back.keys_i64, keys)
        assert back.host_tokens == 0
    host = read_word2vec_format(path)
    np.testing.assert_array_equal(host.table.view(np.uint32), bits.reshape(3001, 128))


def test_device_reader_equals_the_host_reader(hip_device, tmp_path):
    toks = [t for t, _ in cpu.BOUNDARY] + cpu.HOST_TOKENS
    files = [er.file_of([f'nœud{i}' if i % 2 else i for i in range(len(toks))],
                        [[t, '1.5'] for t in toks])]
    files += [f'{body.count(10) + (body[-1] != 10)} 2\n'.encode() + body for body in cpu.LAYOUTS]
    for data in files:
        path = cpu._write(tmp_path, data)
        host = read_word2vec_format(path)
        for chunk in (256 << 20, 64, 1):
            got = read_word2vec_format(path, device=hip_device, chunk_bytes=chunk)
            np.testing.assert_array_equal(got.table.cpu().numpy().view(np.uint32),
                                          host.table.view(np.uint32))
            assert got.keys() == host.keys() and got.host_tokens == host.host_tokens
            assert (got.keys_i64 is None) == (host.keys_i64 is None)
    for text, line in cpu.ERRORS:
        with pytest.raises(ValueError, match=rf'line {line}\b'):
            read_word2vec_format(cpu._write(tmp_path, text), device=hip_device, chunk_bytes=16)


def test_align_on_the_device(hip_device, tmp_path):
    from shallow_encoders.word2vec.embeddings_io import align_word2vec
    rng = np.random.default_rng(0)
    ids = np.sort(rng.choice(10 ** 6, size=500, replace=False)).astype(np.int64)
    g = cpu._edge_list_graph(ids)
    table = rng.normal(0, 0.3, size=(501, 8)).astype(np.float32)
    perm = rng.permutation(500)[:450]
    path = str(tmp_path / 'a.emb')
    save_word2vec_format(path, table, keys=ids[perm], rows=perm + 1)
    read = read_word2vec_format(path, device=hip_device)
    got = align_word2vec(read, g, missing='zero')
    assert got.device == read.table.device
    want = np.zeros_like(table)
    want[perm + 1] = table[perm + 1]
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match='50 vocabulary rows'):
        align_word2vec(read, g)


def test_downstream_tool_on_the_device_backends(hip_device, tmp_path):
    from tools import export_embeddings
    from tools import graph_model_downstream_classification as downstream
    _, argv = cpu.karate_checkpoint(str(tmp_path / 'runs'))
    argv += ['downstream.node_classification.backend=device',
             'downstream.edge_classification.backend=device']
    path = export_embeddings.main(argv)
    from_checkpoint = downstream.main(argv)
    from_file = downstream.main(argv + [f'downstream.embeddings_path={path}'])
    assert set(from_file) == {'node_accuracy', 'node_best', 'node_macro_f1', 'edge_accuracy',
                              'edge_best'}
    assert from_file == from_checkpoint
