"""Weighted text edge lists on the device (dw_edgelist_parse_weighted through
graph/edge_list.py): every weight equals ``float(token)`` bit for bit after the host's patch, the
tokens the kernel hands back are exactly those the integer restatement (tests/strtod_ref.py)
cannot decide, and the graph equals the host path's and networkx's."""
import ctypes
import functools
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgelist_ref as ref  # noqa: E402
import strtod_ref as sref  # noqa: E402

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph import edge_list as el  # noqa: E402
from shallow_encoders.graph.edge_list import read_edge_arrays, read_edge_list  # noqa: E402

pytestmark = pytest.mark.gpu

STAGE = 16384      # bytes a block stages (csrc/dw_edgelist.hip: PARSE_STAGE)
OVER = 256         # and the overrun behind them (PARSE_OVER)
N_LINES = 65537


def device_parse(data: bytes, dev, skip=0, misalign=0, und_cap=el.UNDECIDED_CAPACITY):
    """dw_edgelist_parse_weighted on its own: dict of src, dst, weight bits, the sorted undecided
    (edge, offset) pairs that fit the list, their count, lines seen, bad line or -1, status."""
    n = len(data)
    cap = (n + 1) // 4 + 1
    with torch.cuda.device(dev):
        text = None
        if n:
            buf = torch.frombuffer(bytearray(b'9' * misalign + data), dtype=torch.uint8).to(dev)
            text = buf[misalign:]
            assert text.data_ptr() % 16 == misalign
        nb = ctypes.c_size_t(0)
        _native.call('dw_edgelist_workspace_bytes', n, 0, ctypes.byref(nb))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        src = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        dst = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        wt = torch.full((cap,), -7.0, dtype=torch.float64, device=dev)
        und = torch.full((2 * und_cap + 2,), -7, dtype=torch.int64, device=dev)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_edgelist_parse_weighted', _native.ptr(text), n, skip,
                     _native.ptr(el._pow5_device(dev)), _native.ptr(src), _native.ptr(dst),
                     _native.ptr(wt), cap, _native.ptr(und), und_cap, _native.ptr(info),
                     _native.ptr(info[3:]), _native.ptr(status), _native.ptr(ws), ws.numel(),
                     _native.stream(dev))
        k, lines, n_und, bad = info.tolist()
    assert (src[k:] == -7).all() and (dst[k:] == -7).all() and (wt[k:] == -7.0).all()
    kept = min(n_und, und_cap)
    assert (und[2 * kept:] == -7).all()   # nothing written past the list's capacity
    pairs = sorted(tuple(p) for p in und[:2 * kept].view(-1, 2).tolist())
    return dict(src=src[:k].tolist(), dst=dst[:k].tolist(),
                w=wt[:k].cpu().numpy().view(np.uint64).tolist(), und=pairs, n_und=n_und,
                lines=lines, bad=bad, status=int(status.item()))


def _n_lines(data: bytes) -> int:
    return data.count(b'\n') + (0 if data.endswith(b'\n') or not data else 1)


def _expect(data: bytes, skip=0):
    """The restatement's answer for a whole text: src, dst, float() bits, the kernel's expected
    weight bits (0.0 where undecided) and the undecided (edge, offset) pairs."""
    src, dst, toks, offs = sref.parse_text_weighted(data, skip, refuse_infinite=False)
    restated = [sref.token_bits(t) for t in toks]
    assert sref.BAD not in restated
    fbits = [sref.float_bits(t) for t in toks]
    for r, f in zip(restated, fbits):
        assert r is sref.UNDECIDED or r == f
    kernel = [0 if r is sref.UNDECIDED else r for r in restated]
    und = sorted((i, o) for i, (r, o) in enumerate(zip(restated, offs)) if r is sref.UNDECIDED)
    return dict(src=src, dst=dst, fbits=fbits, w=kernel, und=und)


def _check_parse(data: bytes, dev, skip=0, misalign=0):
    want = _expect(data, skip)
    got = device_parse(data, dev, skip, misalign)
    assert got['status'] == 0 and got['bad'] == -1 and got['lines'] == _n_lines(data)
    assert (got['src'], got['dst']) == (want['src'], want['dst'])
    assert got['w'] == want['w']
    assert got['und'] == want['und'] and got['n_und'] == len(want['und'])
    assert device_parse(data, dev, skip, misalign) == got   # a rerun is bit-identical
    return want


def _write(tmp_path, data, name='edges.txt'):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _line_of(exc):
    m = re.search(r'line (\d+)', str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


def _bits(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def _finite(tok):
    return sref.float_bits(tok) & (0x7FF << 52) != 0x7FF << 52


# ---- the format file and the bad tokens -----------------------------------------------------------
def test_format_file(tmp_path, hip_device):
    data = sref.FORMAT_TEXT_WEIGHTED
    want = _check_parse(data, hip_device)
    assert len(want['src']) == 11 and len(want['und']) == 1   # 4.9e-324: a subnormal
    _check_parse(data, hip_device, skip=6)
    for empty in (b'', b'\n', b'# c'):
        _check_parse(empty, hip_device)
    path = _write(tmp_path, data)
    for chunk in (1 << 20, 64, 48):
        s, d, w = read_edge_arrays(path, device=hip_device, chunk_bytes=chunk, weighted=True)
        assert w.is_cuda and w.dtype == torch.float64
        assert (s.tolist(), d.tolist(), _bits(w)) == (want['src'], want['dst'], want['fbits'])
    hs, hd, hw = read_edge_arrays(path, weighted=True)
    assert (hs.tolist(), hd.tolist(), hw.view(np.uint64).tolist()) == (
        want['src'], want['dst'], want['fbits'])


@pytest.mark.parametrize('k', range(4))
def test_bad_lines_name_the_line(tmp_path, k, hip_device):
    for bad in sref.BAD_LINES_WEIGHTED[k::4]:
        data = b'# c\n1 2 0.5\n\n' + bad + b'\n3 4 1\n' + bad + b'\n'
        got = device_parse(data, hip_device)
        assert got['status'] == _native.DW_S_BAD_TEXT and got['bad'] == 3, bad   # 0-based
        with pytest.raises(ref.BadLine) as e0:
            sref.parse_text_weighted(data)
        assert e0.value.line_no == 4
        with pytest.raises(ValueError) as e:
            read_edge_arrays(_write(tmp_path, data), device=hip_device, weighted=True)
        assert _line_of(e) == 4, bad


# ---- the corpora ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus_text(name):
    toks = sref.corpus(name, N_LINES)[:N_LINES]
    ids = np.random.default_rng(3).integers(0, 10 ** 6, size=(len(toks), 2)).tolist()
    return b''.join(b'%d %d %s\n' % (u, v, t) for (u, v), t in zip(ids, toks))


@pytest.mark.parametrize('name', sorted(sref.CORPORA))
def test_corpus(tmp_path, name, hip_device):
    data = _corpus_text(name)
    assert _n_lines(data) == N_LINES and len(data) > 64 * STAGE // 2
    want = _check_parse(data, hip_device)
    assert len(want['src']) == N_LINES
    if name in sref.NO_UNDECIDED:
        assert not want['und']
    # through the chunk loop: float() bit for bit after the host's patch (the tokens that round
    # to infinity are refused: test_overflow_names_the_line; here they are left out)
    lines = data.split(b'\n')[:-1]
    keep = [i for i, ln in enumerate(lines) if _finite(ln.split(b' ')[2])]
    if len(keep) < len(lines):
        assert name in ('wq', 'midpoints', 'forms')
        data = b''.join(lines[i] + b'\n' for i in keep)
    s, d, w = read_edge_arrays(_write(tmp_path, data), device=hip_device, weighted=True)
    assert s.tolist() == [want['src'][i] for i in keep]
    assert _bits(w) == [want['fbits'][i] for i in keep]


# ---- boundaries -------------------------------------------------------------------------------------
def _fill_to(parts, start):
    """Comment lines so that the next line starts at byte ``start``."""
    need = start - sum(len(p) for p in parts)
    assert need >= 2
    parts.append(b'#' + b'c' * (need - 2) + b'\n')


def _straddles(start, tok, edge):
    return start < edge < start + len(tok)


def test_tokens_across_segment_stage_and_overrun_edges(hip_device):
    tok = b'12345.7890123456789012345e-3'   # 24 significant digits: w and w + 1 are compared
    parts, at = [], []                         # at: (where the token starts, which edge it crosses)
    for i in range(400):                       # lines of 37 bytes: every offset within a segment
        parts.append(b'%03d %03d ' % (i, 999 - i) + tok + b'\n')
    _fill_to(parts, STAGE - 20)
    parts.append(b'1 2  ' + tok + b'\n')                       # across the stage's edge
    at.append((STAGE - 15, STAGE))
    _fill_to(parts, 2 * STAGE - 5)                             # a line of block 1 whose token
    parts.append(b'3 4' + b' ' * (OVER - 10) + tok + b'\n')    # crosses the overrun's edge
    at.append((2 * STAGE - 5 + 3 + OVER - 10, 2 * STAGE + OVER))
    _fill_to(parts, 3 * STAGE - 8)                             # and one wholly behind the overrun
    parts.append(b'5 6' + b',' * (OVER + 40) + tok + b'\n')
    at.append((3 * STAGE - 8 + 3 + OVER + 40, None))
    parts.append(b'7 8 ' + b'0' * 40 + b'.' + b'0' * 22 + b'1' + b'\n')   # a 64-byte token
    data = b''.join(parts) + b'9 10 1.5'                       # the weight is the last byte
    for start, edge in at:
        assert data[start:start + len(tok)] == tok and data[start - 1:start] in b' ,'
        assert edge is None or _straddles(start, tok, edge)
    offs = [37 * i + 8 for i in range(400)]
    assert {(-o) % 64 for o in offs if _straddles(o, tok, o + (-o) % 64)} == set(range(1, len(tok)))
    want = _check_parse(data, hip_device)
    assert len(want['src']) == 405 and want['src'][-5:] == [1, 3, 5, 7, 9]
    for misalign in (1, 7, 8):   # the staging loads bytes then
        _check_parse(data, hip_device, misalign=misalign)
    # 65 bytes: a bad line, wherever the 65th byte falls
    long = data.replace(b'7 8 ' + b'0' * 40, b'7 8 ' + b'0' * 41)
    got = device_parse(long, hip_device, misalign=3)
    assert got['status'] == _native.DW_S_BAD_TEXT and got['bad'] == _n_lines(long) - 2


def _device_parse_ids(data: bytes, dev):
    """dw_edgelist_parse (the id-only instantiation) on its own: src, dst, lines, bad, status."""
    n = len(data)
    cap = (n + 1) // 4 + 1
    with torch.cuda.device(dev):
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        nb = ctypes.c_size_t(0)
        _native.call('dw_edgelist_workspace_bytes', n, 0, ctypes.byref(nb))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        src = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        dst = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        info = torch.zeros(3, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_edgelist_parse', _native.ptr(text), n, 0, _native.ptr(src),
                     _native.ptr(dst), cap, _native.ptr(info), _native.ptr(info[2:]),
                     _native.ptr(status), _native.ptr(ws), ws.numel(), _native.stream(dev))
        k, lines, bad = info.tolist()
    assert (src[k:] == -7).all() and (dst[k:] == -7).all()
    return src[:k].tolist(), dst[:k].tolist(), lines, bad, int(status.item())


def test_both_parsers_agree_where_the_second_id_ends_at_an_edge(hip_device):
    """The two grammars are one function (parse_line<WEIGHTED>), so a slip in the prefix they
    share would move both parsers together: one "u v w" text, just past a stage and its overrun,
    goes through dw_edgelist_parse (the weight is an extra column) and dw_edgelist_parse_weighted;
    both equal each other and parse_lines_host where the second id — the last field they share —
    ends at a segment's edge and at the stage's edge, and for a line that starts in the overrun."""
    rng = np.random.default_rng(17)
    forms = [b'1e3', b'-0', b'.5', b'5.', b'+2.5E-3']
    parts, toks = [b'# u v w\n', b'\n', b' \t\n', b'% a comment\n', b'\r\n'], []

    def add(u, v, tok, end=b'\n'):
        parts.append(b'%d %d %s' % (u, v, tok) + end)
        toks.append(tok)

    def lines_until(limit):   # random lines, then one comment line up to ``limit`` exactly
        i = 0
        while sum(len(p) for p in parts) + 100 < limit:
            u, v = rng.integers(0, 10 ** 6, size=2).tolist()
            tok = forms[i // 9 % len(forms)] if i % 9 == 4 else repr(rng.random() + 0.5).encode()
            add(u, v, tok, b'\r\n' if i % 5 == 2 else b'\n')
            if i % 11 == 7:
                parts.append(b'\n' if i % 2 else b'  # between\n')
            i += 1
        _fill_to(parts, limit)

    seg_edge = 64 * 97
    lines_until(seg_edge - 7)
    add(11, 2222, b'0.5')                    # '11 2222': the separator behind it is at the edge
    lines_until(STAGE - 7)
    add(33, 4444, b'1.25', b'\r\n')
    in_overrun = sum(len(p) for p in parts)  # the next line starts behind the stage's edge
    add(55, 66, b'7.75')
    lines_until(STAGE + OVER + 300)
    add(77, 88, b'0.1')
    data = b''.join(parts)
    assert STAGE + OVER < len(data) < STAGE + OVER + 1024
    for edge in (seg_edge, STAGE):
        assert data[edge - 4:edge + 1] in (b'2222 ', b'4444 ')
    assert STAGE < in_overrun < STAGE + OVER and data[in_overrun - 1:in_overrun + 5] == b'\n55 66'
    hs, hd, h_lines = el.parse_lines_host(data)
    ws, wd, ww, w_lines = el.parse_lines_host(data, weighted=True)
    assert len(hs) == len(toks) > 500 and h_lines == w_lines == _n_lines(data)
    assert (ws.tolist(), wd.tolist()) == (hs.tolist(), hd.tolist())
    assert ww.view(np.uint64).tolist() == [sref.float_bits(t) for t in toks]
    assert all(sref.token_bits(t) == sref.float_bits(t) for t in toks)   # none is undecided
    ids = _device_parse_ids(data, hip_device)
    assert ids == (hs.tolist(), hd.tolist(), h_lines, -1, 0)
    got = device_parse(data, hip_device)
    assert got['status'] == 0 and got['bad'] == -1
    assert (got['src'], got['dst'], got['lines']) == ids[:3]
    assert got['w'] == [sref.float_bits(t) for t in toks]   # float(token), bit for bit
    assert got['n_und'] == 0 and got['und'] == []


# ---- chunks -----------------------------------------------------------------------------------------
def _undecided_lines(n, seed):
    """n lines; every seventh weight is one the kernel hands back (subnormal / 25 digits that the
    first 19 do not settle / an exact midpoint above 2^64)."""
    rng = np.random.default_rng(seed)
    hard = [b'4.9e-324', b'1e-310', b'-2.5e-320', str((2 * (1 << 52) + 1) << 70).encode()]
    hard += [t for t in sref.corpus('digits25', 40000) if sref.token_bits(t) is sref.UNDECIDED][:6]
    assert len(hard) >= 8 and all(sref.token_bits(t) is sref.UNDECIDED for t in hard)
    out = []
    for i, (u, v) in enumerate(rng.integers(0, 10 ** 6, size=(n, 2)).tolist()):
        t = hard[(i // 7) % len(hard)] if i % 7 == 3 else repr(rng.random() + 0.5).encode()
        out.append(b'%d %d %s\n' % (u, v, t))
    return out


def test_chunks_and_global_line_numbers(tmp_path, hip_device):
    lines = _undecided_lines(400, seed=4)
    data = b'# header\n' + b''.join(lines)
    assert len(data) > 3 * 4096
    want = _expect(data)
    assert len(want['und']) >= 50
    path = _write(tmp_path, data)
    one = read_edge_arrays(path, device=hip_device, weighted=True)
    many = read_edge_arrays(path, device=hip_device, weighted=True, chunk_bytes=4096)
    for s, d, w in (one, many):
        assert (s.tolist(), d.tolist(), _bits(w)) == (want['src'], want['dst'], want['fbits'])
    hs, hd, hw = read_edge_arrays(path, weighted=True, chunk_bytes=4096)
    assert hw.view(np.uint64).tolist() == want['fbits']
    # a bad weight, an infinite one, each in a late chunk: the line number stays global
    for tok in (b'1.5x', b'nan', b'1e999', b'-1e999'):
        bad = lines[:350] + [b'1 2 ' + tok + b'\n'] + lines[350:]
        path = _write(tmp_path, b'# header\n' + b''.join(bad), 'bad.txt')
        assert sum(len(x) for x in bad[:350]) > 2 * 4096
        for device in (hip_device, None):
            with pytest.raises(ValueError) as e:
                read_edge_arrays(path, device=device, weighted=True, chunk_bytes=4096)
            assert _line_of(e) == 352, tok
        with pytest.raises(ValueError) as e:
            read_edge_arrays(path, device=hip_device, weighted=True)
        assert _line_of(e) == 352, tok
    # an infinite weight ahead of a bad line in the same chunk: the first offence is named
    both = lines[:10] + [b'1 2 1e999\n'] + lines[10:20] + [b'1 2 x\n']
    path = _write(tmp_path, b''.join(both), 'both.txt')
    for device in (hip_device, None):
        with pytest.raises(ValueError) as e:
            read_edge_arrays(path, device=device, weighted=True)
        assert _line_of(e) == 11


def test_skip_rows(tmp_path, hip_device):
    path = _write(tmp_path, b'source,target,weight\n1,2,0.5\n2,3,x\n', 'edges.csv')
    with pytest.raises(ValueError) as e:
        read_edge_list(path, device=hip_device, weighted=True)
    assert _line_of(e) == 1
    with pytest.raises(ValueError) as e:
        read_edge_list(path, device=hip_device, weighted=True, skip_rows=1)
    assert _line_of(e) == 3
    path = _write(tmp_path, b'source,target,weight\n1,2,0.5\n2,3,7\n', 'good.csv')
    g = read_edge_list(path, device=hip_device, weighted=True, skip_rows=1)
    ref.assert_same_graph(g, ref.networkx_csr([1, 2], [2, 3], [0.5, 7.0]))


# ---- more undecided tokens than the list holds -------------------------------------------------------
def test_hand_over_overflow_takes_the_host_route(tmp_path, hip_device):
    data = b''.join(_undecided_lines(200, seed=6))
    want = _expect(data)
    assert len(want['und']) > 4
    got = device_parse(data, hip_device, und_cap=4)
    assert got['n_und'] == len(want['und']) and len(got['und']) == 4   # counted, not stored
    assert set(got['und']) <= set(want['und']) and got['w'] == want['w']
    path = _write(tmp_path, data)
    for chunk in (1 << 20, 2048):
        s, d, w = read_edge_arrays(path, device=hip_device, weighted=True, chunk_bytes=chunk,
                                   undecided_capacity=4)
        assert (s.tolist(), d.tolist(), _bits(w)) == (want['src'], want['dst'], want['fbits'])


# ---- graphs -------------------------------------------------------------------------------------------
def _weighted_text(src, dst, w):
    return ''.join(f'{u} {v} {x!r}\n' for u, v, x in zip(src.tolist(), dst.tolist(),
                                                          w.tolist())).encode()


@pytest.mark.parametrize('case', ['sparse_weighted', 'single_loop'])
def test_weighted_graph(tmp_path, case, hip_device):
    src, dst, w = ref.ARRAY_CASES[case]()
    path = _write(tmp_path, _weighted_text(src, dst, w))
    dev = read_edge_list(path, device=hip_device, weighted=True)
    assert dev.col is None and dev.weighted   # built and kept in HBM
    ref.assert_same_graph(dev, read_edge_list(path, weighted=True))
    ref.assert_same_graph(dev, ref.networkx_csr(src, dst, w))
    assert dev.device_tensors(hip_device)['weights'].dtype == torch.float64
    ref.assert_same_graph(read_edge_list(path, device=hip_device), ref.networkx_csr(src, dst))
    if case == 'sparse_weighted':   # last occurrence wins, on both directions
        g = dev
        u, v = int(src[10]), int(dst[10])   # repeated, reversed, at 50
        iu = 1 + int(np.searchsorted(g.itos.ids, u))
        iv = 1 + int(np.searchsorted(g.itos.ids, v))
        rp, col, wt = np.asarray(g.row_ptr), g.host_col(), g.weights
        last = max(i for i in range(60) if {int(src[i]), int(dst[i])} == {u, v})
        assert last >= 50
        for a, b in ((iu, iv), (iv, iu)):
            k = rp[a] + int(np.flatnonzero(col[rp[a]:rp[a + 1]] == b)[0])
            assert wt[k] == w[last]


# ---- end to end ---------------------------------------------------------------------------------------
def test_dataset_config_walks_and_negative_weight(tmp_path, hip_device):
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.graph.random_walk_generator import DeepWalk
    rng = np.random.default_rng(12)
    e = [(i, (i + 1) % 20) for i in range(20)] + [(int(a), int(b)) for a, b in
                                                  rng.integers(0, 20, size=(20, 2))]
    w = rng.random(40) + 0.5
    text = ''.join(f'{u} {v} {x!r}\n' for (u, v), x in zip(e, w.tolist())).encode()
    assert text.count(b'\n') == 40
    path = _write(tmp_path, text)

    def dataset(p, *more):
        random.seed(0)
        c = load_config('sge_sg_edge_list', overrides=[
            f'datamodule.additional_parameters.path={p}',
            'datamodule.additional_parameters.walks_per_node=4',
            'datamodule.additional_parameters.walk_length=8', *more])
        return c.datamodule.instantiate_dataset().dataset

    ds = dataset(path, 'datamodule.additional_parameters.weighted=true')
    g = ds.csr
    assert g.weighted and g.col is None
    ref.assert_same_graph(g, ref.networkx_csr([a for a, _ in e], [b for _, b in e], w))
    walks = ds.next_walk_batch(64)
    assert walks.shape == (64, 8)
    rp, col = np.asarray(g.row_ptr), g.host_col()
    for walk in walks.tolist():
        for a, b in zip(walk, walk[1:]):
            assert b in col[rp[a]:rp[a + 1]]
    assert not dataset(path).csr.weighted   # the flag off: the same file, unweighted
    # one negative weight: refused where the walker's alias table is built, as for arrays
    neg = b'0 1 -0.001\n' + text.split(b'\n', 1)[1]
    assert text.startswith(b'0 1 ') and neg.count(b'-') == 1
    with pytest.raises(ValueError, match='negative weight'):
        bad = read_edge_list(_write(tmp_path, neg, 'neg.txt'), device=hip_device, weighted=True)
        DeepWalk(bad, 8, rng='philox', device=hip_device).walk_batch(
            torch.arange(1, 5, dtype=torch.int32), walk_id0=0)
