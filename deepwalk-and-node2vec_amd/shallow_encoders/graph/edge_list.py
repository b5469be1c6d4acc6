"""A user's edge list — a text / CSV file, ``.npy`` / ``.npz`` arrays, or two id arrays — straight
to the CSR the walkers use, on the host (numpy) or in HBM (csrc/dw_edgelist.hip).

The result equals, array for array, ``CSRGraph.from_networkx`` of the graph networkx would build
from the same edges (tests/edgelist_ref.py runs exactly that):

  * nodes: the distinct endpoint ids, ascending; node i is named ``n`` + its id zero-padded to
    ``max(7, digits of the largest id)``, so the vocabulary's lexicographic order is the numeric
    one and vocabulary id = 1 + rank (row 0 is ``<unk>``); no node is isolated;
  * edges: an undirected pair {u, v} is kept once, at the position and in the orientation of its
    first occurrence (either orientation counts as an occurrence); its weight is that of its
    LAST occurrence (networkx updates the edge's attribute dict); a self-loop is kept, once;
  * rows: kept edge i contributes u->v at 2i and v->u at 2i+1 (a self-loop: one entry), stably
    sorted by source — each row lists its neighbours in order of first occurrence; both
    directions carry the edge's weight.

Limits: ids in [0, 10^18), fewer than 2^31 raw edges, 2^31 - 1 nodes and 2^31 directed entries.
An input without a single edge (an empty file, comments only) is a ``ValueError``: a graph with
no nodes has no vocabulary and nothing to walk.

Text format (``read_edge_list``): one edge per line; lines end in ``\\n`` (a ``\\r`` closing the
line is dropped; the last line may lack its ``\\n``); lines of blanks (space, tab) only and lines
whose first non-blank byte is ``#`` or ``%`` are skipped; a data line is optional blanks, an
unsigned decimal of 1-18 digits (leading zeros allowed), one or more separators from {space, tab,
comma}, a second such number, then the end of the line or a separator followed by anything
(extra columns are ignored, as ``nx.read_edgelist(data=False)`` does). Every other line — a sign,
a 19th digit, a missing second field, a non-digit where a number starts or right behind one — is
a ``ValueError`` naming its 1-based line number.

Weighted text (``weighted=True``; off by default, and then a third column is an extra column like
any other): a data line is the two ids as above, one or more separators, and a weight token,
then the end of the line or a separator followed by anything. The token is an optional ``+`` or
``-``; then digits with an optional ``.`` and more digits, or a ``.`` followed by at least one
digit (``5``, ``5.``, ``5.25``, ``.25``); then an optional exponent: ``e`` or ``E``, an optional
sign, one to four digits. Leading and trailing zeros are allowed, a token is at most 64 bytes,
and ``-0`` gives -0.0. Everything else is a bad line naming its 1-based line number: no third
field, ``nan`` / ``inf`` / ``infinity`` in any case, hex, ``_``, ``1e``, ``.``, ``e5``,
``1.2.3``, ``--1``, ``1.5x``. The weight is ``float(token)`` bit for bit — what networkx stores
— on both paths: the host calls ``float``; the device converts in integer arithmetic
(Eisel-Lemire; csrc/dw_strtod.h) and hands the few tokens it cannot decide (more than 19
significant digits that the first 19 do not settle, subnormal, underflowing or overflowing
values) back to the host's ``float`` chunk by chunk. A token whose value rounds to +-inf
(``1e999``) is a ``ValueError`` naming its line; underflow to a subnormal or to zero is legal.

Node labels (``read_node_labels``) come in a file of their own, one line per node under the same
line rules: optional blanks, the node's id (1-18 digits), one or more separators, the label token
(a run of bytes other than the separators and line ends), then the end of the line or a separator
followed by anything. An id that appears twice is a ``ValueError`` naming its second line.

Multi-label files (``read_node_label_sets``, e.g. BlogCatalog's ``group-edges.csv``) follow the
same line rules, except that every token after the id is a label (``node l1 [l2 ...]``) and a node
may appear on several lines: its labels are unioned.
"""
import os
import re
from typing import List, Optional, Tuple

import numpy as np
import torch

from shallow_encoders.graph.csr import CSRGraph, IdNames, id_name_width

ID_LIMIT = 10 ** 18
_LIMIT_31 = 1 << 31
DEFAULT_CHUNK_BYTES = 256 << 20


# ---- arrays -> CSR -------------------------------------------------------------------------------
def _is_device(device) -> bool:
    return device is not None and torch.device(device).type == 'cuda'


def _check_ids(lo: int, hi: int) -> None:
    if lo < 0 or hi >= ID_LIMIT:
        raise ValueError(f'edge-list node ids must lie in [0, 10^18); got {lo if lo < 0 else hi}')


def _host_ids(x, what: str) -> np.ndarray:
    a = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in 'iu':
        raise TypeError(f'{what} must be a 1-d integer array')
    if a.size:
        _check_ids(int(a.min()), int(a.max()))
    return np.ascontiguousarray(a, dtype=np.int64)


def _check_sizes(m: int, m_dst: int, weights) -> None:
    if m != m_dst:
        raise ValueError(f'src and dst differ in length ({m} != {m_dst})')
    if weights is not None and len(weights) != m:
        raise ValueError(f'weights has {len(weights)} entries for {m} edges')
    if m == 0:
        raise ValueError('the edge list holds no edges: a graph without nodes has no vocabulary '
                         'and cannot be walked')
    if m >= _LIMIT_31:
        raise ValueError(f'{m} raw edges: the edge-list build takes fewer than 2^31')


def _check_graph(n: int, nnz_bound: int) -> None:
    if n >= _LIMIT_31 - 1:
        raise ValueError(f'{n} nodes: vocabulary ids are int32 (fewer than 2^31 - 1 nodes)')
    if nnz_bound >= _LIMIT_31:
        raise ValueError(f'{nnz_bound} directed entries: the CSR build takes fewer than 2^31')


def edge_list_csr(src, dst, weights=None, device=None) -> CSRGraph:
    """The CSR of the undirected graph with edges (src[i], dst[i]) — raw int64 ids in [0, 10^18),
    optional float64 ``weights`` — built with numpy (``device=None``) or in HBM (identical
    arrays; module docstring for the contract)."""
    if _is_device(device):
        return _edge_list_csr_device(src, dst, weights, device)
    src, dst = _host_ids(src, 'src'), _host_ids(dst, 'dst')
    if weights is not None:
        weights = weights.cpu().numpy() if isinstance(weights, torch.Tensor) else weights
        weights = np.ascontiguousarray(weights, dtype=np.float64)
    _check_sizes(len(src), len(dst), weights)
    # nodes: rank = index among the sorted distinct ids
    ids, inv = np.unique(np.stack([src, dst], axis=1).ravel(), return_inverse=True)
    inv = inv.reshape(-1)
    n = len(ids)
    ru, rv = inv[0::2], inv[1::2]
    # edges: runs of equal (min, max) in raw order; head = first occurrence, tail = last
    key = np.minimum(ru, rv) * np.int64(max(n, 1)) + np.maximum(ru, rv)
    _check_graph(n, 0)
    order = np.argsort(key, kind='stable')
    ks = key[order]
    change = ks[1:] != ks[:-1]
    first = order[np.concatenate([[True], change])]
    last = order[np.concatenate([change, [True]])]
    sel = np.argsort(first)
    first, last = first[sel], last[sel]
    eu, ev = ru[first], rv[first]
    ew = None if weights is None else weights[last]
    # rows: u->v at 2i, v->u at 2i+1 (not for a self-loop), stable by source
    E = len(eu)
    _check_graph(n, 2 * E)
    s2 = np.empty(2 * E, dtype=np.int64)
    d2 = np.empty(2 * E, dtype=np.int64)
    s2[0::2], d2[0::2] = eu, ev
    s2[1::2], d2[1::2] = ev, eu
    live = np.ones(2 * E, dtype=bool)
    live[1::2] = eu != ev
    entry = np.flatnonzero(live)
    entry = entry[np.argsort(s2[entry], kind='stable')]
    col = (d2[entry] + 1).astype(np.int32)
    row_ptr = np.zeros(n + 2, dtype=np.int64)
    np.cumsum(np.bincount(s2[entry], minlength=n), out=row_ptr[2:])
    w = None if ew is None else ew[entry >> 1]
    return CSRGraph.from_arrays(row_ptr, col, w, itos=IdNames(ids, id_name_width(int(ids[-1]))))


def _device_ids(x, dev, what: str) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        if x.dim() != 1 or x.dtype not in (torch.int64, torch.int32):
            raise TypeError(f'{what} must be a 1-d integer tensor')
        return x.to(device=dev, dtype=torch.int64).contiguous()
    return torch.from_numpy(_host_ids(x, what)).to(dev)


def _edge_list_csr_device(src, dst, weights, device) -> CSRGraph:
    """edge_list_csr in HBM: dw_edges_canonical + dw_csr_from_edges_loops."""
    import ctypes

    from shallow_encoders import _native
    dev = _native.require_device(device)
    with torch.cuda.device(dev):
        src, dst = _device_ids(src, dev, 'src'), _device_ids(dst, dev, 'dst')
        if weights is not None:
            weights = torch.as_tensor(weights, dtype=torch.float64).to(dev).contiguous()
        m = src.numel()
        _check_sizes(m, dst.numel(), weights)
        lo = int(torch.minimum(src.min(), dst.min()))
        hi = int(torch.maximum(src.max(), dst.max()))
        _check_ids(lo, hi)
        id_bits = max(1, hi.bit_length())   # the endpoint sort reads only the bits in use
        s = _native.stream(dev)
        nbytes = ctypes.c_size_t(0)
        _native.call('dw_edgelist_workspace_bytes', 0, m, ctypes.byref(nbytes))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        node_ids = torch.empty(2 * m, dtype=torch.int64, device=dev)
        edges = torch.empty(m, dtype=torch.int64, device=dev)
        ew = None if weights is None else torch.empty(m, dtype=torch.float64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_edges_canonical', _native.ptr(src), _native.ptr(dst),
                     _native.ptr(weights), m, id_bits, _native.ptr(node_ids), _native.ptr(edges),
                     _native.ptr(ew), _native.ptr(counts), _native.ptr(status), _native.ptr(ws),
                     ws.numel(), s)
        n, E = (int(x) for x in counts.tolist())   # synchronises
        _native.check_status(status, 'edge-list canonical form')
        _check_graph(n, 2 * E)
        ids = node_ids[:n].cpu().numpy()
        del node_ids, src, dst, weights
        row_ptr = torch.empty(n + 2, dtype=torch.int64, device=dev)
        col = torch.empty(2 * E, dtype=torch.int32, device=dev)
        w = None if ew is None else torch.empty(2 * E, dtype=torch.float64, device=dev)
        _native.call('dw_csr_from_edges_loops', _native.ptr(edges), _native.ptr(ew), E, n,
                     _native.ptr(row_ptr), _native.ptr(col), _native.ptr(w), _native.ptr(status),
                     _native.ptr(ws), ws.numel(), s)
        _native.check_status(status, 'edge-list CSR build')
        nnz = int(row_ptr[n + 1])
        del ws, edges, ew
    return CSRGraph.from_device(row_ptr, col[:nnz], IdNames(ids, id_name_width(int(ids[-1]))),
                                None if w is None else w[:nnz])


# ---- text -> arrays ------------------------------------------------------------------------------
_DATA_LINE = re.compile(rb'([0-9]{1,18})[ \t,]+([0-9]{1,18})(?:[ \t,]|\Z)')


_WEIGHT_TOKEN = rb'[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]{1,4})?'
_WEIGHTED_LINE = re.compile(rb'([0-9]{1,18})[ \t,]+([0-9]{1,18})[ \t,]+(' + _WEIGHT_TOKEN
                            + rb')(?:[ \t,]|\Z)')
_TOKEN_AT = re.compile(rb'[^ \t,\r\n]*')
MAX_WEIGHT_TOKEN = 64
UNDECIDED_CAPACITY = 65536   # (edge, offset) entries a chunk may hand back before the host twin


def _finite_weight(token: bytes, where: str, line_no: int) -> float:
    w = float(token)
    if w - w != 0.0:
        raise ValueError(f'{where}: line {line_no}: the weight {token.decode()} is not finite')
    return w


def parse_lines_host(buf: bytes, skip_lines: int = 0, first_line: int = 1,
                     where: str = 'edge list', weighted: bool = False):
    """(src, dst, lines seen) — ``weighted``: (src, dst, weights, lines seen) — of a piece of
    text that starts at a line start; ``first_line``: the 1-based number of its first line (for
    the error message). The host twin of dw_edgelist_parse / dw_edgelist_parse_weighted."""
    lines = buf.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    src: List[int] = []
    dst: List[int] = []
    wts: List[float] = []
    pattern = _WEIGHTED_LINE if weighted else _DATA_LINE
    for k, line in enumerate(lines):
        if k < skip_lines:
            continue
        if line.endswith(b'\r'):
            line = line[:-1]
        t = line.lstrip(b' \t')
        if not t or t[:1] in (b'#', b'%'):
            continue
        m = pattern.match(t)
        if m is None or (weighted and len(m.group(3)) > MAX_WEIGHT_TOKEN):
            raise ValueError(f'{where}: line {first_line + k} is not '
                             f'{"a weighted edge" if weighted else "an edge"}: '
                             f'{line[:60].decode(errors="replace")!r}')
        src.append(int(m.group(1)))
        dst.append(int(m.group(2)))
        if weighted:
            wts.append(_finite_weight(m.group(3), where, first_line + k))
    s, d = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if weighted:
        return s, d, np.asarray(wts, dtype=np.float64), len(lines)
    return s, d, len(lines)


_POW5 = {}   # device index -> the powers of five of dw_edgelist_parse_weighted, in HBM


def _pow5_device(dev) -> torch.Tensor:
    from shallow_encoders import _native
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _POW5:
        table = np.empty(2 * 651, dtype=np.uint64)
        _native.call('dw_pow5_table', table.ctypes.data)
        _POW5[key] = torch.from_numpy(table.view(np.int64)).to(dev)
    return _POW5[key]


def _patch_undecided(und: np.ndarray, stage: np.ndarray, n: int, wbuf: torch.Tensor, where: str,
                     lines_seen: int) -> Optional[Tuple[int, str]]:
    """Converts the chunk's undecided tokens (rows (edge, offset) of ``und``; ``stage[:n]`` still
    holds the text) with ``float`` and writes them into ``wbuf``. Returns (1-based line, message)
    of the first one that is not finite, else None."""
    und = und[np.argsort(und[:, 0], kind='stable')]
    vals = np.empty(len(und), dtype=np.float64)
    for i, off in enumerate(und[:, 1].tolist()):
        token = _TOKEN_AT.match(stage[off:min(n, off + MAX_WEIGHT_TOKEN)].tobytes()).group(0)
        v = float(token)
        vals[i] = v
        if v - v != 0.0:
            line = lines_seen + int(np.count_nonzero(stage[:off] == 10)) + 1
            return line, f'{where}: line {line}: the weight {token.decode()} is not finite'
    wbuf[torch.from_numpy(und[:, 0].copy()).to(wbuf.device)] = torch.from_numpy(vals).to(
        wbuf.device)
    return None


def _last_newline(view: np.ndarray, n: int) -> int:
    """Index of the last '\\n' in view[:n], or -1 (searched backwards in windows)."""
    hi = n
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        k = view[lo:hi].tobytes().rfind(b'\n')
        if k >= 0:
            return lo + k
        hi = lo
    return -1


def _text_chunks(path: str, stage: np.ndarray):
    """Yields n: stage[:n] holds the next whole lines of the file. The host cuts each chunk at
    its last '\\n' and carries the rest over, so the staging buffer (len(stage) bytes) bounds the
    memory whatever the file's size; a line that does not fit is an error."""
    size = len(stage)
    carry = 0
    with open(path, 'rb', buffering=0) as f:
        while True:
            got = carry
            while got < size:   # (a raw read may return less than asked)
                k = f.readinto(memoryview(stage)[got:size])
                if not k:
                    break
                got += k
            if got < size:   # end of file: everything left, with or without a final '\n'
                if got:
                    yield got
                return
            cut = _last_newline(stage, got)
            if cut < 0:
                raise ValueError(f'{path}: a line is longer than chunk_bytes={size}')
            yield cut + 1
            carry = got - (cut + 1)
            stage[:carry] = stage[cut + 1:got].copy()


def read_edge_arrays(path: str, device=None, skip_rows: int = 0,
                     chunk_bytes: int = DEFAULT_CHUNK_BYTES, weighted: bool = False,
                     undecided_capacity: int = UNDECIDED_CAPACITY):
    """(src, dst) — ``weighted``: (src, dst, weights float64) — of a text edge list, in file
    order: numpy arrays (``device=None``, parsed on the host) or device tensors (parsed in HBM by
    dw_edgelist_parse / dw_edgelist_parse_weighted, chunk by chunk). ``undecided_capacity``: the
    weight tokens a chunk may hand back to the host one by one; past it the host parses the whole
    chunk's weights (the same values, slowly)."""
    if chunk_bytes < 1 or skip_rows < 0 or undecided_capacity < 0:
        raise ValueError('chunk_bytes must be positive, skip_rows and undecided_capacity '
                         'non-negative')
    # one spare byte: a file of exactly chunk_bytes is then seen to end, not cut
    size = int(min(chunk_bytes, os.path.getsize(path) + 1))
    on_device = _is_device(device)
    if on_device:
        import ctypes

        from shallow_encoders import _native
        dev = _native.require_device(device)
        stage_t = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        stage = stage_t.numpy()
        cap = (size + 1) // 4 + 1
        nbytes = ctypes.c_size_t(0)
        _native.call('dw_edgelist_workspace_bytes', size, 0, ctypes.byref(nbytes))
        with torch.cuda.device(dev):
            text = torch.empty(size, dtype=torch.uint8, device=dev)
            ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
            sbuf = torch.empty(cap, dtype=torch.int64, device=dev)
            dbuf = torch.empty(cap, dtype=torch.int64, device=dev)
            # edges, lines, [undecided tokens,] bad line
            info = torch.zeros(4 if weighted else 3, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            if weighted:
                wbuf = torch.empty(cap, dtype=torch.float64, device=dev)
                ubuf = torch.empty(2 * max(undecided_capacity, 1), dtype=torch.int64, device=dev)
                pow5 = _pow5_device(dev)
    else:
        stage = np.empty(size, dtype=np.uint8)
    srcs, dsts, wtss, lines_seen = [], [], [], 0
    for n in _text_chunks(path, stage):
        skip = max(0, skip_rows - lines_seen)
        if on_device:
            with torch.cuda.device(dev):
                text[:n].copy_(stage_t[:n], non_blocking=True)
                tail = (_native.ptr(info), _native.ptr(info[-1:]), _native.ptr(status),
                        _native.ptr(ws), ws.numel(), _native.stream(dev))
                if weighted:
                    _native.call('dw_edgelist_parse_weighted', _native.ptr(text), n, skip,
                                 _native.ptr(pow5), _native.ptr(sbuf), _native.ptr(dbuf),
                                 _native.ptr(wbuf), cap, _native.ptr(ubuf), undecided_capacity,
                                 *tail)
                else:
                    _native.call('dw_edgelist_parse', _native.ptr(text), n, skip,
                                 _native.ptr(sbuf), _native.ptr(dbuf), cap, *tail)
                counts = [int(x) for x in info.tolist()]   # synchronises: stage is free
                k, n_lines, bad = counts[0], counts[1], counts[-1]
                # the first offence of the chunk, in file order: a bad line or (weighted) an
                # infinite weight
                first = None
                if int(status.item()) & _native.DW_S_BAD_TEXT:
                    what = 'a weighted edge' if weighted else 'an edge'
                    first = (lines_seen + bad + 1,
                             f'{path}: line {lines_seen + bad + 1} is not {what}')
                if weighted:
                    n_und = counts[2]
                    w_chunk = wbuf[:k]
                    if n_und > undecided_capacity:   # the host twin raises for either offence
                        w_host = parse_lines_host(stage[:n].tobytes(), skip, lines_seen + 1, path,
                                                  weighted=True)[2]
                        w_chunk = torch.from_numpy(w_host).to(dev)
                    elif n_und:
                        inf = _patch_undecided(ubuf[:2 * n_und].cpu().numpy().reshape(-1, 2),
                                               stage, n, wbuf, path, lines_seen)
                        if inf is not None and (first is None or inf[0] < first[0]):
                            first = inf
                if first is not None:
                    raise ValueError(first[1])
                _native.check_status(status, 'edge-list parse')
                srcs.append(sbuf[:k].clone())
                dsts.append(dbuf[:k].clone())
                if weighted:
                    wtss.append(w_chunk.clone())
        else:
            *arrays, n_lines = parse_lines_host(stage[:n].tobytes(), skip, lines_seen + 1, path,
                                                weighted=weighted)
            for acc, x in zip((srcs, dsts, wtss), arrays):
                acc.append(x)
        lines_seen += n_lines
    if on_device:
        if not srcs:
            z = torch.empty(0, dtype=torch.int64, device=dev)
            out = (z, z.clone(), torch.empty(0, dtype=torch.float64, device=dev))
        else:
            out = (torch.cat(srcs), torch.cat(dsts), torch.cat(wtss) if weighted else None)
    elif not srcs:
        out = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64),
               np.empty(0, dtype=np.float64))
    else:
        out = (np.concatenate(srcs), np.concatenate(dsts),
               np.concatenate(wtss) if weighted else None)
    return out if weighted else out[:2]


def read_edge_list(path: str, device=None, skip_rows: int = 0,
                   chunk_bytes: int = DEFAULT_CHUNK_BYTES, weighted: bool = False) -> CSRGraph:
    """The CSR of an edge-list file: ``.npz`` (``src``, ``dst``, optional ``weight``), ``.npy``
    (int ``[m, 2]``), anything else as text (module docstring), read in chunks of ``chunk_bytes``.
    ``device``: build in HBM (text parsed there too) instead of with numpy — the same arrays.
    ``weighted``: a text file's third column is the edge's weight (``.npz`` carries its own
    ``weight`` whatever the flag says; ``.npy`` has no room for one)."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    weights = None
    if ext == '.npz':
        with np.load(path, allow_pickle=False) as f:
            src, dst = f['src'], f['dst']
            weights = f['weight'] if 'weight' in f.files else None
    elif ext == '.npy':
        if weighted:
            raise ValueError(f'{path}: an .npy edge list is an integer [m, 2] array and holds '
                             f'no weights; use .npz with a weight array, or text')
        a = np.load(path, allow_pickle=False)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f'{path}: expected an integer array of shape [m, 2], got '
                             f'{a.shape}')
        src, dst = a[:, 0], a[:, 1]
    elif weighted:
        src, dst, weights = read_edge_arrays(path, device, skip_rows, chunk_bytes, weighted=True)
    else:
        src, dst = read_edge_arrays(path, device, skip_rows, chunk_bytes)
    if len(src) == 0:
        raise ValueError(f'{path}: no edges (a graph without nodes has no vocabulary and '
                         f'cannot be walked)')
    return edge_list_csr(src, dst, weights, device)


# ---- node labels ---------------------------------------------------------------------------------
_LABEL_LINE = re.compile(rb'([0-9]{1,18})[ \t,]+([^ \t,\r\n]+)(?:[ \t,]|\Z)')


def _label_lines(path: str, skip_rows: int):
    """(index, line without its line end, the line without leading blanks) of a label file's
    lines that hold data: not skipped, not blank, no comment."""
    with open(path, 'rb') as f:
        lines = f.read().split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    for k, line in enumerate(lines):
        if k < skip_rows:
            continue
        if line.endswith(b'\r'):
            line = line[:-1]
        t = line.lstrip(b' \t')
        if not t or t[:1] in (b'#', b'%'):
            continue
        yield k, line, t


def read_node_labels(path: str, skip_rows: int = 0) -> Tuple[np.ndarray, List[str]]:
    """(ids int64[m], tokens list[str]) of a node-label file, in file order: ``.npz`` (integer
    arrays ``node`` and ``label``; the labels' decimal strings are the tokens), anything else as
    text (module docstring). Parsed on the host: the file has one line per node, not per edge."""
    path = os.fspath(path)
    if skip_rows < 0:
        raise ValueError('skip_rows must be non-negative')
    if os.path.splitext(path)[1].lower() == '.npz':
        with np.load(path, allow_pickle=False) as f:
            node, label = np.asarray(f['node']), np.asarray(f['label'])
        if node.ndim != 1 or node.shape != label.shape or node.dtype.kind not in 'iu' \
                or label.dtype.kind not in 'iu':
            raise ValueError(f'{path}: node and label must be 1-d integer arrays of one length')
        ids = _host_ids(node, 'node')
        uniq, first = np.unique(ids, return_index=True)
        if len(uniq) != len(ids):
            second = int(np.setdiff1d(np.arange(len(ids)), first)[0])
            raise ValueError(f'{path}: node {int(ids[second])} is labelled twice (entry '
                             f'{second + 1})')
        return ids, [str(int(v)) for v in label]
    ids: List[int] = []
    tokens: List[str] = []
    seen = set()
    for k, line, t in _label_lines(path, skip_rows):
        m = _LABEL_LINE.match(t)
        if m is None:
            raise ValueError(f'{path}: line {k + 1} is not a node label: '
                             f'{line[:60].decode(errors="replace")!r}')
        node = int(m.group(1))
        if node in seen:
            raise ValueError(f'{path}: line {k + 1} labels node {node} a second time')
        seen.add(node)
        ids.append(node)
        tokens.append(m.group(2).decode(errors='replace'))
    return np.asarray(ids, dtype=np.int64), tokens


_LABEL_SET_LINE = re.compile(rb'([0-9]{1,18})((?:[ \t,]+[^ \t,\r\n]+)+)[ \t,]*\Z')


def read_node_label_sets(path: str, skip_rows: int = 0) -> Tuple[np.ndarray, List[List[str]]]:
    """(ids int64[m], label tokens of each id) of a multi-label file: the distinct ids in order
    of first appearance, each with its distinct tokens in order of first appearance. ``.npz``
    (integer arrays ``node`` and ``label``, one entry per (node, label) pair), anything else as
    text lines ``node l1 [l2 ...]`` (module docstring). A node may be named on several lines or
    entries; a repeated pair counts once."""
    path = os.fspath(path)
    if skip_rows < 0:
        raise ValueError('skip_rows must be non-negative')
    sets = {}
    if os.path.splitext(path)[1].lower() == '.npz':
        with np.load(path, allow_pickle=False) as f:
            node, label = np.asarray(f['node']), np.asarray(f['label'])
        if node.ndim != 1 or node.shape != label.shape or node.dtype.kind not in 'iu' \
                or label.dtype.kind not in 'iu':
            raise ValueError(f'{path}: node and label must be 1-d integer arrays of one length')
        for u, v in zip(_host_ids(node, 'node').tolist(), label.tolist()):
            sets.setdefault(u, {})[str(v)] = None
    else:
        for k, line, t in _label_lines(path, skip_rows):
            m = _LABEL_SET_LINE.match(t)
            if m is None:
                raise ValueError(f'{path}: line {k + 1} is not a node and its labels: '
                                 f'{line[:60].decode(errors="replace")!r}')
            mine = sets.setdefault(int(m.group(1)), {})
            for token in re.split(rb'[ \t,]+', m.group(2).strip(b' \t,')):
                mine[token.decode(errors='replace')] = None
    return np.asarray(list(sets), dtype=np.int64), [list(v) for v in sets.values()]
