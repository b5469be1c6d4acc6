"""Embedding tables as word2vec text (the ``.emb`` files node2vec and DeepWalk emit).

    <n> <d>\\n
    <key> <T(v_0)> <T(v_1)> ... <T(v_{d-1})>\\n      (n such lines)

single spaces, ``\\n`` line ends, no trailing blanks. ``T(x)`` is the shortest decimal that reads
back as the float32 ``x``, laid out as ``repr(float)`` lays out a double with those digits
(``0.0001``, ``1e-05``, ``-0.0``, ``nan``, ``inf``); gensim's ``load_word2vec_format`` and
``np.loadtxt`` read the files. A device tensor is converted by the HIP kernels of
csrc/dw_embtext.hip, a host tensor or array by the same code compiled for the host
(``dw_embtext_host``): the two paths write the same bytes.
"""
import contextlib
import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from shallow_encoders import _native

TABLE_WORDS = 79
MAX_TOKEN = 19
_tables = {}


def f32text_table(device: Optional[torch.device] = None):
    """The conversion's powers-of-five table (dw_f32text_table): a numpy uint64 [79] array, or
    its copy on ``device`` as int64 bits; built once."""
    if 'host' not in _tables:
        t = np.zeros(TABLE_WORDS, dtype=np.uint64)
        _native.call('dw_f32text_table', t.ctypes.data)
        _tables['host'] = t
    if device is None:
        return _tables['host']
    key = str(device)
    if key not in _tables:
        _tables[key] = torch.from_numpy(_tables['host'].view(np.int64)).to(device)
    return _tables[key]


def _key_arrays(keys, n: int):
    """(int64 [n] or None, uint8 bytes or None, int64 [n + 1] offsets or None) of ``keys``."""
    if keys is None:
        return np.arange(n, dtype=np.int64), None, None
    if isinstance(keys, torch.Tensor):
        keys = keys.detach().cpu().numpy()
    if isinstance(keys, np.ndarray) and keys.dtype.kind in 'iu':
        k = np.ascontiguousarray(keys, dtype=np.int64)
        if k.shape != (n,):
            raise ValueError(f'keys must have one entry per line: {k.shape} for {n} lines')
        if n and int(k.min()) < 0:
            raise ValueError(f'integer keys must be >= 0, got {int(k.min())}')
        return k, None, None
    keys = list(keys)
    if len(keys) != n:
        raise ValueError(f'keys must have one entry per line: {len(keys)} for {n} lines')
    if all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in keys):
        return _key_arrays(np.asarray(keys, dtype=np.int64), n)
    enc = []
    for i, k in enumerate(keys):
        if not isinstance(k, str):
            raise TypeError(f'key {i} is {type(k).__name__}: keys are all int or all str')
        if k == '' or any(c.isspace() for c in k):
            raise ValueError(f'key {i} ({k!r}) is empty or holds a blank, a tab or a line end')
        enc.append(k.encode('utf-8'))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=off[1:])
    data = np.frombuffer(b''.join(enc) or b'\0', dtype=np.uint8).copy()
    return None, data, off


def _first_nonfinite(table, rows) -> Tuple[int, int, int]:
    """(line, table row, column) of the first nan or inf among the written rows."""
    t = torch.as_tensor(table)
    step = max(1, (1 << 24) // max(1, t.shape[1]))
    n = len(rows) if rows is not None else t.shape[0]
    for a in range(0, n, step):
        sel = t[torch.as_tensor(rows[a:a + step], device=t.device)] if rows is not None \
            else t[a:a + step]
        bad = (~torch.isfinite(sel)).nonzero()
        if len(bad):
            r, c = int(bad[0, 0]) + a, int(bad[0, 1])
            return r, (int(rows[r]) if rows is not None else r), c
    raise AssertionError('no non-finite value found')


def _chunks(line_off: np.ndarray, chunk_bytes: int) -> List[Tuple[int, int]]:
    """Row ranges [r0, r1) of at most chunk_bytes each, and of at least one line."""
    out, r0, n = [], 0, len(line_off) - 1
    while r0 < n:
        r1 = int(np.searchsorted(line_off, line_off[r0] + chunk_bytes, side='right')) - 1
        r1 = min(n, max(r0 + 1, r1))
        out.append((r0, r1))
        r0 = r1
    return out


def _p(a) -> Optional[int]:
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def save_word2vec_format(path: str, table, keys=None, rows=None, nonfinite: str = 'error',
                         chunk_bytes: int = 256 << 20) -> int:
    """Write rows of ``table`` (float32 [V, d], a torch tensor or numpy array) to ``path`` in
    word2vec text format; returns the bytes written.

    rows: int64 ids of the rows to write, in file order (None: all of them). keys: one per
    written row — an int64 array or tensor (>= 0), a sequence of str (UTF-8, no blank, tab or
    line end), or None for the row's position. nonfinite: 'error' raises ValueError naming the
    first nan or inf (row, column) before anything is written; 'write' keeps ``nan`` / ``inf``.
    The file is written in chunks of at most chunk_bytes that break at line ends (a longer line
    is a chunk of its own); on the device the copy of one chunk to the host overlaps the file
    write of the one before it."""
    if nonfinite not in ('error', 'write'):
        raise ValueError(f'nonfinite must be "error" or "write", got {nonfinite!r}')
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes must be >= 1')
    on_device = isinstance(table, torch.Tensor) and table.is_cuda
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.float32 or table.dim() != 2:
            raise ValueError('table must be float32 [V, d]')
        table = table.detach().contiguous()
        if not on_device:
            table = table.numpy()
    else:
        table = np.asarray(table)
        if table.dtype != np.float32 or table.ndim != 2:
            raise ValueError('table must be float32 [V, d]')
        table = np.ascontiguousarray(table)
    V, d = int(table.shape[0]), int(table.shape[1])
    if V < 1 or d < 1:
        raise ValueError(f'table must hold at least one row and one column, got {V} x {d}')
    if rows is not None:
        if isinstance(rows, torch.Tensor):
            rows = rows.detach().cpu().numpy()
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 1:
            raise ValueError('rows must be one-dimensional')
    n = len(rows) if rows is not None else V
    k64, kbytes, koff = _key_arrays(keys, n)
    write = _write_device if on_device else _write_host
    return write(path, table, V, d, rows, n, k64, kbytes, koff, nonfinite, chunk_bytes)


@contextlib.contextmanager
def _output(path: str):
    """The file opened for writing; a failure while it is written leaves no file behind."""
    f = open(path, 'wb')
    try:
        with f:
            yield f
    except BaseException:
        os.remove(path)
        raise


def _check(st: int, table, rows, nonfinite: str) -> None:
    if st & _native.DW_S_BAD_INDEX:
        raise IndexError(f'save_word2vec_format: a row id is outside [0, {table.shape[0]})')
    if st & _native.DW_S_NONFINITE and nonfinite == 'error':
        line, r, c = _first_nonfinite(table, rows)
        raise ValueError(f'save_word2vec_format: non-finite value {float(table[r, c])} at row {r}, '
                         f'column {c} (line {line + 2} of the file); pass nonfinite="write" to '
                         f'keep it')
    if st & ~(_native.DW_S_BAD_INDEX | _native.DW_S_NONFINITE):
        raise RuntimeError(f'save_word2vec_format: status {st:#x}')


def _write_host(path, table, V, d, rows, n, k64, kbytes, koff, nonfinite, chunk_bytes) -> int:
    line_off = np.zeros(n + 1, dtype=np.int64)
    status = ctypes.c_int32(0)
    args = (table.ctypes.data, V, d, _p(rows), n, _p(k64), _p(kbytes), _p(koff),
            line_off.ctypes.data)
    _native.call('dw_embtext_host', *args, 0, n, None, 0, ctypes.byref(status))
    _check(status.value, table, rows, nonfinite)
    spans = _chunks(line_off, chunk_bytes)
    buf = np.empty(max([int(line_off[b] - line_off[a]) for a, b in spans] + [1]), dtype=np.uint8)
    header = f'{n} {d}\n'.encode()
    with _output(path) as f:
        f.write(header)
        for a, b in spans:
            size = int(line_off[b] - line_off[a])
            _native.call('dw_embtext_host', *args, a, b, buf.ctypes.data, size,
                         ctypes.byref(status))
            f.write(memoryview(buf)[:size])
    return len(header) + int(line_off[n])


def _write_device(path, table, V, d, rows, n, k64, kbytes, koff, nonfinite, chunk_bytes) -> int:
    dev = table.device
    _native.require_device(dev)

    def up(a):
        return None if a is None else torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        rows_d, k64_d, kbytes_d, koff_d = up(rows), up(k64), up(kbytes), up(koff)
        tab = f32text_table(dev)
        line_off_d = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = ctypes.c_size_t(0)
        _native.call('dw_embtext_workspace_bytes', n, d, ctypes.byref(ws_bytes))
        ws = torch.empty(max(1, ws_bytes.value), dtype=torch.uint8, device=dev)
        ins = (table.data_ptr(), V, d, _p(rows_d), n, _p(k64_d), _p(kbytes_d), _p(koff_d),
               tab.data_ptr())
        _native.call('dw_embtext_sizes', *ins, line_off_d.data_ptr(), status.data_ptr(),
                     ws.data_ptr(), ws.numel(), _native.stream(dev))
        line_off = line_off_d.cpu().numpy()
        _check(int(status.item()), table, rows, nonfinite)
        spans = _chunks(line_off, chunk_bytes)
        cap = max([int(line_off[b] - line_off[a]) for a, b in spans] + [1])
        dbuf = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        hbuf = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        header = f'{n} {d}\n'.encode()
        with _output(path) as f:
            f.write(header)

            def flush(k):   # chunk k's bytes are on the host once its event has passed
                a, b = spans[k]
                done[k % 2].synchronize()
                f.write(memoryview(hbuf[k % 2].numpy())[:int(line_off[b] - line_off[a])])
            for k, (a, b) in enumerate(spans):
                size = int(line_off[b] - line_off[a])
                _native.call('dw_embtext_write', *ins, line_off_d.data_ptr(), a, b,
                             dbuf[k % 2].data_ptr(), cap, status.data_ptr(), _native.stream(dev))
                hbuf[k % 2][:size].copy_(dbuf[k % 2][:size], non_blocking=True)
                done[k % 2].record()
                if k:
                    flush(k - 1)   # the file write of chunk k - 1 runs beside chunk k's copy
            if spans:
                flush(len(spans) - 1)
        _check(int(status.item()), table, rows, 'write')
    return len(header) + int(line_off[n])


def load_word2vec_format(path: str) -> Tuple[List[str], np.ndarray]:
    """(keys, float32 [n, d] table) of a word2vec text file. A token's value is
    ``numpy.float32(float(token))``, as gensim and ``np.loadtxt`` read it. Host only. A header
    that does not match the body, a short or long line and an unparsable token raise ValueError
    naming the 1-based line."""
    with open(path, 'rb') as f:
        lines = f.read().split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    head = lines[0].split() if lines else []
    try:
        n, d = (int(x) for x in head)
        if n < 0 or d < 1:
            raise ValueError
    except ValueError:
        raise ValueError(f'{path}: line 1: the header must be "<n> <d>"') from None
    if len(lines) - 1 != n:
        raise ValueError(f'{path}: line 1: the header announces {n} lines, the file holds '
                         f'{len(lines) - 1}' + (f' (line {n + 2} is the first extra one)'
                                                if len(lines) - 1 > n else ''))
    keys: List[str] = []
    table = np.empty((n, d), dtype=np.float64)
    for i, raw in enumerate(lines[1:]):
        parts = raw.split()
        if len(parts) != d + 1:
            raise ValueError(f'{path}: line {i + 2}: {len(parts) - 1} values, the header '
                             f'announces {d}')
        try:
            keys.append(parts[0].decode('utf-8'))
            table[i] = [float(p) for p in parts[1:]]
        except ValueError as exc:
            raise ValueError(f'{path}: line {i + 2}: {exc}') from None
    return keys, table.astype(np.float32)

