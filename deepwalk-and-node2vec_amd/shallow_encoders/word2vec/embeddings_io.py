"""Embedding tables as word2vec text (the ``.emb`` files node2vec and DeepWalk emit).

    <n> <d>\\n
    <key> <T(v_0)> <T(v_1)> ... <T(v_{d-1})>\\n      (n such lines)

single spaces, ``\\n`` line ends, no trailing blanks. ``T(x)`` is the shortest decimal that reads
back as the float32 ``x``, laid out as ``repr(float)`` lays out a double with those digits
(``0.0001``, ``1e-05``, ``-0.0``, ``nan``, ``inf``); gensim's ``load_word2vec_format`` and
``np.loadtxt`` read the files. A device tensor is converted by the HIP kernels of
csrc/dw_embtext.hip, a host tensor or array by the same code compiled for the host
(``dw_embtext_host``): the two paths write the same bytes.

The way back is ``read_word2vec_format``: any such file — this writer's, the node2vec and DeepWalk
reference programs', gensim's — into a float32 table, by the HIP kernels of csrc/dw_embread.hip
on a device or the same code on the host (``dw_embread_host``), a token's value being
``numpy.float32(float(token))`` as in ``load_word2vec_format``; ``align_word2vec`` then places the
rows at the vocabulary rows their keys name.
"""
import contextlib
import ctypes
import logging
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from shallow_encoders import _native

logger = logging.getLogger('EmbeddingsIO')

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



# ------------------------------------------------------------------------------------ reading
UNDECIDED_CAPACITY = 1 << 16   # entries of a chunk's first try; a fuller chunk is parsed again
_pow5 = {}


def pow5_table(device: Optional[torch.device] = None):
    """The decimal conversion's powers of five (dw_pow5_table): a numpy uint64 [1302] array, or
    its copy on ``device`` as int64 bits; built once."""
    if 'host' not in _pow5:
        t = np.zeros(1302, dtype=np.uint64)
        _native.call('dw_pow5_table', t.ctypes.data)
        _pow5['host'] = t
    if device is None:
        return _pow5['host']
    key = str(device)
    if key not in _pow5:
        _pow5[key] = torch.from_numpy(_pow5['host'].view(np.int64)).to(device)
    return _pow5[key]


class Word2VecText:
    """What read_word2vec_format returns: ``n`` lines of ``d`` values; ``table`` float32 [n, d]
    (a torch tensor on the reader's device, or a numpy array); ``keys_i64`` int64 [n] when every
    key is a plain decimal integer (1 to 18 digits, no sign, no leading zero), else None;
    ``keys()`` the keys as str, in file order; ``host_tokens`` how many value tokens the native
    conversion left to Python's float()."""

    def __init__(self, n, d, table, key_values, text_keys, host_tokens=0):
        self.n, self.d, self.table, self.host_tokens = n, d, table, host_tokens
        self._values = key_values      # int64 [n], -1 where the key is in _text
        self._text = text_keys         # {line: str}
        self.keys_i64 = key_values if not text_keys else None

    def keys(self) -> List[str]:
        out = [str(v) for v in self._values.tolist()]
        for i, k in self._text.items():
            out[i] = k
        return out


class _TextError(Exception):
    """A line of the body is wrong: the 0-based body line and what is wrong with it."""

    def __init__(self, line: int, what: str):
        super().__init__(what)
        self.line, self.what = line, what


def _line_chunks(f, chunk_bytes: int):
    """The rest of ``f`` in runs of whole lines of at most chunk_bytes each; a longer line is a
    chunk of its own, and the last chunk may lack its line end."""
    buf, step = b'', max(chunk_bytes, 1 << 16)
    while True:
        cut = buf.rfind(b'\n', 0, chunk_bytes) + 1 or buf.find(b'\n') + 1
        if cut:
            yield memoryview(buf)[:cut]   # (no copy of the chunk; the short rest is copied)
            buf = buf[cut:]
            continue
        block = f.read(step)
        if not block:
            if buf:
                yield memoryview(buf)
            return
        buf = buf + block if buf else block


def _settle(chunk, row0, lines, bad_line, status, undecided, key_off, key_len, key_i64, table,
            text_keys):
    """A parsed chunk's host work: the undecided tokens through float(), the text keys' bytes
    from the host's copy of the chunk, and the chunk's first error. ``undecided``: int64 [k, 4];
    key_off / key_len / key_i64: the chunk's rows (key_off None when every key is an integer: a
    bad line's row keeps the arrays' initial 0, so it is never taken for a text key);
    ``table``: the whole table (tensor or array). Returns the values to patch in."""
    first = None   # (body line, message)

    def fail(line, what):
        nonlocal first
        if first is None or line < first[0]:
            first = (line, what)
    if status & _native.DW_S_BAD_TEXT:
        fail(row0 + bad_line, 'the line does not hold a key and the announced number of values')
    patches = []
    for r, c, off, ln in undecided.tolist():
        tok = bytes(chunk[off:off + ln])
        try:
            patches.append((r, c, float(tok)))
        except ValueError:
            fail(r, f'could not convert {tok[:40]!r} to float')
    if key_off is not None:
        for i in np.flatnonzero(key_i64 < 0).tolist():
            raw = bytes(chunk[int(key_off[i]):int(key_off[i] + key_len[i])])
            try:
                text_keys[row0 + i] = raw.decode('utf-8')
            except UnicodeDecodeError as exc:
                fail(row0 + i, str(exc))
    if first is not None:
        raise _TextError(*first)
    return patches


def _patch(table, patches) -> None:
    if not patches:
        return
    with np.errstate(over='ignore'):
        vals = np.asarray([v for _, _, v in patches], dtype=np.float64).astype(np.float32)
    rows = np.asarray([r for r, _, _ in patches], dtype=np.int64)
    cols = np.asarray([c for _, c, _ in patches], dtype=np.int64)
    if isinstance(table, torch.Tensor):
        table[torch.from_numpy(rows).to(table.device), torch.from_numpy(cols).to(table.device)] = \
            torch.from_numpy(vals).to(table.device)
    else:
        table[rows, cols] = vals


def _read_host(chunks, n, d):
    table = np.zeros((n, d), dtype=np.float32)
    key_off, key_len = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    key_i64 = np.zeros(n, dtype=np.int64)
    counts, err = np.zeros(2, dtype=np.int64), ctypes.c_int64(-1)
    text_keys, row0, host_tokens = {}, 0, 0
    for chunk in chunks:
        data = np.frombuffer(chunk, dtype=np.uint8)
        cap = UNDECIDED_CAPACITY
        while True:
            und = np.zeros((cap, 4), dtype=np.int64)
            status = ctypes.c_int32(0)
            _native.call('dw_embread_host', data.ctypes.data, len(data), d, table.ctypes.data, n,
                         row0, key_off.ctypes.data, key_len.ctypes.data, key_i64.ctypes.data,
                         und.ctypes.data, cap, counts.ctypes.data, ctypes.byref(err),
                         ctypes.byref(status))
            if counts[1] <= cap:
                break
            cap = int(counts[1])
        lines = int(counts[0])
        if row0 + lines > n:
            raise _TextError(-1, 'more lines than announced')
        sl = slice(row0, row0 + lines)
        text = bool(status.value & _native.DW_S_TEXT_KEY)
        _patch(table, _settle(data, row0, lines, err.value, status.value, und[:int(counts[1])],
                              key_off[sl] if text else None, key_len[sl], key_i64[sl], table,
                              text_keys))
        row0 += lines
        host_tokens += int(counts[1])
    if row0 != n:
        raise _TextError(-1, 'fewer lines than announced')
    return table, key_i64, text_keys, host_tokens


class _DeviceReader:
    """The device buffers of one read: the outputs, and per staging slot the chunk's text in
    pinned host memory and in HBM, its status word, counters and undecided list."""

    def __init__(self, dev, n, d, cap_bytes):
        self.dev, self.n, self.d = dev, n, d

        def z(*shape, dtype=torch.int64):
            return torch.zeros(*shape, dtype=dtype, device=dev)
        self.table = z(n, d, dtype=torch.float32)
        self.key_off, self.key_len, self.key_i64 = z(n), z(n), z(n)
        self.line_off = z(n + 1)
        self.pow5 = pow5_table(dev)
        self.copy_stream = torch.cuda.Stream(dev)
        self.copied = [torch.cuda.Event() for _ in range(2)]
        self.status = [z(1, dtype=torch.int32) for _ in range(2)]
        self.counts = [z(2) for _ in range(2)]
        self.err = [z(1) for _ in range(2)]
        self.undecided = [z(UNDECIDED_CAPACITY, 4) for _ in range(2)]
        self.hbuf = self.dbuf = self.ws = None
        self.host_tokens = 0
        self.reserve(cap_bytes)

    def reserve(self, cap_bytes):
        """Staging and workspace for chunks of cap_bytes (grown for a line longer than that)."""
        if self.hbuf is not None and self.hbuf[0].numel() >= cap_bytes:
            return
        torch.cuda.synchronize(self.dev)
        self.hbuf = [torch.empty(cap_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.dbuf = [torch.empty(cap_bytes, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        ws_bytes = ctypes.c_size_t(0)
        _native.call('dw_embread_workspace_bytes', cap_bytes, ctypes.byref(ws_bytes))
        self.ws = torch.empty(max(1, ws_bytes.value), dtype=torch.uint8, device=self.dev)

    def upload(self, k, chunk):
        """Chunk k to HBM on the copy stream, beside whatever the main stream runs."""
        s, size = k % 2, len(chunk)
        self.hbuf[s].numpy()[:size] = np.frombuffer(chunk, dtype=np.uint8)
        with torch.cuda.stream(self.copy_stream):
            self.dbuf[s][:size].copy_(self.hbuf[s][:size], non_blocking=True)
            self.copied[s].record()

    def parse(self, k, size, row0):
        """Both passes over chunk k; returns its line count (one synchronisation, between the
        passes: the header's n is checked against it before anything is stored)."""
        s, st = k % 2, _native.stream(self.dev)
        torch.cuda.current_stream(self.dev).wait_event(self.copied[s])
        self.status[s].zero_()
        text = self.dbuf[s].data_ptr()
        _native.call('dw_embread_lines', text, size, self.line_off.data_ptr(), self.n - row0,
                     self.counts[s].data_ptr(), self.err[s].data_ptr(), self.ws.data_ptr(),
                     self.ws.numel(), st)
        lines = int(self.counts[s][0].item())
        if row0 + lines > self.n:
            raise _TextError(-1, 'more lines than announced')
        self.launch(s, text, size, lines, row0, self.undecided[s])
        return lines

    def launch(self, s, text, size, lines, row0, undecided):
        _native.call('dw_embread_parse', text, size, self.line_off.data_ptr(), lines, self.d,
                     self.pow5.data_ptr(), self.table.data_ptr(), self.n, row0,
                     self.key_off.data_ptr(), self.key_len.data_ptr(), self.key_i64.data_ptr(),
                     undecided.data_ptr(), undecided.shape[0], self.counts[s].data_ptr(),
                     self.err[s].data_ptr(), self.status[s].data_ptr(), _native.stream(self.dev))

    def settle(self, k, size, lines, row0, text_keys):
        """Waits for chunk k's parse and does its host work (_settle)."""
        s = k % 2
        status, n_und = int(self.status[s].item()), int(self.counts[s][1].item())
        und = self.undecided[s]
        self.host_tokens += n_und
        if n_und > und.shape[0]:   # the list overflowed: the outputs are pure, parse once more
            und = torch.zeros(n_und, 4, dtype=torch.int64, device=self.dev)
            self.counts[s][1] = 0
            self.launch(s, self.dbuf[s].data_ptr(), size, lines, row0, und)
        sl = slice(row0, row0 + lines)
        text = bool(status & _native.DW_S_TEXT_KEY)
        patches = _settle(self.hbuf[s].numpy()[:size], row0, lines, int(self.err[s].item()), status,
                          und[:n_und].cpu().numpy(),
                          self.key_off[sl].cpu().numpy() if text else None,
                          self.key_len[sl].cpu().numpy() if text else None,
                          self.key_i64[sl].cpu().numpy() if text else None, self.table,
                          text_keys)
        _patch(self.table, patches)


def _read_device(chunks, n, d, dev, chunk_bytes, size_hint):
    dev = _native.require_device(dev)
    with torch.cuda.device(dev):
        rd = _DeviceReader(dev, n, d, max(16, min(chunk_bytes, size_hint)))
        text_keys, row0, pending = {}, 0, None
        for k, chunk in enumerate(chunks):
            if len(chunk) > rd.hbuf[0].numel():   # a line longer than chunk_bytes
                if pending is not None:
                    rd.settle(*pending, text_keys)
                    pending = None
                rd.reserve(len(chunk))
            rd.upload(k, chunk)
            if pending is not None:   # chunk k - 1's parse ran beside this copy
                rd.settle(*pending, text_keys)
            lines = rd.parse(k, len(chunk), row0)
            pending = (k, len(chunk), lines, row0)
            row0 += lines
        if pending is not None:
            rd.settle(*pending, text_keys)
        if row0 != n:
            raise _TextError(-1, 'fewer lines than announced')
        return rd.table, rd.key_i64.cpu().numpy(), text_keys, rd.host_tokens


def read_word2vec_format(path: str, device=None, chunk_bytes: int = 256 << 20) -> Word2VecText:
    """A word2vec text file as a Word2VecText, read by the HIP kernels of csrc/dw_embread.hip on
    ``device`` (the table stays there), or with device=None by the same code on the host
    (``dw_embread_host``, a numpy table): both give the same bits, those of load_word2vec_format
    — a token's value is ``numpy.float32(float(token))`` — and refuse the same files with a
    ValueError naming the 1-based line. The file is read in chunks of at most chunk_bytes that
    break at line ends (a longer line is a chunk of its own); on the device they go through two
    pinned staging buffers, so the copy of a chunk runs beside the parse of the one before it."""
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes must be >= 1')
    with open(path, 'rb') as f:
        head = f.readline()
        try:
            n, d = (int(x) for x in head.split())
            if n < 0 or d < 1:
                raise ValueError
        except ValueError:
            raise ValueError(f'{path}: line 1: the header must be "<n> <d>"') from None
        body = f.tell()
        chunks = _line_chunks(f, chunk_bytes)
        try:
            if device is None:
                out = _read_host(chunks, n, d)
            else:
                out = _read_device(chunks, n, d, device, chunk_bytes,
                                   os.path.getsize(path) - body)
        except _TextError as exc:
            # like the loader, the count of lines is checked before any of them
            f.seek(body)
            rest = f.read()
            held = rest.count(b'\n') + (1 if rest and not rest.endswith(b'\n') else 0)
            if held != n:
                raise ValueError(f'{path}: line 1: the header announces {n} lines, the file '
                                 f'holds {held}') from None
            raise ValueError(f'{path}: line {exc.line + 2}: {exc.what}') from None
    return Word2VecText(n, d, *out)


def _vocabulary_keys(csr_or_vocab, style: str) -> List[str]:
    """One key per vocabulary row, row 0 (``<unk>``) included, as export_keys writes them."""
    if hasattr(csr_or_vocab, 'export_keys'):
        return [str(k) for k in csr_or_vocab.export_keys(style, include_unk=True)]
    itos = csr_or_vocab.get_itos() if hasattr(csr_or_vocab, 'get_itos') else csr_or_vocab
    return [str(k) for k in itos]


def _rows_of_integer_keys(keys: torch.Tensor, csr, V: int):
    """(vocabulary row of every integer key, whether it names one) on the keys' device, for the
    graphs whose 'id' keys are integers; None for the others."""
    from shallow_encoders.graph.csr import IdNames, NodeNames
    itos = getattr(csr, 'itos', None)
    if isinstance(itos, NodeNames):
        return keys + 1, (keys >= 0) & (keys < V - 1)
    if isinstance(itos, IdNames) and len(itos.ids):
        ids = torch.from_numpy(itos.ids).to(keys.device)
        pos = torch.searchsorted(ids, keys).clamp_(max=len(ids) - 1)
        return pos + 1, ids[pos] == keys
    return None


def align_word2vec(result: Word2VecText, csr_or_vocab, missing: str = 'error',
                   style: str = 'id'):
    """float32 [V, d]: the file's rows at the vocabulary rows their keys name, the inverse of
    ``CSRGraph.export_keys(style)`` — with style 'id' an edge-list graph's ids, a synthetic
    graph's node numbers, else ``str(name)``; with 'token' the vocabulary tokens; ``<unk>`` is
    row 0. csr_or_vocab: a CSRGraph, a vocabulary (``get_itos()``) or a list of tokens. Integer
    keys of an edge-list or synthetic graph are matched on the table's device (searchsorted,
    index_copy_), other keys through a dict. A key the vocabulary does not hold and a key that
    occurs twice raise ValueError naming the key and its line. Vocabulary rows the file does not
    hold (row 0 aside) raise under missing='error'; under 'zero' they stay zero rows and their
    count is logged (node2vec's program omits nodes no walk reached). The result is a tensor on
    the table's device, or a numpy array for a numpy table."""
    if missing not in ('error', 'zero'):
        raise ValueError(f'missing must be "error" or "zero", got {missing!r}')
    as_numpy = not isinstance(result.table, torch.Tensor)
    table = torch.from_numpy(result.table) if as_numpy else result.table
    dev = table.device
    V = csr_or_vocab.vocab_size if hasattr(csr_or_vocab, 'vocab_size') else \
        len(_vocabulary_keys(csr_or_vocab, style))
    found = None
    if style == 'id' and result.keys_i64 is not None and result.n:
        found = _rows_of_integer_keys(torch.from_numpy(result.keys_i64).to(dev), csr_or_vocab, V)
    if found is not None:
        rows, ok = found
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0, 0])
            raise ValueError(f'key {int(result.keys_i64[i])} (line {i + 2}) is not in the '
                             f'vocabulary')
    else:
        index = {k: r for r, k in enumerate(_vocabulary_keys(csr_or_vocab, style))}
        rows = np.empty(result.n, dtype=np.int64)
        for i, k in enumerate(result.keys()):
            if k not in index:
                raise ValueError(f'key {k!r} (line {i + 2}) is not in the vocabulary')
            rows[i] = index[k]
        rows = torch.from_numpy(rows).to(dev)
    order = torch.argsort(rows, stable=True)
    twice = (rows[order][1:] == rows[order][:-1]).nonzero()
    if len(twice):
        i = int(order[1:][twice[:, 0]].min())
        raise ValueError(f'key {result.keys()[i]!r} (line {i + 2}) occurs twice')
    absent = V - 1 - int((rows != 0).sum())
    if absent:
        if missing == 'error':
            held = torch.zeros(V, dtype=torch.bool, device=dev)
            held[rows] = True
            r = int((~held[1:]).nonzero()[0, 0]) + 1
            raise ValueError(f'{absent} vocabulary rows are not in the file (the first is row '
                             f'{r}); pass missing="zero" to leave them zero')
        logger.info(f'align_word2vec: {absent} of {V - 1} vocabulary rows are not in the file; '
                    f'they stay zero.')
    out = torch.zeros(V, result.d, dtype=torch.float32, device=dev)
    out.index_copy_(0, rows, table)
    return out.numpy() if as_numpy else out
