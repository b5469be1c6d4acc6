"""The word2vec-text reader's contract (shallow_encoders/word2vec/embeddings_io.py:
read_word2vec_format) restated with CPython and numpy alone — test infrastructure:

  * ``law``: a value token's float32 bits, ``numpy.float32(float(token))``;
  * ``read_body``: a file body to table bits, key spans, integer keys, line count, first bad
    line and status, by ``split(b'\\n')`` and ``.split()``; independent of the native code;
  * ``host_body`` / ``token``: the library's host path (dw_embread_host, dw_f32_token_host)
    through ctypes, with outputs of exactly the needed size and canaries behind them.
"""
import ctypes
import re
import warnings

import numpy as np

S_BAD_TEXT = 256
S_TEXT_KEY = 8192
TOKEN_BAD, TOKEN_DECIDED, TOKEN_UNDECIDED = 0, 1, 2
CANARY = 0x5A


def law(tok) -> int:
    """uint32 bits of numpy.float32(float(tok)); ValueError where float() refuses."""
    if isinstance(tok, str):
        tok = tok.encode()
    with warnings.catch_warnings(), np.errstate(over='ignore'):
        warnings.simplefilter('ignore')
        return int(np.asarray([float(tok)], dtype=np.float64).astype(np.float32)
                   .view(np.uint32)[0])


def key_value(key: bytes) -> int:
    """The key as an integer where str(int) gives its bytes back (1 to 18 digits), else -1."""
    return int(key) if re.fullmatch(rb'0|[1-9][0-9]{0,17}', key) else -1


def read_body(body: bytes, d: int, n_rows=None, row0: int = 0):
    """dict(table uint32 [n_rows, d], key_off, key_len, key_i64, lines, err_line, status,
    unparsable) of a body. A token float() refuses reads as 0.0 and is listed in ``unparsable``
    as (row, column); rows of bad lines and rows the body does not reach keep their zeros."""
    lines = body.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    n_rows = row0 + len(lines) if n_rows is None else n_rows
    table = np.zeros((n_rows, d), dtype=np.uint32)
    key_off, key_len = np.zeros(n_rows, dtype=np.int64), np.zeros(n_rows, dtype=np.int64)
    key_i64 = np.zeros(n_rows, dtype=np.int64)
    err_line, status, unparsable, start = -1, 0, [], 0
    for i, raw in enumerate(lines):
        row = row0 + i
        parts = raw.split()
        if row < n_rows:
            if len(parts) != d + 1:
                status |= S_BAD_TEXT
                err_line = i if err_line < 0 else err_line
            else:
                at = re.search(rb'[^ \t\r\x0b\x0c]', raw).start()
                key_off[row], key_len[row] = start + at, len(parts[0])
                key_i64[row] = key_value(parts[0])
                if key_i64[row] < 0:
                    status |= S_TEXT_KEY
                for c, tok in enumerate(parts[1:]):
                    try:
                        table[row, c] = law(tok)
                    except ValueError:
                        unparsable.append((row, c))
        start += len(raw) + 1
    return dict(table=table, key_off=key_off, key_len=key_len, key_i64=key_i64,
                lines=len(lines), err_line=err_line, status=status, unparsable=unparsable)


def _lib():
    from shallow_encoders import _native
    return _native, _native.load()


def token(tok):
    """(kind, uint32 bits) of one value token from dw_f32_token_host."""
    _native, _ = _lib()
    if isinstance(tok, str):
        tok = tok.encode()
    buf = np.frombuffer(tok, dtype=np.uint8).copy() if tok else np.zeros(1, dtype=np.uint8)
    kind, bits = ctypes.c_int32(-1), ctypes.c_uint32(0xDEADBEEF)
    _native.call('dw_f32_token_host', buf.ctypes.data, len(tok), ctypes.byref(kind),
                 ctypes.byref(bits))
    return kind.value, bits.value


def host_body(body: bytes, d: int, n_rows=None, row0: int = 0, undecided_capacity: int = 4096):
    """read_body's dict from dw_embread_host, plus ``undecided`` (a sorted list of (row, column,
    offset, length)) and ``n_undecided``; undecided tokens read as 0.0, as on the device. The
    text sits in an array of exactly len(body) bytes, the outputs have canaries behind them."""
    _native, _ = _lib()
    if n_rows is None:
        n_rows = row0 + body.count(b'\n') + (1 if body and not body.endswith(b'\n') else 0)
    text = np.frombuffer(body, dtype=np.uint8).copy() if body else np.zeros(0, dtype=np.uint8)

    def guarded(n, dtype):
        a = np.zeros(n + 4, dtype=dtype)
        a[n:].view(np.uint8)[:] = CANARY
        return a
    table = guarded(n_rows * d, np.uint32)
    key_off, key_len, key_i64 = (guarded(n_rows, np.int64) for _ in range(3))
    und = guarded(4 * undecided_capacity, np.int64)
    counts, err, status = np.zeros(2, dtype=np.int64), ctypes.c_int64(-7), ctypes.c_int32(0)
    _native.call('dw_embread_host', text.ctypes.data if len(text) else None, len(text), d,
                 table.ctypes.data, n_rows, row0, key_off.ctypes.data, key_len.ctypes.data,
                 key_i64.ctypes.data, und.ctypes.data, undecided_capacity, counts.ctypes.data,
                 ctypes.byref(err), ctypes.byref(status))
    for a, n in ((table, n_rows * d), (key_off, n_rows), (key_len, n_rows), (key_i64, n_rows),
                 (und, 4 * undecided_capacity)):
        assert (a[n:].view(np.uint8) == CANARY).all(), 'dw_embread_host wrote past an output'
    kept = min(int(counts[1]), undecided_capacity)
    return dict(table=table[:n_rows * d].reshape(n_rows, d), key_off=key_off[:n_rows],
                key_len=key_len[:n_rows], key_i64=key_i64[:n_rows], lines=int(counts[0]),
                err_line=err.value, status=status.value, n_undecided=int(counts[1]),
                undecided=sorted(map(tuple, und[:4 * kept].reshape(-1, 4).tolist())))


def file_of(keys, rows, header=None, sep=' ', eol='\n') -> bytes:
    """A file of the given token rows (lists of str), each behind its key."""
    d = len(rows[0]) if rows else 1
    head = f'{len(rows)} {d}' if header is None else header
    return (head + eol + ''.join(sep.join([str(k)] + list(r)) + eol
                                 for k, r in zip(keys, rows))).encode('utf-8')
