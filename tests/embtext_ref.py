"""The word2vec-text contract of shallow_encoders/word2vec/embeddings_io.py restated with numpy
and CPython alone — test infrastructure:

  * ``token``: the token of one float32, by the executable definition
    ``repr(float(numpy.format_float_scientific(numpy.float32(x), unique=True, trim='-')))``
    (numpy's unique-mode Dragon4 picks the shortest digits, CPython's repr lays them out);
  * ``file_bytes``: header, keys and joined tokens of a whole file;
  * ``hard_bits``: the float32 bit patterns where a shortest-digits conversion can go wrong;
  * ``host_tokens`` / ``host_file``: the library's host path (dw_embtext_host) through ctypes.
"""
import ctypes

import numpy as np

MAX_TOKEN = 19


def token(x) -> str:
    x = np.float32(x)
    if np.isnan(x):
        return 'nan'
    return repr(float(np.format_float_scientific(x, unique=True, trim='-')))


def tokens(values) -> list:
    return [token(v) for v in np.asarray(values, dtype=np.float32).ravel()]


def file_bytes(keys, table) -> bytes:
    table = np.asarray(table, dtype=np.float32)
    lines = [f'{table.shape[0]} {table.shape[1]}']
    for k, row in zip(keys, table):
        lines.append(' '.join([str(k)] + [token(v) for v in row]))
    return ('\n'.join(lines) + '\n').encode('utf-8')


def as_f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint64).astype(np.uint32).view(np.float32)


def hard_bits() -> np.ndarray:
    """uint32 bit patterns: every power of two with its neighbours (the uneven rounding
    intervals), the floats around every power of ten, the layout thresholds 1e-4 and 1e16,
    2^24 +- 1, the ends of the subnormal and normal ranges, zeros, infinities and NaNs."""
    b = []
    for k in range(-149, 128):
        p = int(np.float32(2.0 ** k).view(np.uint32))
        b += [p - 1, p, p + 1]
    for k in range(-45, 39):
        p = int(np.float32(float(f'1e{k}')).view(np.uint32))
        b += [q for q in range(p - 2, p + 3) if 0 <= q < 0x7F800000]
    for v in (1e-4, 1e16, 1e-5, 1e15, 1e17, 9999999e9):
        p = int(np.float32(v).view(np.uint32))
        b += list(range(p - 3, p + 4))
    b += [int(np.float32(v).view(np.uint32)) for v in (2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2)]
    b += [1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF]          # subnormal ends, FLT_MIN, FLT_MAX
    pos = np.asarray(sorted(set(b)), dtype=np.uint32)
    special = np.asarray([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                          0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA55555],
                         dtype=np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000), special])


def strided_bits(stride: int = 4099) -> np.ndarray:
    """Every stride-th of all 2^32 bit patterns."""
    return np.arange(0, 1 << 32, stride, dtype=np.uint64).astype(np.uint32)


def _lib():
    from shallow_encoders import _native
    return _native, _native.load()


def host_lines(table, rows=None, keys_i64=None, key_strs=None, r0=None, r1=None):
    """(bytes of lines [r0, r1), line_off, status) from dw_embtext_host; the write pass gets a
    buffer of exactly the bytes it needs, with a canary behind it."""
    _native, lib = _lib()
    table = np.ascontiguousarray(table, dtype=np.float32)
    V, d = table.shape
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    n = V if rows is None else len(rows)
    kb = ko = None
    if key_strs is not None:
        enc = [k.encode('utf-8') for k in key_strs]
        ko = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(e) for e in enc], out=ko[1:])
        kb = np.frombuffer(b''.join(enc) or b'\0', dtype=np.uint8).copy()
    elif keys_i64 is None:
        keys_i64 = np.arange(n, dtype=np.int64)
    if keys_i64 is not None:
        keys_i64 = np.ascontiguousarray(keys_i64, dtype=np.int64)

    def p(a):
        return None if a is None else a.ctypes.data
    line_off = np.zeros(n + 1, dtype=np.int64)
    status = ctypes.c_int32(0)
    args = (table.ctypes.data, V, d, p(rows), n, p(keys_i64), p(kb), p(ko), line_off.ctypes.data)
    _native.call('dw_embtext_host', *args, 0, n, None, 0, ctypes.byref(status))
    r0 = 0 if r0 is None else r0
    r1 = n if r1 is None else r1
    size = int(line_off[r1] - line_off[r0])
    buf = np.full(size + 32, 0xA5, dtype=np.uint8)
    _native.call('dw_embtext_host', *args, r0, r1, buf.ctypes.data, size, ctypes.byref(status))
    assert (buf[size:] == 0xA5).all(), 'dw_embtext_host wrote past the bytes it announced'
    return buf[:size].tobytes(), line_off, status.value


def host_tokens(bits) -> list:
    """The library's token of every bit pattern (one value a line, key 0)."""
    vals = np.asarray(bits, dtype=np.uint32).view(np.float32).reshape(-1, 1)
    text, _, _ = host_lines(vals, keys_i64=np.zeros(len(vals), dtype=np.int64))
    lines = text.decode('ascii').split('\n')
    assert lines.pop() == '' and len(lines) == len(vals)
    assert all(ln.startswith('0 ') for ln in lines)
    return [ln[2:] for ln in lines]
