"""Restatement of the weighted edge-list text contract (shallow_encoders/graph/edge_list.py,
``weighted=True``; csrc/dw_strtod.h) in integer-only Python — test infrastructure:

  * ``pow5_entry`` / ``pow5_table``: the 128-bit powers of five, q in [-342, 308];
  * ``convert``: decimal significand w < 2^64 and power of ten q to the bits of a double, or
    ``None`` where the method cannot fix the rounding (Eisel-Lemire: Lemire, "Number parsing at
    a gigabyte per second", 2021);
  * ``scan_token`` / ``token_bits``: the weight token's grammar and its conversion;
  * ``parse_text_weighted``: a byte-at-a-time line parser for ``u v w`` lines;
  * the seeded token corpora and the bad-token list.

The reference is ``float(token)``: nothing here calls it except ``float_bits`` and the line
parser's test for an infinite weight.
"""
import struct

import numpy as np

import edgelist_ref as ref

Q_MIN, Q_MAX = -342, 308
MAX_TOKEN = 64
MAX_EXP_DIGITS = 4
MASK64 = (1 << 64) - 1
UNDECIDED = None


# ---- table ---------------------------------------------------------------------------------------
def pow5_entry(q):
    """(high, low) 64-bit words of the 128-bit approximation of 5^q, normalised to bit 127."""
    if q >= 0:
        p = 5 ** q
        b = p.bit_length()
        c = p << (128 - b) if b <= 128 else p >> (b - 128)
    else:
        p = 5 ** -q
        c = (1 << (p.bit_length() + 127)) // p + 1
        if c >> 128:
            c >>= 1
    assert c >> 127 == 1
    return c >> 64, c & MASK64


_TABLE = None


def pow5_table():
    global _TABLE
    if _TABLE is None:
        _TABLE = [pow5_entry(q) for q in range(Q_MIN, Q_MAX + 1)]
    return _TABLE


# ---- conversion ----------------------------------------------------------------------------------
def convert(w, q):
    """Bits of the double nearest w * 10^q (ties to even), sign excluded; None when undecided:
    the low-bits test fails, or the result is subnormal, zero by underflow, or overflows."""
    if w == 0:
        return 0
    if q < Q_MIN or q > Q_MAX:
        return UNDECIDED
    lz = 64 - w.bit_length()
    w <<= lz
    hi5, lo5 = pow5_table()[q - Q_MIN]
    first = w * hi5
    upper, lower = first >> 64, first & MASK64
    if upper & 0x1FF == 0x1FF:
        second_hi = (w * lo5) >> 64
        lower += second_hi
        if lower >> 64:
            lower &= MASK64
            upper += 1
        if lower == MASK64 and not -27 <= q <= 55:
            return UNDECIDED
    upperbit = upper >> 63
    shift = upperbit + 9
    mantissa = upper >> shift
    power2 = ((217706 * q) >> 16) + 1086 + upperbit - lz
    if power2 <= 0:
        return UNDECIDED
    if lower <= 1 and -4 <= q <= 23 and mantissa & 3 == 1 and (mantissa << shift) == upper:
        mantissa &= ~1   # exactly halfway: round to even
    mantissa += mantissa & 1
    mantissa >>= 1
    if mantissa >= 2 << 52:
        mantissa = 1 << 52
        power2 += 1
    mantissa &= ~(1 << 52)
    if power2 >= 0x7FF:
        return UNDECIDED
    return (power2 << 52) | mantissa


def scan_token(tok):
    """(negative, w, q, truncated) of a weight token — at most 19 significant digits in w, the
    rest dropped (``truncated``: one of them was not zero) — or None for a bad token."""
    if not 1 <= len(tok) <= MAX_TOKEN:
        return None
    i, n = 0, len(tok)
    neg = False
    if tok[i] in b'+-':
        neg = tok[i] == ord('-')
        i += 1
    w, nd, q, seen, truncated = 0, 0, 0, 0, False

    def digit(d, fraction):
        nonlocal w, nd, q, truncated
        if nd < 19:
            if nd or d:
                w = w * 10 + d
                nd += 1
            if fraction:
                q -= 1
        else:
            truncated = truncated or d != 0
            if not fraction:
                q += 1

    while i < n and tok[i] in ref.DIGITS:
        digit(tok[i] - 48, False)
        seen += 1
        i += 1
    if i < n and tok[i] == ord('.'):
        i += 1
        while i < n and tok[i] in ref.DIGITS:
            digit(tok[i] - 48, True)
            seen += 1
            i += 1
    if not seen:
        return None
    if i < n and tok[i] in b'eE':
        i += 1
        eneg = False
        if i < n and tok[i] in b'+-':
            eneg = tok[i] == ord('-')
            i += 1
        start, e = i, 0
        while i < n and tok[i] in ref.DIGITS:
            e = e * 10 + tok[i] - 48
            i += 1
        if not 1 <= i - start <= MAX_EXP_DIGITS:
            return None
        q += -e if eneg else e
    if i != n:
        return None
    return neg, w, q, truncated


BAD = 'bad'


def token_bits(tok):
    """BAD, None (undecided) or the 64 bits of the token's double."""
    s = scan_token(tok)
    if s is None:
        return BAD
    neg, w, q, truncated = s
    bits = convert(w, q)
    if bits is not None and truncated and convert(w + 1, q) != bits:
        bits = None
    if bits is None:
        return UNDECIDED
    return bits | (1 << 63 if neg else 0)


def float_bits(tok):
    return struct.unpack('<Q', struct.pack('<d', float(tok)))[0]


# ---- lines ---------------------------------------------------------------------------------------
def parse_line_weighted(line):
    """None for a skipped line, (u, v, token) for a data line, ValueError otherwise."""
    if line[-1:] == b'\r':
        line = line[:-1]
    q = 0
    while q < len(line) and line[q] in ref.BLANKS:
        q += 1
    if q == len(line) or line[q] in b'#%':
        return None
    fields = []
    for _ in range(2):
        number = ref._number(line, q)
        if number is None:
            raise ValueError('id')
        fields.append(number[0])
        q = number[1]
        if q == len(line) or line[q] not in ref.SEPARATORS:
            raise ValueError('separator')
        while q < len(line) and line[q] in ref.SEPARATORS:
            q += 1
    end = q
    while end < len(line) and line[end] not in ref.SEPARATORS:
        end += 1
    tok = line[q:end]
    if scan_token(tok) is None:
        raise ValueError('weight')
    return fields[0], fields[1], tok


def parse_text_weighted(data, skip_rows=0, refuse_infinite=True):
    """(src, dst, tokens, 0-based offsets of the tokens) of a whole file's bytes; BadLine carries
    the 1-based line number — of a bad line, or of a weight that is not finite (the reader's
    contract; the kernel on its own hands such a token over: ``refuse_infinite=False``)."""
    src, dst, toks, offs = [], [], [], []
    pos = 0
    lines = data.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    for k, line in enumerate(lines):
        if k >= skip_rows:
            try:
                e = parse_line_weighted(line)
            except ValueError:
                raise ref.BadLine(k + 1) from None
            if e is not None:
                if refuse_infinite and float(e[2]) in (float('inf'), float('-inf')):
                    raise ref.BadLine(k + 1)
                src.append(e[0])
                dst.append(e[1])
                toks.append(e[2])
                q = 0   # the token's offset: behind the second separator run
                while line[q] in ref.BLANKS:
                    q += 1
                for _ in range(2):
                    while line[q] in ref.DIGITS:
                        q += 1
                    while line[q] in ref.SEPARATORS:
                        q += 1
                offs.append(pos + q)
        pos += len(line) + 1
    return src, dst, toks, offs


# ---- corpora -------------------------------------------------------------------------------------
def _doubles_all_exponents(rng, n):
    expo = rng.integers(1, 2047, size=n, dtype=np.uint64)
    frac = rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    return ((expo << np.uint64(52)) | frac).view(np.float64)


def corpus(name, n, seed=0):
    """n tokens (bytes) of the named corpus, seeded."""
    rng = np.random.default_rng([seed, sorted(CORPORA).index(name)])
    if name == 'repr_unit':
        return [repr(x).encode() for x in (rng.random(n) + 0.5).tolist()]
    if name == 'repr_scaled':
        x = (rng.random(n) + 0.5) * np.where(rng.random(n) < 0.5, 1e8, 1e-8)
        return [repr(v).encode() for v in x.tolist()]
    if name == 'fixed':
        return [b'%.6f' % v for v in (rng.random(n) * 1000.0).tolist()]
    if name == 'integers':
        digits = rng.integers(1, 19, size=n)
        vals = rng.integers(0, 10 ** 18, size=n) % (10 ** digits)
        return [str(v).encode() for v in vals.tolist()]
    if name == 'normal_doubles':
        return [repr(v).encode() for v in _doubles_all_exponents(rng, n).tolist()]
    if name == 'scientific':
        out = []
        m = rng.integers(0, 10 ** 6, size=n).tolist()
        e = rng.integers(-30, 31, size=n).tolist()
        k = rng.integers(0, 4, size=n).tolist()
        for mi, ei, ki in zip(m, e, k):
            if ki == 0:
                out.append(b'%dE%+03d' % (mi % 10, ei))           # 1E+05
            elif ki == 1:
                out.append(b'%d.%de%d' % (mi // 1000, mi % 1000, ei))   # 2.5e-7
            elif ki == 2:
                out.append(b'%.3E' % (mi * 10.0 ** ei))
            else:
                out.append(b'.%de+%d' % (mi, abs(ei)))
        return out
    if name == 'forms':
        fixed = [b'-0', b'+0', b'0', b'-0.0', b'5.', b'.5', b'-.5', b'+5.', b'005', b'5.2500',
                 b'000.000', b'0e999', b'-0e-999', b'00001.50000e+0002', b'1e0', b'1E-0',
                 b'0.000000000000000000000000000001', b'100000000000000000000',
                 b'1.00000000000000000000000000', b'0' * 63 + b'7', b'9' * 64,
                 b'0.' + b'0' * 61 + b'1', b'1.7976931348623157e308', b'2.2250738585072014e-308']
        out = list(fixed)
        vals = (rng.random(n) * 100.0).tolist()
        k = rng.integers(0, 6, size=n).tolist()
        for v, ki in zip(vals, k):
            s = repr(v).encode()
            out.append([b'-' + s, b'+' + s, b'000' + s, s + b'000', b'-00' + s + b'0',
                        b'%d.' % int(v)][ki])
        return out[:max(n, len(fixed))]
    if name == 'digits25':
        hi = rng.integers(0, 10 ** 12, size=n).tolist()
        lo = rng.integers(0, 10 ** 13, size=n).tolist()
        lead = rng.integers(0, 100, size=n).tolist()
        return [b'%d.%012d%013d' % (a, h, l) for a, h, l in zip(lead, hi, lo)]
    if name == 'wq':
        digits = rng.integers(1, 20, size=n)
        w = [int(a) * 10 ** 10 + int(b) for a, b in
             zip(rng.integers(0, 10 ** 9, size=n), rng.integers(0, 10 ** 10, size=n))]
        q = rng.integers(-330, 301, size=n).tolist()
        return [b'%de%d' % (wi % 10 ** int(d), qi) for wi, d, qi in zip(w, digits.tolist(), q)]
    if name == 'midpoints':
        m = rng.integers(1 << 52, 1 << 53, size=n).tolist()
        # half of them below 2^63: all their digits fit w, and the tie is the method's to break
        e = np.where(rng.random(n) < 0.5, rng.integers(0, 10, size=n),
                     rng.integers(0, 150, size=n)).tolist()
        return [str((2 * mi + 1) << ei).encode() for mi, ei in zip(m, e)]
    raise KeyError(name)


CORPORA = {'repr_unit', 'repr_scaled', 'fixed', 'integers', 'normal_doubles', 'scientific',
           'forms', 'digits25', 'wq', 'midpoints'}
# undecided caps (conditions on the restatement): none at all on what files really hold
NO_UNDECIDED = ('repr_unit', 'repr_scaled', 'fixed', 'integers', 'normal_doubles')
DIGITS25_CAP = 0.01

BAD_TOKENS = [b'nan', b'NaN', b'inf', b'-inf', b'Infinity', b'INFINITY', b'0x1p3', b'0x10', b'1_0',
              b'1e', b'1e+', b'.', b'e5', b'1.2.3', b'--1', b'+-1', b'1.5x', b'+', b'-', b'1e5.0',
              b'1e12345', b'1E', b'1d5', b'1.e', b'0' * 65, b'1.' + b'0' * 63]
# (as the third field; a missing third field is bad too: BAD_LINES_WEIGHTED)
BAD_LINES_WEIGHTED = [b'1 2 ' + t for t in BAD_TOKENS] + [b'1 2', b'1 2 ', b'1,2,', b'1 2\t,',
                                                          b'-1 2 0.5', b'1 x 0.5']
OVERFLOW_TOKENS = [b'1e999', b'-1e999', b'1.8e308', b'1e309', b'9' * 19 + b'e290']

FORMAT_TEXT_WEIGHTED = (b'# a comment\n'
                        b'% another\n'
                        b'\n'
                        b'1 2 0.5\r\n'
                        b'  \t \n'
                        b'3\t4\t1.25e-3\n'
                        b'5,6,7\n'
                        b' \t 7 ,\t, 8 ,, -2.5\n'
                        b'0009 0010 0001.5000\n'
                        b'11 12 0.5 extra columns # here\n'
                        b'13,14,.25,\n'
                        b'   # indented comment\n'
                        b'\r\n'
                        b'100000000000000000 999999999999999999 1E+05\n'
                        b'2 1 -0\n'
                        b'1 3 4.9e-324\r\n'
                        b'15 15 3.')   # no final newline: the weight ends at the last byte
