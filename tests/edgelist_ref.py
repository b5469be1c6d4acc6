"""Restatement of the edge-list contract (shallow_encoders/graph/edge_list.py), written
independently of the product's host path — test infrastructure:

  * ``parse_text``: a pure-Python, byte-at-a-time line parser for the text format;
  * ``networkx_csr``: literally ``nx.Graph().add_edges_from`` / ``add_weighted_edges_from`` over
    the zero-padded names, then ``CSRGraph.from_networkx``.
"""
import numpy as np

BLANKS = b' \t'
SEPARATORS = b' \t,'
DIGITS = b'0123456789'


class BadLine(ValueError):
    def __init__(self, line_no):
        super().__init__(f'line {line_no}')
        self.line_no = line_no


def _number(line, q):
    """(value, position behind it) of the 1-18 digits at q, or None."""
    start = q
    while q < len(line) and line[q] in DIGITS:
        q += 1
    if not 1 <= q - start <= 18:
        return None
    return int(line[start:q]), q


def parse_line(line):
    """None for a skipped line, (u, v) for a data line, ValueError otherwise. ``line`` is the
    line's bytes without its '\\n'."""
    if line[-1:] == b'\r':
        line = line[:-1]
    q = 0
    while q < len(line) and line[q] in BLANKS:
        q += 1
    if q == len(line) or line[q] in b'#%':
        return None
    first = _number(line, q)
    if first is None:
        raise ValueError('first field')
    u, q = first
    if q == len(line) or line[q] not in SEPARATORS:
        raise ValueError('separator')
    while q < len(line) and line[q] in SEPARATORS:
        q += 1
    second = _number(line, q)
    if second is None:
        raise ValueError('second field')
    v, q = second
    if q < len(line) and line[q] not in SEPARATORS:
        raise ValueError('behind the second field')
    return u, v


def parse_text(data, skip_rows=0):
    """(src, dst) lists of a whole file's bytes; BadLine carries the 1-based line number."""
    lines = data.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    src, dst = [], []
    for k, line in enumerate(lines):
        if k < skip_rows:
            continue
        try:
            e = parse_line(line)
        except ValueError:
            raise BadLine(k + 1) from None
        if e is not None:
            src.append(e[0])
            dst.append(e[1])
    return src, dst


def networkx_csr(src, dst, weights=None):
    import networkx as nx

    from shallow_encoders.graph.csr import CSRGraph
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    width = max(7, len(str(max(src + dst))))
    name = lambda x: f'n{x:0{width}d}'   # noqa: E731
    g = nx.Graph()
    if weights is None:
        g.add_edges_from((name(u), name(v)) for u, v in zip(src, dst))
    else:
        g.add_weighted_edges_from((name(u), name(v), float(w))
                                  for u, v, w in zip(src, dst, weights))
    return CSRGraph.from_networkx(g)


def assert_same_graph(got, want):
    """row_ptr, col, weights and itos equal, exactly (``got`` may be device-built)."""
    np.testing.assert_array_equal(got.row_ptr, want.row_ptr)
    np.testing.assert_array_equal(got.host_col(), want.host_col())
    assert got.host_col().dtype == np.int32 and got.row_ptr.dtype == np.int64
    assert got.weighted == want.weighted
    if want.weighted:
        assert got.weights.dtype == np.float64
        np.testing.assert_array_equal(got.weights, want.weights)
    else:
        assert got.weights is None
    assert list(got.itos) == list(want.itos)


# ---- the inputs both test files use ----------------------------------------------------------
def karate_edges():
    import networkx as nx
    e = np.array(list(nx.karate_club_graph().edges()), dtype=np.int64)
    return e[:, 0], e[:, 1], None


def sparse_weighted_edges():
    """60 weighted edges over 10 sparse ids up to 10^17, with duplicates in both orientations
    and repeated self-loops."""
    rng = np.random.default_rng(7)
    ids = np.sort(rng.integers(0, 10 ** 17, size=10))
    ids[0], ids[-1] = 3, 10 ** 17   # a small id and the 18-digit maximum of the draw
    src = ids[rng.integers(0, 10, size=60)]
    dst = ids[rng.integers(0, 10, size=60)]
    src[50:55], dst[50:55] = dst[10:15].copy(), src[10:15].copy()   # reversed repeats
    src[55:58], dst[55:58] = ids[4], ids[4]                          # a self-loop, three times
    w = rng.random(60) + 0.5
    return src, dst, w


def rmat10_doubled():
    from shallow_encoders.graph.rmat import rmat_edges
    e, _ = rmat_edges(10, 4000, seed=3)
    rng = np.random.default_rng(11)
    e = np.concatenate([e, e[:, ::-1]], axis=0)[rng.permutation(2 * len(e))]
    return e[:, 0].copy(), e[:, 1].copy(), None


ARRAY_CASES = {
    'karate': karate_edges,
    'sparse_weighted': sparse_weighted_edges,
    'single_edge': lambda: (np.array([5]), np.array([2]), None),
    'single_loop': lambda: (np.array([9]), np.array([9]), np.array([2.5])),
    'rmat10_doubled': rmat10_doubled,
}

FORMAT_TEXT = (b'# a comment\n'
               b'% another\n'
               b'\n'
               b'1 2\r\n'
               b'  \t \n'
               b'3\t4\n'
               b'5,6\n'
               b' \t 7 ,\t, 8\n'
               b'0009 0010\n'
               b'11 12 0.5 extra columns # here\n'
               b'13,14,\n'
               b'   # indented comment\n'
               b'\r\n'
               b'100000000000000000 999999999999999999\n'
               b'2 1\n'
               b'15 15')   # no final newline

BAD_LINES = [b'-1 2', b'1234567890123456789 1', b'7', b'a b']
