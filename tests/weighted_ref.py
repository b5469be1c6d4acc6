"""A weighted hub graph, weight families and the alias-table mass check (TEST INFRASTRUCTURE).

The weighted walk paths (dw_alias_build, the weighted replay k_walk_replay<2048, 2048>, the
Philox walkers' first_order_pick over prob_thr / alias) are checked on ``hub_graph()``: the
smallest graph whose rows cross the constants those kernels branch on — DW_ADJ_HASH_MIN_DEG = 8,
the 64-lane wave, REPLAY_CH = REPLAY_NCAP = 2048 — with weights from ``sym_weights``. No GPU code
and no fixtures here; tests/test_weighted_oracle.py runs it on the CPU, tests/
test_gpu_walks_weighted.py against the kernels.
"""
import numpy as np

ALWAYS = 0xFFFFFFFF
N_LEAVES = 2500
N_MID = 8            # leaves 1..8 carry pendant nodes: rows of degree 65..2048
N_PENDANT = 300
HUB_ID = 1           # vocabulary ids (node i -> i + 1)
MID_IDS = tuple(range(2, 2 + N_MID))
FAMILIES = ('int', 'dyadic', 'zeros', 'skew', 'float')
# rows of degree <= 8, 9..64, 65..2048, > 2048 (the <unk> row 0, without neighbours, not counted)
DEGREE_CLASSES = (3548, 1344, 8, 1)

_CACHE = {}


def hub_graph():
    """Node 0 is a hub joined to the leaves 1..2500; 4 * 2500 distinct random chords among the
    leaves (default_rng(3), drawn as tests/test_gpu_walks._hub_graph draws them); each of the
    leaves 1..8 also has 300 pendant nodes of its own: 4,902 rows, 29,800 directed edges. Edge
    order: the hub's edges to the even leaves, the chords, the hub's edges to the odd leaves, the
    pendants — so an even leaf's row starts with the hub and ends with a chord, an odd leaf's
    starts with a chord and ends with the hub (the 'zeros' family then has rows with a zero weight
    first and rows with one last). Cached: the graph is shared by the tests and not changed."""
    if 'csr' in _CACHE:
        return _CACHE['csr']
    from shallow_encoders.graph.rmat import csr_from_edges
    rng = np.random.default_rng(3)
    n = N_LEAVES + 1
    chords = set()
    while len(chords) < 4 * N_LEAVES:
        u, v = rng.integers(1, n, size=2)
        if u != v:
            chords.add((min(u, v), max(u, v)))
    edges = [(0, i) for i in range(2, n, 2)]
    edges += sorted((int(u), int(v)) for u, v in chords)
    edges += [(0, i) for i in range(1, n, 2)]
    for k in range(N_MID):
        first = n + k * N_PENDANT
        edges += [(1 + k, first + j) for j in range(N_PENDANT)]
    n_nodes = n + N_MID * N_PENDANT
    csr = csr_from_edges(n_nodes, np.asarray(edges, dtype=np.int64))
    deg = np.diff(csr.row_ptr)[1:]
    assert csr.vocab_size == 4902 and csr.nnz == 29_800
    got = (int((deg <= 8).sum()), int(((deg > 8) & (deg <= 64)).sum()),
           int(((deg > 64) & (deg <= 2048)).sum()), int((deg > 2048).sum()))
    assert got == DEGREE_CLASSES, got
    assert deg[HUB_ID - 1] == N_LEAVES and all(64 < deg[m - 1] <= 2048 for m in MID_IDS)
    _CACHE['csr'] = csr
    return csr


def _pair_hash(lo, hi):
    """A fixed 64-bit mix of the unordered pair (splitmix64's finaliser)."""
    m = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over='ignore'):
        x = (lo.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             + hi.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
             + np.uint64(0x165667B19E3779F9)) & m
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & m
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & m
    return x ^ (x >> np.uint64(31))


def sym_weights(csr, family):
    """float64 weight per directed edge, a pure function of the unordered pair (min, max) of its
    ends, so both directions agree as in nx.Graph.

      'int'     integers 1..7
      'dyadic'  k / 8, k = 1..64
      'zeros'   integers 0..6; an edge touching the hub or a degree-1 node is raised by 1, so every
                row sums to more than 0 (about 10 % of the entries are 0)
      'skew'    1000.0 on about 2 % of the edges, 1..3 elsewhere
      'float'   0.05 + k / 7919: not representable in binary (the Philox walkers only)

    'int', 'dyadic' and 'zeros' keep every partial sum of a step's weights exact for (p, q) =
    (0.25, 4) and (2, 0.5) (random_walk_generator.sum_is_exact)."""
    rp = np.asarray(csr.row_ptr, dtype=np.int64)
    col = np.asarray(csr.host_col(), dtype=np.int64)
    deg = np.diff(rp)
    row = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    h = _pair_hash(np.minimum(row, col), np.maximum(row, col))
    if family == 'int':
        return (1 + (h % np.uint64(7))).astype(np.float64)
    if family == 'dyadic':
        return (1 + (h % np.uint64(64))).astype(np.float64) / 8.0
    if family == 'zeros':
        w = (h % np.uint64(7)).astype(np.float64)
        raised = (row == HUB_ID) | (col == HUB_ID) | (deg[row] == 1) | (deg[col] == 1)
        return w + raised
    if family == 'skew':
        heavy = (h % np.uint64(50)) == 0
        light = (1 + ((h // np.uint64(50)) % np.uint64(3))).astype(np.float64)
        return np.where(heavy, 1000.0, light)
    if family == 'float':
        return 0.05 + (h % np.uint64(7919)).astype(np.float64) / 7919.0
    raise ValueError(f'unknown weight family {family!r}')


def alias_mass_error(row_ptr, prob_thr, alias, weights):
    """How far the law an alias table samples is from the weights' law, in units of the
    truncation the table's format allows.

    For a row of n entries, column j is drawn with probability 1/n and keeps itself with
    pa_j (1 for ALWAYS, else thr_j / 2^32), so entry i is picked with
        mass_i = pa_i / n + sum over j with alias_j = i, thr_j != ALWAYS of (1 - pa_j) / n.
    The table floors pa_j to a multiple of 2^-32, so column j hands less than 2^-32 of its own
    mass to its alias and nothing else is lost: |mass_i - w_i / sum w| * n is at most
        bound_i = (1 + indeg_i) * 2^-32 + n * 2^-50
    (indeg_i: the non-ALWAYS columns whose alias is i; the second term: the build's fp64
    rounding, a few ulps per update of an entry's scaled weight, at most n updates).

    Returns (the worst |mass_i - w_i / sum w| * n / bound_i over every entry, the number of
    entries with w_i == 0 and mass_i != 0)."""
    rp = np.asarray(row_ptr, dtype=np.int64)
    deg = np.diff(rp)
    nnz = int(rp[-1])
    thr = np.asarray(prob_thr).view(np.uint32).astype(np.int64)[:nnz]
    al = np.asarray(alias, dtype=np.int64)[:nnz]
    w = np.asarray(weights, dtype=np.float64)[:nnz]
    row = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    n = deg[row].astype(np.float64)
    assert ((al >= 0) & (al < deg[row])).all(), 'an alias outside its row'
    keep = thr == ALWAYS
    pa = np.where(keep, 1.0, thr / 4294967296.0)
    target = rp[row] + al
    mass_n = pa.copy()                                   # n * mass
    np.add.at(mass_n, target[~keep], 1.0 - pa[~keep])
    indeg = np.bincount(target[~keep], minlength=nnz)
    total = np.zeros(len(deg))
    np.add.at(total, row, w)
    want_n = w * n / total[row]
    bound = (1.0 + indeg) * 2.0 ** -32 + n * 2.0 ** -50
    worst = float(np.max(np.abs(mass_n - want_n) / bound)) if nnz else 0.0
    return worst, int(((w == 0) & (mass_n != 0)).sum())
