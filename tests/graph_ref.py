"""Plain references for the graph-build kernels (dw_rmat.hip, dw_graph.hip, and the hub bitmap /
edge-inline kernels of dw_walk.hip): numpy and Python ints only, no torch, no native library.

Test infrastructure. Everything here is exact (integers and bit patterns).
"""
import numpy as np

PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
M128 = (1 << 128) - 1
M64 = (1 << 64) - 1
RMAT_ABCD = (0.57, 0.19, 0.19, 0.05)   # (the product's default, restated)


# ---- numpy's PCG64, restated on Python ints -------------------------------------------------------
def pcg64_doubles(state: int, inc: int, k: int):
    """The next ``k`` doubles of numpy's PCG64 from ``(state, inc)``: ``(float64[k], new state)``.
    Per draw: state = state * M + inc (mod 2^128), out = XSL-RR of the NEW state (the xor of its
    halves rotated right by its top 6 bits), double = (out >> 11) * 2^-53."""
    out = np.empty(k, dtype=np.float64)
    for i in range(k):
        state = (state * PCG_MULT + inc) & M128
        hi, lo = state >> 64, state & M64
        x, r = hi ^ lo, hi >> 58
        o = ((x >> r) | (x << ((64 - r) & 63))) & M64
        out[i] = (o >> 11) * 2.0 ** -53
    return out, state


def seed_state(seed: int):
    """(state, inc) of ``numpy.random.default_rng(seed)`` (the seeding itself is numpy's)."""
    st = np.random.default_rng(seed).bit_generator.state['state']
    return int(st['state']), int(st['inc'])


# ---- R-MAT ---------------------------------------------------------------------------------------
def rmat_draws(scale: int, n_edges: int, seed: int, abcd=RMAT_ABCD):
    """The raw ``(src, dst)`` (Python-int lists) of every draw, before self-loop removal and
    dedupe: level-major uniforms (draw ``l * n_edges + e`` is edge e's level-l uniform), most
    significant bit first; src |= (r >= a+b), dst |= (a <= r < a+b) | (r >= a+b+c)."""
    a, b, c, _ = abcd
    t1, t2, t3 = a, a + b, a + b + c
    state, inc = seed_state(seed)
    src, dst = [0] * n_edges, [0] * n_edges
    for level in range(scale):
        r, state = pcg64_doubles(state, inc, n_edges)
        bit = 1 << (scale - 1 - level)
        for e, x in enumerate(r.tolist()):
            if x >= t2:
                src[e] |= bit
            if (t1 <= x < t2) or x >= t3:
                dst[e] |= bit
    return src, dst


def rmat_unique(scale: int, n_edges: int, seed: int, abcd=RMAT_ABCD) -> np.ndarray:
    """uint64 packed ``u << 32 | v`` of the kept draws in draw order: self-loops dropped, of every
    undirected edge the FIRST draw kept (in its drawn direction). Works up to scale 31."""
    src, dst = rmat_draws(scale, n_edges, seed, abcd)
    seen, kept = set(), []
    for u, v in zip(src, dst):
        if u == v:
            continue
        key = (u, v) if u < v else (v, u)
        if key in seen:
            continue
        seen.add(key)
        kept.append((u << 32) | v)
    return np.array(kept, dtype=np.uint64)


# (scale, n_edges, seed, abcd): the small awkward shapes of the R-MAT pipeline
Q = (0.25, 0.25, 0.25, 0.25)
RMAT_LATTICE = [
    (1, 1, 0, RMAT_ABCD),             # smallest everything
    (1, 17, 0, RMAT_ABCD),            # 17 draws, 1 edge; the second thread holds one draw
    (3, 15, 0, (1.0, 0.0, 0.0, 0.0)),  # every draw (0, 0): 0 kept, all nodes isolated
    (3, 33, 0, (0.0, 1.0, 0.0, 0.0)),  # every draw (0, 7): exactly 1 kept, draw 0
    (3, 33, 0, (0.0, 0.0, 0.0, 1.0)),  # every draw (7, 7): 0 kept
    (5, 4095, 3, Q),                  # one block of 256 x 16 draws, minus 1
    (5, 4096, 3, Q),                  # exactly one block; dense dedupe, no isolated node
    (5, 4097, 3, Q),                  # one block plus 1
    (10, 4099, 7, RMAT_ABCD),         # another PCG stream (inc); isolated nodes to patch
    (12, 40_001, 0, RMAT_ABCD),       # the walk fixtures' graph size, off the multiple of 16
]


def lattice_id(case) -> str:
    scale, n_edges, seed, abcd = case
    name = 'default' if abcd == RMAT_ABCD else '-'.join(f'{x:g}' for x in abcd)
    return f's{scale}-e{n_edges}-seed{seed}-{name}'


# ---- the ladder graph ------------------------------------------------------------------------------
RUNG_DEGREES = (0, 1, 8, 9, 12, 13, 24, 25, 63, 64, 65, 128, 129, 1025)


def ladder_graph():
    """A bipartite CSR ``(row_ptr int64[V+1], col int32[nnz])`` whose degrees sit on the kernels'
    thresholds. Rows 0..13 are the rungs, of degrees RUNG_DEGREES (row 0, the vocabulary's
    ``<unk>``, has none); rung i is joined to the first deg_i leaves, listed in a shuffled,
    non-ascending order. Leaf j < 1024 is row 14 + j; the last used leaf (j = 1024) is row
    V - 1 = 1056 and rows 1038..1055 are empty, so V = 1057 = 1 (mod 32) with V - 1 a neighbour
    of the longest rung, as are ids 31, 32 and 63. A leaf lists the rungs that reach it in
    descending order: leaf 0 has 13 neighbours, leaf 12 has 9, leaves 13..23 have 8."""
    n_rungs, n_leaves = len(RUNG_DEGREES), max(RUNG_DEGREES)
    V = 1057
    leaf_id = np.arange(n_rungs, n_rungs + n_leaves, dtype=np.int64)
    leaf_id[-1] = V - 1
    rng = np.random.default_rng(2024)
    rows = [[] for _ in range(V)]
    for i, deg in enumerate(RUNG_DEGREES):
        nbrs = leaf_id[:deg][rng.permutation(deg)]
        if deg > 1:
            assert (np.diff(nbrs) < 0).any(), 'a rung must not list its leaves ascending'
        rows[i] = nbrs.tolist()
    for j in range(n_leaves):
        rows[leaf_id[j]] = [i for i in range(n_rungs - 1, -1, -1) if RUNG_DEGREES[i] > j]
    row_ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    col = np.array([x for r in rows for x in r], dtype=np.int32)
    return row_ptr, col


# ---- CSR utilities ---------------------------------------------------------------------------------
def validate(row_ptr, col) -> bool:
    """dw_csr_validate's rule: row_ptr starts at 0, ends at nnz, never descends; 0 <= col < V."""
    row_ptr, col = np.asarray(row_ptr), np.asarray(col)
    V = len(row_ptr) - 1
    return bool(row_ptr[0] == 0 and row_ptr[V] == len(col) and (np.diff(row_ptr) >= 0).all()
                and (col >= 0).all() and (col < V).all())


def rows_sorted(row_ptr, col) -> np.ndarray:
    """``col`` with every row ascending (dw_csr_sort_copy)."""
    out = np.array(col, dtype=np.int32)
    for r in range(len(row_ptr) - 1):
        out[row_ptr[r]:row_ptr[r + 1]].sort()
    return out


def has_repeated_neighbour(row_ptr, col) -> bool:
    """Whether some row lists an id twice (dw_csr_check_simple over the sorted copy)."""
    for r in range(len(row_ptr) - 1):
        row = col[row_ptr[r]:row_ptr[r + 1]]
        if len(set(row.tolist())) != len(row):
            return True
    return False


def hub_bits(row_ptr, col, rows, words: int) -> np.ndarray:
    """uint32[len(rows), words]: bit ``x & 31`` (little-endian) of word ``x >> 5`` of row k is
    set iff x is a neighbour of ``rows[k]`` (dw_hub_bitmaps)."""
    out = np.zeros((len(rows), words), dtype=np.uint32)
    for k, r in enumerate(rows):
        for x in col[row_ptr[r]:row_ptr[r + 1]].tolist():
            out[k, x >> 5] |= np.uint32(1 << (x & 31))
    return out


def edges_inline(row_ptr, col) -> np.ndarray:
    """int32[nnz, 4]: {x, deg(x), row_ptr[x] low word, high word} per entry x = col[e]
    (dw_edges_inline_build)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    x = np.asarray(col, dtype=np.int64)
    a = row_ptr[x]
    out = np.empty((len(x), 4), dtype=np.int32)
    out[:, 0] = x
    out[:, 1] = row_ptr[x + 1] - a
    out[:, 2] = (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    out[:, 3] = a >> 32
    return out


def adj_buckets(deg: int) -> int:
    """Buckets (of 16 slots) of a row's adjacency hash: none up to degree 8, else load <= 3/4."""
    return (4 * deg + 47) // 48 if deg > 8 else 0


def adj_home(x: int, nb: int) -> int:
    return ((((x & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) * nb) >> 32


def check_adj_hash(row_ptr, col, off, tab, hpos=None) -> None:
    """Assert the adjacency hash layout's specification (not one insertion order: slot order
    under atomicCAS is not deterministic):
      * row u owns 16 * adj_buckets(deg) slots at off[u] (none up to degree 8), off[0] == 0;
      * the non-empty (>= 0) slots of a row are exactly its neighbours, each once;
      * every neighbour is reached from its home bucket by cyclic bucket steps without first
        passing a bucket that has a free slot;
      * with ``hpos``: col[row_ptr[u] + hpos[s]] == tab[s] on full slots, hpos[s] == -1 on empty."""
    V = len(row_ptr) - 1
    assert len(off) == V + 1 and off[0] == 0
    for u in range(V):
        a, b = int(row_ptr[u]), int(row_ptr[u + 1])
        nb = adj_buckets(b - a)
        assert off[u + 1] - off[u] == 16 * nb, f'row {u}: {off[u + 1] - off[u]} slots, nb {nb}'
        if nb == 0:
            continue
        t = np.asarray(tab[off[u]:off[u + 1]])
        nbrs = col[a:b]
        full = t[t >= 0]
        assert (t[t < 0] == -1).all(), f'row {u}: an empty slot is not -1'
        assert len(full) == len(nbrs) and np.array_equal(np.sort(full), np.sort(nbrs)), \
            f'row {u}: the full slots are not the neighbours, each once'
        buckets = t.reshape(nb, 16)
        free = (buckets < 0).any(axis=1)
        for x in nbrs.tolist():
            bk = adj_home(x, nb)
            for _ in range(nb):
                if (buckets[bk] == x).any():
                    break
                assert not free[bk], f'row {u}: neighbour {x} sits behind a bucket with a free slot'
                bk = (bk + 1) % nb
            else:
                raise AssertionError(f'row {u}: neighbour {x} not found')
        if hpos is not None:
            h = np.asarray(hpos[off[u]:off[u + 1]])
            assert (h[t < 0] == -1).all(), f'row {u}: hpos of an empty slot is not -1'
            hf = h[t >= 0]
            assert ((hf >= 0) & (hf < b - a)).all(), f'row {u}: hpos out of the row'
            assert np.array_equal(col[a + hf], full), f'row {u}: hpos does not point at the key'
