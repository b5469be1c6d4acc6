"""CPU checks of the device R-MAT path's host half and of the graph references themselves:
the PCG64 jump table against numpy's own ``advance``, the Python-int PCG64 restatement against
``rng.random()``, ``graph_ref.rmat_unique`` against the product's numpy generator, and
``graph_ref.check_adj_hash`` against hand-corrupted tables (a checker that accepts everything
checks nothing)."""
import numpy as np
import pytest

import graph_ref as gr
from shallow_encoders.graph.rmat import _pcg_advance, _pcg_jump_table, rmat_edges

SEEDS = [0, 1, 12345]
ADVANCES = [0, 1, 15, 16, 17, 4099, 2 ** 31 - 1, 31 * (2 ** 31 - 1)]


@pytest.mark.parametrize('k', ADVANCES)
@pytest.mark.parametrize('seed', SEEDS)
def test_pcg_advance_equals_numpy_advance(seed, k):
    """_pcg_advance over _pcg_jump_table lands on the state numpy's bit_generator.advance(k)
    gives, and the restated output function turns that state into the next rng.random()."""
    s0, inc = gr.seed_state(seed)
    rng = np.random.default_rng(seed)
    rng.bit_generator.advance(k)
    st = rng.bit_generator.state['state']
    got = _pcg_advance(s0, k, _pcg_jump_table(inc))
    assert got == int(st['state']) and inc == int(st['inc'])
    nxt, after = gr.pcg64_doubles(got, inc, 1)
    assert nxt[0] == rng.random()
    assert after == int(rng.bit_generator.state['state']['state'])


@pytest.mark.parametrize('seed', SEEDS)
def test_pcg64_doubles_equal_numpy_stream(seed):
    s0, inc = gr.seed_state(seed)
    got, state = gr.pcg64_doubles(s0, inc, 4099)
    rng = np.random.default_rng(seed)
    np.testing.assert_array_equal(got, rng.random(4099))
    assert state == int(rng.bit_generator.state['state']['state'])
    assert state == _pcg_advance(s0, 4099, _pcg_jump_table(inc))


def test_jump_table_entries_are_powers_of_the_step():
    """Entry i is 2^i single steps (checked by stepping, for the entries a loop can reach)."""
    s0, inc = gr.seed_state(7)
    table = _pcg_jump_table(inc)
    assert len(table) == 64 and table[0] == (gr.PCG_MULT, inc)
    s, n = s0, 0
    for i in range(13):
        while n < (1 << i):
            s = (s * gr.PCG_MULT + inc) & gr.M128
            n += 1
        a, c = table[i]
        assert (a * s0 + c) & gr.M128 == s


@pytest.mark.parametrize('case', gr.RMAT_LATTICE, ids=gr.lattice_id)
def test_rmat_unique_equals_numpy_generator(case):
    """The Python-int draw and first-occurrence dedupe equal rmat_edges less its patch edges."""
    scale, n_edges, seed, abcd = case
    edges, n_patched = rmat_edges(scale, n_edges, seed, abcd)
    got = gr.rmat_unique(scale, n_edges, seed, abcd)
    m = len(got)
    ref = (edges[:m, 0].astype(np.uint64) << np.uint64(32)) | edges[:m, 1].astype(np.uint64)
    np.testing.assert_array_equal(got, ref)
    # what follows are the patch edges: one per isolated node, less mirrored pairs
    assert (n_patched + 1) // 2 <= len(edges) - m <= n_patched
    src, dst = gr.rmat_draws(scale, n_edges, seed, abcd)
    assert len(src) == len(dst) == n_edges and max(src + dst) < (1 << scale)


def test_rmat_unique_scale31_uses_the_high_bits():
    got = gr.rmat_unique(31, 1000, 0)
    assert len(got) == 1000   # no self-loop, no repeat at this size
    assert max(int(got.max() >> np.uint64(32)), int((got & np.uint64(0xFFFFFFFF)).max())) >= 2 ** 30


# ---- the adjacency-table checker must refuse a wrong table ----------------------------------------
def _host_tables(row_ptr, col):
    """Sequential insertion by the layout's rule: (off, tab, hpos)."""
    V = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([16 * gr.adj_buckets(int(d)) for d in deg], out=off[1:])
    tab = np.full(off[V], -1, dtype=np.int32)
    hpos = np.full(off[V], -1, dtype=np.int32)
    for u in range(V):
        nb = gr.adj_buckets(int(deg[u]))
        if nb == 0:
            continue
        for i, x in enumerate(col[row_ptr[u]:row_ptr[u + 1]].tolist()):
            bk = gr.adj_home(x, nb)
            for _ in range(nb):
                s0 = off[u] + 16 * bk
                free = np.flatnonzero(tab[s0:s0 + 16] < 0)
                if len(free):
                    tab[s0 + free[0]], hpos[s0 + free[0]] = x, i
                    break
                bk = (bk + 1) % nb
            else:
                raise AssertionError('a table at load <= 3/4 cannot be full')
    return off, tab, hpos


@pytest.fixture(scope='module')
def ladder_tables():
    row_ptr, col = gr.ladder_graph()
    return (row_ptr, col) + _host_tables(row_ptr, col)


def test_ladder_graph_shape():
    row_ptr, col = gr.ladder_graph()
    V = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    assert V % 32 == 1 and (col == V - 1).any()
    assert tuple(deg[:len(gr.RUNG_DEGREES)]) == gr.RUNG_DEGREES
    hub = col[row_ptr[13]:row_ptr[14]]
    assert {31, 32, 63, V - 1} <= set(hub.tolist())
    leaves = deg[len(gr.RUNG_DEGREES):]
    assert (leaves == 8).any() and (leaves == 9).any()
    assert gr.validate(row_ptr, col) and not gr.has_repeated_neighbour(row_ptr, col)
    # undirected: every entry has its mirror
    rows = np.repeat(np.arange(V), deg)
    fwd = set(zip(rows.tolist(), col.tolist()))
    assert fwd == {(v, u) for u, v in fwd}
    bad = col.copy()
    bad[row_ptr[2]] = bad[row_ptr[2] + 1]
    assert gr.has_repeated_neighbour(row_ptr, bad)
    for r in range(2, len(gr.RUNG_DEGREES)):   # every rung's list is out of order
        row = col[row_ptr[r]:row_ptr[r + 1]]
        assert (np.diff(row) < 0).any()


def test_check_adj_hash_accepts_sequential_insertion(ladder_tables):
    row_ptr, col, off, tab, hpos = ladder_tables
    gr.check_adj_hash(row_ptr, col, off, tab)
    gr.check_adj_hash(row_ptr, col, off, tab, hpos)
    nb = np.diff(off) // 16
    assert {1, 2, 3} <= set(nb.tolist())


def _row_slots(off, tab, u):
    t = tab[off[u]:off[u + 1]]
    return off[u] + np.flatnonzero(t >= 0), off[u] + np.flatnonzero(t < 0)


@pytest.mark.parametrize('rung', [5, 7])   # degree 13 (2 buckets) and 25 (3 buckets)
def test_check_adj_hash_rejects_moved_neighbour(ladder_tables, rung):
    row_ptr, col, off, tab, hpos = ladder_tables
    nb = (off[rung + 1] - off[rung]) // 16
    full, free = _row_slots(off, tab, rung)
    s = full[0]                                   # (load <= 3/4: its home bucket has free slots)
    home = (s - off[rung]) // 16
    assert gr.adj_home(int(tab[s]), nb) == home
    dest = [f for f in free if (f - off[rung]) // 16 == (home + 1) % nb][0]
    bad, bad_h = tab.copy(), hpos.copy()
    bad[dest], bad_h[dest] = bad[s], bad_h[s]
    bad[s], bad_h[s] = -1, -1
    with pytest.raises(AssertionError, match='behind a bucket with a free slot'):
        gr.check_adj_hash(row_ptr, col, off, bad, bad_h)


def test_check_adj_hash_rejects_duplicated_slot(ladder_tables):
    row_ptr, col, off, tab, hpos = ladder_tables
    full, free = _row_slots(off, tab, 7)
    bad = tab.copy()
    bad[free[0]] = bad[full[0]]
    with pytest.raises(AssertionError, match='each once'):
        gr.check_adj_hash(row_ptr, col, off, bad)


def test_check_adj_hash_rejects_shifted_hpos(ladder_tables):
    row_ptr, col, off, tab, hpos = ladder_tables
    full, _ = _row_slots(off, tab, 7)
    bad = hpos.copy()
    bad[full[3]] = (bad[full[3]] + 1) % 25
    gr.check_adj_hash(row_ptr, col, off, tab, hpos)
    with pytest.raises(AssertionError, match='hpos does not point at the key'):
        gr.check_adj_hash(row_ptr, col, off, tab, bad)
    bad = hpos.copy()
    _, free = _row_slots(off, tab, 7)
    bad[free[0]] = 0
    with pytest.raises(AssertionError, match='empty slot'):
        gr.check_adj_hash(row_ptr, col, off, tab, bad)


def test_check_adj_hash_rejects_wrong_table_size(ladder_tables):
    row_ptr, col, off, tab, hpos = ladder_tables
    bad = off.copy()
    bad[3:] += 16     # slots for the degree-8 rung
    with pytest.raises(AssertionError, match='slots'):
        gr.check_adj_hash(row_ptr, col, bad, np.concatenate([tab, np.full(16, -1, np.int32)]))
