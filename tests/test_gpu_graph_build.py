"""The graph-build kernels against the plain references of tests/graph_ref.py at small edge
shapes: the R-MAT draw / dedupe / isolated list / CSR build (dw_rmat.hip), the CSR checks, sorted
copy, adjacency hash and its positions (dw_graph.hip), and the hub bitmaps and edge-inline
entries (dw_walk.hip). Every comparison is exact; every case is a few thousand edges at most."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import graph_ref as gr
from shallow_encoders import _native
from shallow_encoders.graph.csr import CSRGraph
from shallow_encoders.graph.rmat import (_rmat_edges_device, csr_from_edges, rmat_edges,
                                         rmat_graph)

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)   # (a copy: fixtures are read-only)


def _pack(edges) -> np.ndarray:
    e = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    return ((e[:, 0] << np.uint64(32)) | e[:, 1]).view(np.int64)


# ---- R-MAT: the full pipeline ----------------------------------------------------------------------
@pytest.mark.parametrize('case', gr.RMAT_LATTICE, ids=gr.lattice_id)
def test_rmat_pipeline_equals_host_build(case, hip_device):
    """dw_rmat_edges -> dw_graph_isolated -> host patch draws -> dw_csr_from_edges equals the
    numpy generator's CSR: tail threads, one block +-1, the degenerate dedupes (0 or 1 kept),
    another PCG stream, other thresholds."""
    scale, n_edges, seed, abcd = case
    edges, n_patched = rmat_edges(scale, n_edges, seed, abcd)
    host = csr_from_edges(1 << scale, edges)
    dev = rmat_graph(scale, n_edges, seed, device=hip_device, abcd=abcd)
    np.testing.assert_array_equal(dev.row_ptr, host.row_ptr)
    np.testing.assert_array_equal(dev.host_col(), host.col)
    assert len(dev.itos) == len(host.itos) == (1 << scale) + 1
    # the case reaches what it is there for
    kept = _n_unique(case)
    assert (n_patched + 1) // 2 <= len(edges) - kept <= n_patched
    if abcd in ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)):
        assert kept == 0 and n_patched == 1 << scale
    elif abcd == (0.0, 1.0, 0.0, 0.0):
        assert kept == 1 and tuple(edges[0]) == (0, 7)
    elif abcd == gr.Q:
        assert n_patched == 0 and kept <= 496 < n_edges // 4
    elif scale == 10:
        assert n_patched > 0


@functools.lru_cache(maxsize=None)
def _unique(case):
    return gr.rmat_unique(*case)


def _n_unique(case) -> int:
    return len(_unique(case))


SCALE31 = (31, 1000, 0, gr.RMAT_ABCD)


@pytest.mark.parametrize('case', gr.RMAT_LATTICE + [SCALE31], ids=gr.lattice_id)
def test_rmat_draw_and_dedupe_equal_reference(case, hip_device):
    """The draw and dedupe step alone: the packed kept edges, in draw order, equal the Python-int
    restatement. At scale 31 the sort keys use their whole 63-bit range."""
    scale, n_edges, seed, abcd = case
    # a workspace that is not zero, so a draw left unwritten is an edge, not a dropped (0, 0)
    nbytes = ctypes.c_size_t(0)
    _native.call('dw_ingest_workspace_bytes', scale, n_edges, 1, ctypes.byref(nbytes))
    ws = (torch.arange(int(nbytes.value), device=hip_device) % 251).to(torch.uint8)
    edges, m, rng = _rmat_edges_device(scale, n_edges, seed, abcd, hip_device, ws=ws)
    ref = _unique(case)
    assert m == len(ref)
    np.testing.assert_array_equal(edges[:m].cpu().numpy().view(np.uint64), ref)
    if scale == 31:
        ends = np.concatenate([ref >> np.uint64(32), ref & np.uint64(0xFFFFFFFF)])
        assert ends.max() >= 2 ** 30 and m == n_edges
    # the generator handed back stands past the edge draws
    ref_rng = np.random.default_rng(seed)
    ref_rng.bit_generator.advance(scale * n_edges)
    assert rng.bit_generator.state == ref_rng.bit_generator.state


# ---- dw_graph_isolated / dw_csr_from_edges, called directly -----------------------------------------
def _workspace(n_edges, n_nodes, dev):
    nbytes = ctypes.c_size_t(0)
    _native.call('dw_ingest_workspace_bytes', 1, max(n_edges, 1), n_nodes, ctypes.byref(nbytes))
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)


def _isolated(edges, n_nodes, dev):
    packed = _dev(_pack(edges), dev) if len(edges) else torch.empty(1, dtype=torch.int64,
                                                                    device=dev)
    ws = _workspace(len(edges), n_nodes, dev)
    iso = torch.full((n_nodes,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call('dw_graph_isolated', _native.ptr(packed), len(edges), n_nodes, _native.ptr(iso),
                 _native.ptr(count), _native.ptr(status), _native.ptr(ws), ws.numel(),
                 _native.stream(dev))
    k = int(count[0])
    return iso[:max(k, 0)].cpu().numpy(), k, int(status[0])


def _isolated_case(n, which):
    """Edges over n nodes that leave exactly the wanted nodes without one. Where a loop-free list
    cannot (n = 1, or one of two nodes), the others get a self-loop: the entry point counts both
    ends of every edge it is given."""
    want = {'first': {0}, 'last': {n - 1}, 'none': set(), 'all': set(range(n))}[which]
    rest = [u for u in range(n) if u not in want]
    if len(rest) == 1:
        edges = [(rest[0], rest[0])]
    else:   # a path through the rest, listed from its far end, directions alternating
        edges = [(a, b) if i % 2 else (b, a)
                 for i, (a, b) in enumerate(zip(rest[::-1][:-1], rest[::-1][1:]))]
    return edges, sorted(want)


@pytest.mark.parametrize('which', ['first', 'last', 'none', 'all'])
@pytest.mark.parametrize('n', [1, 2, 33])
def test_graph_isolated_direct(n, which, hip_device):
    edges, want = _isolated_case(n, which)
    iso, k, status = _isolated(edges, n, hip_device)
    assert status == 0 and k == len(want)
    np.testing.assert_array_equal(iso, want)


def _csr_direct(edges, n_nodes, dev):
    m = len(edges)
    packed = _dev(_pack(edges), dev) if m else torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(m, n_nodes, dev)
    row_ptr = torch.full((n_nodes + 2,), -7, dtype=torch.int64, device=dev)
    col = torch.full((max(2 * m, 1),), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call('dw_csr_from_edges', _native.ptr(packed), m, n_nodes, _native.ptr(row_ptr),
                 _native.ptr(col), _native.ptr(status), _native.ptr(ws), ws.numel(),
                 _native.stream(dev))
    return row_ptr.cpu().numpy(), col[:2 * m].cpu().numpy(), int(status[0])


def _csr_rows_reference(edges, n_nodes):
    """Rows in edge-list order: edge (u, v) appends v + 1 to row u + 1, then u + 1 to row v + 1."""
    rows = [[] for _ in range(n_nodes + 1)]
    for u, v in edges:
        rows[u + 1].append(v + 1)
        rows[v + 1].append(u + 1)
    row_ptr = np.zeros(n_nodes + 2, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    return row_ptr, np.array([x for r in rows for x in r], dtype=np.int32)


def _fan(n):
    """Many edges on node 0 (and on node n - 1), the other endpoint descending and the direction
    alternating: an unstable sort, or one that drops a key bit, lists a row in another order."""
    edges = [(0, v) if v % 2 else (v, 0) for v in range(n - 1, 0, -1)]
    edges += [(n - 1, v) if v % 3 else (v, n - 1) for v in range(n - 2, 0, -1)]
    return edges


CSR_DIRECT = {
    'n1-empty': (1, []), 'n2-empty': (2, []), 'n33-empty': (33, []),
    'n2-one': (2, [(1, 0)]),
    'n32-fan': (32, _fan(32)), 'n33-fan': (33, _fan(33)),
    'n64-fan': (64, _fan(64)), 'n65-fan': (65, _fan(65)),
}


@pytest.mark.parametrize('name', list(CSR_DIRECT))
def test_csr_from_edges_direct(name, hip_device):
    """n_edges = 0 gives an all-zero row_ptr; rows keep edge-list order on both sides of a power
    of two (the sort's bit count)."""
    n, edges = CSR_DIRECT[name]
    row_ptr, col, status = _csr_direct(edges, n, hip_device)
    ref_ptr, ref_col = _csr_rows_reference(edges, n)
    assert status == 0
    np.testing.assert_array_equal(row_ptr, ref_ptr)
    np.testing.assert_array_equal(col, ref_col)
    if not edges:
        assert not row_ptr.any()
    else:   # the product's own host build says the same
        host = csr_from_edges(n, np.asarray(edges, dtype=np.int64))
        np.testing.assert_array_equal(row_ptr, host.row_ptr)
        np.testing.assert_array_equal(col, host.col)


@pytest.mark.parametrize('half', ['src', 'dst'])
@pytest.mark.parametrize('entry', ['dw_graph_isolated', 'dw_csr_from_edges'])
def test_endpoint_out_of_range_sets_bad_csr(entry, half, hip_device):
    """An endpoint equal to n_nodes sets DW_S_BAD_CSR; the call itself returns DW_OK."""
    n = 33
    edges = [(0, 1), (2, 32), (n, 5) if half == 'src' else (5, n), (7, 8)]
    if entry == 'dw_graph_isolated':
        status = _isolated(edges, n, hip_device)[2]
    else:
        status = _csr_direct(edges, n, hip_device)[2]
    assert status == _native.DW_S_BAD_CSR
    ok = [e for e in edges if max(e) < n]
    assert (_isolated(ok, n, hip_device)[2], _csr_direct(ok, n, hip_device)[2]) == (0, 0)


# ---- CSR utilities on the ladder graph ---------------------------------------------------------------
@pytest.fixture(scope='module')
def ladder():
    row_ptr, col = gr.ladder_graph()
    row_ptr.setflags(write=False)
    col.setflags(write=False)
    return row_ptr, col


def _validate_status(row_ptr, col, dev) -> int:
    rp, c = _dev(row_ptr, dev), _dev(col, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call('dw_csr_validate', _native.ptr(rp), _native.ptr(c), len(row_ptr) - 1, len(col),
                 _native.ptr(status), _native.stream(dev))
    return int(status[0])


def _malformed(row_ptr, col, how):
    row_ptr, col = row_ptr.copy(), col.copy()
    V, nnz = len(row_ptr) - 1, len(col)
    if how == 'head':
        row_ptr[0] = row_ptr[1] = 1  # (row 0 is empty: moved with it, nothing descends)
    elif how == 'tail':
        row_ptr[V] = nnz - 1        # (the last row has one entry: still not descending)
    elif how == 'descending':
        row_ptr[V // 2] = row_ptr[V // 2 + 1] + 1
    elif how == 'col_negative':
        col[nnz // 2] = -1
    elif how == 'col_V':
        col[nnz // 2] = V
    return row_ptr, col


MALFORMED = ['head', 'tail', 'descending', 'col_negative', 'col_V']


def test_csr_validate_accepts_ladder(ladder, hip_device):
    assert gr.validate(*ladder)
    assert _validate_status(*ladder, hip_device) == 0


@pytest.mark.parametrize('how', MALFORMED)
def test_csr_validate_refuses(how, ladder, hip_device):
    row_ptr, col = _malformed(*ladder, how)
    assert not gr.validate(row_ptr, col)
    # exactly one rule is broken
    d = np.diff(row_ptr)
    broken = [row_ptr[0] != 0, row_ptr[-1] != len(col), (d < 0).any(), (col < 0).any(),
              (col >= len(row_ptr) - 1).any()]
    assert sum(bool(b) for b in broken) == 1
    assert _validate_status(row_ptr, col, hip_device) == _native.DW_S_BAD_CSR


@pytest.mark.parametrize('how', MALFORMED)
def test_csr_graph_refuses_malformed_arrays(how, ladder, hip_device):
    row_ptr, col = _malformed(*ladder, how)
    with pytest.raises(ValueError, match='malformed CSR'):
        CSRGraph.from_arrays(row_ptr, col).device_tensors(hip_device)


def _sort_copy(row_ptr, col, dev):
    """(col_sorted, DW_S_* of dw_csr_check_simple), both entry points called directly."""
    rp, c = _dev(row_ptr, dev), _dev(col, dev)
    V, nnz = len(row_ptr) - 1, len(col)
    out = torch.full((nnz,), -7, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t(0)
    s = _native.stream(dev)
    _native.call('dw_csr_sort_copy', _native.ptr(rp), _native.ptr(c), V, nnz, _native.ptr(out),
                 None, ctypes.byref(nbytes), s)
    tmp = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=dev)
    _native.call('dw_csr_sort_copy', _native.ptr(rp), _native.ptr(c), V, nnz, _native.ptr(out),
                 _native.ptr(tmp), ctypes.byref(nbytes), s)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call('dw_csr_check_simple', _native.ptr(rp), _native.ptr(out), V, nnz,
                 _native.ptr(status), s)
    return out.cpu().numpy(), int(status[0])


def test_sort_copy_and_simple_check_on_ladder(ladder, hip_device):
    row_ptr, col = ladder
    got, status = _sort_copy(row_ptr, col, hip_device)
    ref = gr.rows_sorted(row_ptr, col)
    assert not np.array_equal(ref, col)
    np.testing.assert_array_equal(got, ref)
    assert status == 0 and not gr.has_repeated_neighbour(row_ptr, col)


def test_simple_check_ignores_equal_ids_across_a_row_boundary(ladder, hip_device):
    """Row r ends and row r + 1 begins with the same id (sorted): not a repeated neighbour."""
    row_ptr, col = ladder
    ref = gr.rows_sorted(row_ptr, col)
    a = row_ptr[2]              # rung 1 is {first leaf}; rung 2's sorted row starts with it
    assert row_ptr[1] < a < row_ptr[3] and ref[a - 1] == ref[a]
    # and with nothing else in the graph: rows {5, 7}, {7, 9}, {7}, {}, {7, 8}
    rp = np.array([0, 2, 4, 5, 5, 7, 7, 7, 7, 7, 7], dtype=np.int64)
    c = np.array([7, 5, 9, 7, 7, 8, 7], dtype=np.int32)
    got, status = _sort_copy(rp, c, hip_device)
    np.testing.assert_array_equal(got, [5, 7, 7, 9, 7, 7, 8])
    assert status == 0
    assert _sort_copy(row_ptr, col, hip_device)[1] == 0


def _with_repeat(row_ptr, col, where):
    row_ptr, col = row_ptr.copy(), col.copy()
    if where == 'last_row':     # the last row (one entry) lists its neighbour twice
        row_ptr[-1] += 1
        return row_ptr, np.append(col, col[-1])
    p = int(where)
    r = 11                      # the rung of degree 128: two passes of the 64 lanes
    a, b = row_ptr[r], row_ptr[r + 1]
    s = np.sort(col[a:b])
    col[a + np.flatnonzero(col[a:b] == s[p + 1])[0]] = s[p]   # sorted positions p, p + 1 equal
    return row_ptr, col


@pytest.mark.parametrize('where', ['0', '63', '64', 'last_row'])
def test_simple_check_flags_one_repeat(where, ladder, hip_device):
    row_ptr, col = _with_repeat(*ladder, where)
    assert gr.has_repeated_neighbour(row_ptr, col)
    ref = gr.rows_sorted(row_ptr, col)
    if where != 'last_row':
        a = row_ptr[11]
        assert ref[a + int(where)] == ref[a + int(where) + 1]
    got, status = _sort_copy(row_ptr, col, hip_device)
    np.testing.assert_array_equal(got, ref)
    assert status == _native.DW_S_DUP_NEIGHBOR


def test_adjacency_hash_and_positions_on_ladder(ladder, hip_device):
    """Degrees exactly at 8|9 (hash or not) and 12|13, 24|25 (1 -> 2 -> 3 buckets)."""
    row_ptr, col = ladder
    d = CSRGraph.from_arrays(row_ptr, col).device_tensors(hip_device, need_adj_pos=True)
    off = d['adj_off'].cpu().numpy()
    tab = d['adj_hash'].cpu().numpy()
    hpos = d['adj_hpos'].cpu().numpy()
    assert len(tab) == len(hpos) == off[-1]
    gr.check_adj_hash(row_ptr, col, off, tab, hpos)
    slots = np.diff(off)
    assert {1, 2, 3} <= set((slots // 16).tolist())
    deg = np.diff(row_ptr)
    assert (deg[2], slots[2], deg[3], slots[3]) == (8, 0, 9, 16)
    assert (slots[4], slots[5], slots[6], slots[7]) == (16, 32, 32, 48)
    leaves = deg[len(gr.RUNG_DEGREES):]
    assert (leaves == 8).any() and (leaves == 9).any()


def test_hub_bitmaps_direct(ladder, hip_device):
    row_ptr, col = ladder
    V = len(row_ptr) - 1
    words = (V + 31) // 32
    rows = [13, 12, 1]          # the rungs of degree 1025, 129 and 1
    assert [int(row_ptr[r + 1] - row_ptr[r]) for r in rows] == [1025, 129, 1]
    rp, c = _dev(row_ptr, hip_device), _dev(col, hip_device)
    hubs = torch.tensor(rows, dtype=torch.int32, device=hip_device)
    bits = torch.full((len(rows), words), -1, dtype=torch.int32, device=hip_device)
    _native.call('dw_hub_bitmaps', _native.ptr(rp), _native.ptr(c), V, _native.ptr(hubs),
                 len(rows), words, _native.ptr(bits), _native.stream(hip_device))
    got = bits.cpu().numpy().view(np.uint32)
    ref = gr.hub_bits(row_ptr, col, rows, words)
    np.testing.assert_array_equal(got, ref)
    assert V % 32 == 1 and (got[:, -1] >> np.uint32(V % 32) == 0).all()
    assert got[0, -1] == 1                                     # id V - 1
    assert got[0, 0] >> np.uint32(31) == 1 and got[0, 1] & np.uint32(1) == 1   # ids 31 and 32
    assert got[0, 1] >> np.uint32(31) == 1                     # id 63
    assert [int(np.unpackbits(g.view(np.uint8)).sum()) for g in got] == [1025, 129, 1]


def test_edges_inline_direct(ladder, hip_device):
    row_ptr, col = ladder
    rp, c = _dev(row_ptr, hip_device), _dev(col, hip_device)
    e = torch.full((len(col), 4), -7, dtype=torch.int32, device=hip_device)
    _native.call('dw_edges_inline_build', _native.ptr(rp), _native.ptr(c), len(row_ptr) - 1,
                 len(col), _native.ptr(e), _native.stream(hip_device))
    np.testing.assert_array_equal(e.cpu().numpy(), gr.edges_inline(row_ptr, col))
