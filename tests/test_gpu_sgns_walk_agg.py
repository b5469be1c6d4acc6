"""Walk aggregation (k_walk_agg: each walk position's positive out-gradient terms summed once
before the sort) on the MI355X: mode 1 (on) against mode 0 (off) of the same build, and against
the float64 closed form (oracle/sgns_ref.py).

Bars, all taken from tests/test_gpu_sgns.py:
  * on vs off (the same sums reassociated): the bar at which test_fused_sgns_random_case_vs_oracle
    compares the sorted path with the atomic one — rtol 1e-4, atol 1e-6 * max |g_in|;
  * on vs float64: that test's oracle bar — rtol 1e-4, atol 1e-6 * max |g_in| (float64);
  * g_in and the four loss sums: bit-equal between the modes (pass 1's arithmetic is the same).

Bit-equality of g_in is a property of the code only where the order of its float atomics is:
one atomic row per centre, ordered inside a wave (a wave takes 4 consecutive centres one after
the other), unordered between waves. The cases therefore keep the centres of one node inside one
wave, or give a node at most two centre occurrences (two float additions onto zero commute):
the generic shapes draw every walk position as a distinct node, the structured ones (bounce,
V = 4, hub) are sized so. The loss sums are float64 atomics of per-block float sums: exact at
these sizes (a few hundred terms of like magnitude), so their order does not show.
"""
import os

import numpy as np
import pytest
import torch

from oracle import philox as ph
from oracle import sgns_ref
from test_gpu_sgns import assert_no_row_drift, assert_params_close

from shallow_encoders import _native
from shallow_encoders.word2vec import sgns
from shallow_encoders.word2vec.sgns import sgns_accumulate, sgns_phase2_pieces, set_walk_agg

pytestmark = pytest.mark.gpu

SEED, OFFSET = 11, 700


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    set_walk_agg({'0': 0, '1': 1}.get(os.environ.get('DW_SGNS_WALK_AGG', ''), -1))


def _tables(V, d, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((V, d), generator=g) - 0.5).cuda(),
            (torch.rand((V, d), generator=g) - 0.5).cuda())


def _distinct_walks(n, L, V, seed):
    """Every position of every walk a different node (see the module docstring)."""
    rng = np.random.default_rng(seed)
    return rng.permutation(V)[:n * L].reshape(n, L).astype(np.int32)


def _run(mode, walks, w_in, w_out, R, K, noise=None, phases=(0,), expect_agg=None):
    """One accumulate under `mode`; returns (g_in, g_out, loss sums, status word)."""
    set_walk_agg(mode)
    n, L = walks.shape
    d = w_in.shape[1]
    if expect_agg is not None:
        assert sgns.walk_agg_active(n, L, R, K, d) == expect_agg
    wk = torch.as_tensor(walks).cuda()
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    acc = torch.zeros(4, dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    for ph_ in phases:
        sgns_accumulate(w_in, w_out, g_in, g_out, K, walks=wk, context_radius=R, noise=noise,
                        seed=SEED, noise_offset=OFFSET, loss_acc=acc, status=status, phase=ph_)
    torch.cuda.synchronize()
    return g_in, g_out, acc, int(status.item())


def _check_modes(on, off, ref=None):
    """on / off: _run results of modes 1 and 0; ref: (g_in, g_out) float64 or None."""
    gi1, go1, acc1, st1 = on
    gi0, go0, acc0, st0 = off
    scale = float(gi0.abs().max()) if ref is None else float(np.abs(ref[0]).max())
    print('max |g_out on - off|', float((go1 - go0).abs().max()), 'max |g_in on - off|',
          float((gi1 - gi0).abs().max()), 'loss on - off', (acc1 - acc0).tolist(),
          'scale', scale)
    assert st1 == st0
    assert torch.equal(acc1, acc0)
    assert torch.equal(gi1, gi0)
    torch.testing.assert_close(go1, go0, rtol=1e-4, atol=1e-6 * scale)
    if ref is not None:
        np.testing.assert_allclose(gi1.cpu().numpy(), ref[0], rtol=1e-4, atol=1e-6 * scale)
        np.testing.assert_allclose(go1.cpu().numpy(), ref[1], rtol=1e-4, atol=1e-6 * scale)


def _oracle(walks, w_in, w_out, R, K, noise):
    ins, tgt = sgns_ref.sg_windows(walks, R)
    _, gi, go = sgns_ref.sgns_grads_closed_form(w_in.cpu().numpy(), w_out.cpu().numpy(), ins,
                                                tgt, noise)
    return gi, go


SHAPES = [(n, L, R, K, d) for n in (1, 3)
          for (L, R, K, d) in ((5, 2, 1, 64), (6, 2, 1, 64), (12, 2, 3, 128), (12, 2, 1, 256),
                               (12, 2, 1, 512))] + [(5, 80, 5, 5, 128)]


@pytest.mark.parametrize('replay', [False, True])
@pytest.mark.parametrize('n,L,R,K,d', SHAPES)
def test_agg_on_equals_off_and_float64(hip_device, n, L, R, K, d, replay):
    """(5, 2): one centre per walk, so positions 0 and 4 have exactly one term; (6, 2): two
    centres; d = 256 / 512: two and four column slices; (80, 5, 5, 128): the flagship window.
    noise=None draws the device Philox negatives, replay passes the same ids in."""
    V = 1000
    walks = _distinct_walks(n, L, V, seed=L + d)
    w_in, w_out = _tables(V, d, seed=d + n)
    ids = ph.device_noise(SEED, OFFSET, n * (L - 2 * R), 2 * R, K, V)
    noise = torch.as_tensor(ids).cuda() if replay else None
    on = _run(1, walks, w_in, w_out, R, K, noise, expect_agg=True)
    off = _run(0, walks, w_in, w_out, R, K, noise, expect_agg=False)
    _check_modes(on, off, _oracle(walks, w_in, w_out, R, K, ids))


def test_bounce_walk_same_row_at_many_positions(hip_device):
    """a, b, a, b, ...: out rows a and b each sit at half the positions, every aggregate row of
    a has the centre b as its only source node and the other way round. L = 8, R = 2: the four
    centres a, b, a, b are one wave's, so g_in's atomics are ordered."""
    V, d, R, K, L = 50, 64, 2, 1, 8
    walks = np.array([[7, 9] * (L // 2)], dtype=np.int32)
    w_in, w_out = _tables(V, d, seed=1)
    ids = ph.device_noise(SEED, OFFSET, L - 2 * R, 2 * R, K, V)
    on = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    off = _run(0, walks, w_in, w_out, R, K, expect_agg=False)
    _check_modes(on, off, _oracle(walks, w_in, w_out, R, K, ids))


def test_four_rows_three_walks_rows_straddle_chunks(hip_device):
    """V = 4 with 3 walks: every out row has many records (51 aggregated, 48 per term, in
    32-record gather chunks: rows straddle them). L = 5: one centre per walk, the three centres
    are one wave's."""
    V, d, R, K, L = 4, 64, 2, 3, 5
    walks = np.array([[0, 1, 2, 3, 0], [3, 3, 1, 0, 2], [2, 0, 2, 1, 1]], dtype=np.int32)
    w_in, w_out = _tables(V, d, seed=2)
    ids = ph.device_noise(SEED, OFFSET, 3, 2 * R, K, V)
    on = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    off = _run(0, walks, w_in, w_out, R, K, expect_agg=False)
    _check_modes(on, off, _oracle(walks, w_in, w_out, R, K, ids))


def test_all_walks_through_node_1(hip_device):
    """Node 1 at position 1 of every walk (a context of the first two centres, never a centre):
    out row 1 collects one aggregate record per walk."""
    V, d, R, K, L, n = 1000, 64, 2, 1, 12, 3
    walks = _distinct_walks(n, L, V - 2, seed=4) + 2
    walks[:, 1] = 1
    w_in, w_out = _tables(V, d, seed=3)
    ids = ph.device_noise(SEED, OFFSET, n * (L - 2 * R), 2 * R, K, V)
    on = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    off = _run(0, walks, w_in, w_out, R, K, expect_agg=False)
    assert float(on[1][1].abs().max()) > 0.0
    _check_modes(on, off, _oracle(walks, w_in, w_out, R, K, ids))


def test_bad_ids_set_the_status_and_drop_their_terms(hip_device):
    """One id of -1 (a centre and a context) and one >= V (a context only): DW_S_BAD_INDEX in
    both modes, and every row matches mode 0 (the bad slots contribute nothing in either)."""
    V, d, R, K, L = 1000, 128, 2, 3, 12
    walks = _distinct_walks(1, L, V, seed=5)
    walks[0, 5] = -1
    walks[0, 0] = V + 3
    w_in, w_out = _tables(V, d, seed=4)
    on = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    off = _run(0, walks, w_in, w_out, R, K, expect_agg=False)
    assert on[3] & _native.DW_S_BAD_INDEX and off[3] & _native.DW_S_BAD_INDEX
    assert bool(torch.isfinite(on[1]).all())
    _check_modes(on, off)


def test_phase_0_equals_phase_1_plus_2(hip_device):
    V, d, R, K, L, n = 1000, 128, 2, 3, 12, 3
    walks = _distinct_walks(n, L, V, seed=6)
    w_in, w_out = _tables(V, d, seed=5)
    whole = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    split = _run(1, walks, w_in, w_out, R, K, phases=(1, 2), expect_agg=True)
    _check_modes(split, whole)


def test_pieces_equal_the_unpieced_call(hip_device):
    """sgns_phase2_pieces with 3 pieces after a phase-1 call, aggregation on, against phase 0
    (the bar of test_phase2_pieces_equal_phase2)."""
    V, d, R, K, L, n = 300, 128, 2, 3, 12, 3
    walks = _distinct_walks(n, L, V, seed=7)
    w_in, w_out = _tables(V, d, seed=6)
    ref_in, ref_out, _, _ = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    wk = torch.as_tensor(walks).cuda()
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    sgns_accumulate(w_in, w_out, g_in, g_out, K, walks=wk, context_radius=R, seed=SEED,
                    noise_offset=OFFSET, phase=1)
    seen = []
    sgns_phase2_pieces(w_in, g_out, K, walks=wk, context_radius=R, n_pieces=3, piece_rows=100,
                       on_piece=seen.append)
    torch.cuda.synchronize()
    assert seen == [0, 1, 2]
    assert torch.equal(g_in, ref_in)
    np.testing.assert_allclose(g_out.cpu().numpy(), ref_out.cpu().numpy(), rtol=1e-5,
                               atol=1e-6 * float(ref_out.abs().max()))


def test_same_call_twice_is_bit_identical(hip_device):
    """27 records (12 negatives + 15 aggregates): one 32-record gather chunk, no boundary
    atomics, and the aggregate rows are summed in a fixed order: g_out repeats bit for bit."""
    V, d, R, K, L, n = 1000, 64, 2, 1, 5, 3
    walks = _distinct_walks(n, L, V, seed=8)
    w_in, w_out = _tables(V, d, seed=7)
    a = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    b = _run(1, walks, w_in, w_out, R, K, expect_agg=True)
    assert torch.equal(a[1], b[1])
    assert float(a[1].abs().max()) > 0.0


def test_fused_out_adam_equals_unfused(hip_device):
    """out_adam= (dw_sgns_walks_phase2_adam) against the unfused phase 2 + the HIP Adam, both
    with aggregation on, at the bar of test_fused_out_table_adam_equals_unfused."""
    from shallow_encoders.graph.random_walk_generator import DeepWalk
    from shallow_encoders.graph.rmat import rmat_graph
    from shallow_encoders.word2vec.sharding import ShardedTables
    set_walk_agg(1)
    csr = rmat_graph(12, 40_000, 0, device=hip_device)
    walker = DeepWalk(csr, 40, rng='philox', seed=3, device=hip_device)
    V, R, K, d, nw, steps = csr.vocab_size, 3, 4, 128, 32, 3
    assert sgns.walk_agg_active(nw, 40, R, K, d)
    fused = ShardedTables(V, d, hip_device, lr=0.02, init_seed=5)
    plain = ShardedTables(V, d, hip_device, lr=0.02, init_seed=5)
    for step in range(steps):
        starts = torch.randint(1, V, (nw,), generator=torch.Generator().manual_seed(step),
                               dtype=torch.int32).to(hip_device)
        walks = walker.walk_batch(starts, walk_id0=step * nw)
        for t, fuse in ((fused, True), (plain, False)):
            kw = dict(walks=walks, context_radius=R, seed=7, noise_offset=step * nw * 34)
            sgns_accumulate(t.w_in, t.w_out, t.g_in, t.g_out, K, phase=1, **kw)
            t.exchange_in()
            spec = t.out_adam_spec() if fuse else None
            sgns_accumulate(t.w_in, t.w_out, t.g_in, t.g_out, K, phase=2, out_adam=spec, **kw)
            t.exchange_out(fused_out=fuse)
            t.sync()
    torch.cuda.synchronize()
    assert float(fused.grads.abs().max()) == 0.0
    assert int(fused._row_flags.max()) == 0
    for a, b in ((fused.w_in, plain.w_in), (fused.w_out, plain.w_out)):
        assert_params_close(a.cpu().numpy(), b.cpu().numpy(), 0.02, max_frac=5e-3,
                            max_abs=2.05 * 0.02 * steps)
        assert_no_row_drift(a.cpu().numpy(), b.cpu().numpy())
    np.testing.assert_allclose(fused.m.cpu().numpy(), plain.m.cpu().numpy(), rtol=1e-3,
                               atol=1e-6)


def test_deterministic_mode_keeps_the_per_term_records(hip_device):
    """After enable_exact the predicate keeps the legacy records: auto and off give
    bit-identical tables (the fixed-point sums are per term)."""
    from shallow_encoders.word2vec.sharding import ShardedTables, replicated_step
    V, d, R, K, L, n, steps = 500, 128, 2, 3, 12, 16, 2
    walks = torch.randint(1, V, (steps, n, L), generator=torch.Generator().manual_seed(3),
                          dtype=torch.int32)
    per = L - 2 * R
    scale = 1.0 / (n * per * 2 * R)

    def run(mode):
        set_walk_agg(mode)
        assert sgns.walk_agg_active(n, L, R, K, d) == (mode != 0)   # (shape alone)
        t = ShardedTables(V, d, hip_device, lr=0.01, init_seed=2)
        t.enable_exact(scale)
        acc = torch.zeros(4, dtype=torch.float64, device=hip_device)
        st = torch.zeros(1, dtype=torch.int32, device=hip_device)
        for s in range(steps):
            replicated_step(t, walks[s].cuda(), R, K, seed=5, noise_offset=s * n * per,
                            grad_scale=scale, loss_acc=acc, status=st)
        torch.cuda.synchronize()
        _native.check_status(st, 'replicated_step')
        return [x.cpu().clone() for x in (t.w_in, t.w_out, acc)]

    for x, y in zip(run(-1), run(0)):
        assert torch.equal(x, y)


def test_legacy_sized_workspace_is_refused(hip_device):
    """A workspace of dw_sgns_workspace_bytes passed to a walks call with aggregation on:
    DW_E_INVALID_ARG and a message, nothing launched."""
    import ctypes
    V, d, R, K, L, n = 1000, 128, 2, 3, 12, 3
    set_walk_agg(1)
    walks = torch.as_tensor(_distinct_walks(n, L, V, seed=9)).cuda()
    w_in, w_out = _tables(V, d, seed=8)
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    acc = torch.zeros(4, dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    nbytes, wbytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _native.call('dw_sgns_workspace_bytes', n * (L - 2 * R), 2 * R, K, V, ctypes.byref(nbytes))
    _native.call('dw_sgns_walks_workspace_bytes', n, L, R, K, V, d, ctypes.byref(wbytes))
    assert wbytes.value > nbytes.value
    ws = torch.empty(wbytes.value, dtype=torch.uint8, device='cuda')
    lib = _native.load()
    args = (_native.ptr(walks), n, L, R, K, V, d, _native.ptr(w_in), _native.ptr(w_out),
            _native.ptr(g_in), _native.ptr(g_out), None, SEED, OFFSET, 1.0,
            _native.ptr(acc), _native.ptr(status), _native.ptr(ws))
    rc = lib.dw_sgns_walks(*args, nbytes.value, _native.stream(hip_device))
    assert rc == _native.DW_E_INVALID_ARG
    assert b'workspace too small' in lib.dw_last_error_string()
    torch.cuda.synchronize()
    assert float(g_in.abs().max()) == 0.0 and float(g_out.abs().max()) == 0.0
    assert lib.dw_sgns_walks(*args, wbytes.value, _native.stream(hip_device)) == _native.DW_OK
    torch.cuda.synchronize()
    assert float(g_out.abs().max()) > 0.0


def test_graphed_step_equals_eager_with_aggregation(hip_device):
    """GraphedStep with scatter='sorted' at C2's shape (2R(L-2R) = 24 >= 2L = 20: the auto mode
    aggregates): graphed equals eager at the bars of tests/test_gpu_graphed.py."""
    from test_gpu_graphed import B, D, K as GK, L as GL, LR, R as GR, SEED as GSEED, _setup
    from shallow_encoders.word2vec.graphed import GraphedStep
    from shallow_encoders.word2vec.sharding import ShardedTables, replicated_step
    set_walk_agg(-1)
    assert sgns.walk_agg_active(B, GL, GR, GK, D)
    dev = hip_device
    csr, walker, epoch = _setup(dev)
    V = csr.vocab_size
    grad_scale = 1.0 / (B * (GL - 2 * GR) * 2 * GR)
    warm, steps = 2, 6
    runs = []
    for mode in ('eager', 'graph'):
        t = ShardedTables(V, D, dev, lr=LR, init_seed=0, overlap_in=True)
        acc = torch.zeros(4, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def eager(s):
            g0 = s * B
            st = epoch[torch.arange(g0, g0 + B, device=dev) % epoch.numel()]
            walks = walker.walk_batch(st, walk_id0=g0, check=False)
            replicated_step(t, walks, GR, GK, seed=GSEED, noise_offset=g0 * (GL - 2 * GR),
                            grad_scale=grad_scale, loss_acc=acc, status=status,
                            scatter='sorted', fuse_out_adam=True)
        for s in range(warm):
            eager(s)
        if mode == 'eager':
            for s in range(warm, warm + steps):
                eager(s)
        else:
            gs = GraphedStep(t, walker, epoch, B, GR, GK, seed=GSEED, grad_scale=grad_scale,
                             loss_acc=acc, status=status, first_walk_id=warm * B,
                             n_steps=steps, scatter='sorted', unroll=1)
            for _ in range(steps):
                gs.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        runs.append((t.w_in.cpu().numpy(), t.w_out.cpu().numpy(), acc.cpu().numpy()))
    (wi_e, wo_e, acc_e), (wi_g, wo_g, acc_g) = runs
    np.testing.assert_allclose(acc_g, acc_e, rtol=1e-9)
    for got, exp in ((wi_g, wi_e), (wo_g, wo_e)):
        assert_params_close(got, exp, LR)
        assert_no_row_drift(got, exp)
