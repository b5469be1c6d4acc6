"""Owner-computes SGNS (N > 1 layout) on the GPU: dw_sgns_owner_pass1 / dw_sgns_owner_pass2.

Rank r of W holds the out-table rows o with o % W == r and computes only those output slots of
the whole global batch. Checked here on one device by running every owner in turn:
  * each owner's gradients equal the oracle's owner split (sgns_grads_closed_form(owner=r));
  * the owners' parts add up to the single-device step (dw_sgns_walks_phase): the partial
    g_in's sum to g_in, the local g_out slices are g_out's rows r, r+W, ...; loss sums add up;
    the record counts add up to every slot;
  * the slice's fused Adam equals pass 2 followed by dw_adam_dense on the slice;
  * an empty batch still gives every slice row its g = 0 Adam step; bad ids are reported;
  * two ranks (gloo, both on cuda:0) training with OwnerTables + owner_step equal one process
    training the whole batch (ShardedTables).
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import sgns_ref
from shallow_encoders import _native
from shallow_encoders.word2vec.sgns import (loss_terms, sgns_accumulate, sgns_owner_pass1,
                                           sgns_owner_pass2)
from test_gpu_sgns import assert_no_row_drift, assert_params_close

pytestmark = pytest.mark.gpu


def _owner_parts(w_in, w_out, walks, R, K, W, noise=None, seed=9, noise_offset=0, scale=None):
    """Every owner's (partial g_in, local g_out, loss_acc, n_records) for the same batch."""
    V, d = w_out.shape
    S = -(-V // W)
    parts = []
    for r in range(W):
        rows = torch.arange(S, device=w_out.device) * W + r
        w_loc = torch.zeros((S, d), dtype=torch.float32, device=w_out.device)
        keep = rows < V
        w_loc[keep] = w_out[rows[keep]]
        g_in = torch.zeros_like(w_in)
        g_loc = torch.zeros_like(w_loc)
        acc = sgns_owner_pass1(w_in, w_loc, g_in, K, walks=walks, context_radius=R, owner=r,
                               n_owners=W, vocab_size=V, noise=noise, seed=seed,
                               noise_offset=noise_offset, grad_scale=scale)
        n = sgns_owner_pass2(w_in, w_loc, g_loc, K, walks=walks, context_radius=R)
        parts.append((g_in, g_loc, acc, n, rows, keep))
    return parts


@pytest.mark.parametrize('d,W', [(128, 1), (128, 2), (128, 3), (64, 8), (256, 5)])
def test_owner_parts_vs_oracle_and_full_step(hip_device, d, W):
    rng = np.random.default_rng(d + W)
    V, R, K, L, n = 3001, 3, 4, 24, 40
    w_in0, w_out0 = sgns_ref.xavier_tables(V, d, seed=d)
    walks = rng.integers(0, V, size=(n, L)).astype(np.int32)
    walks[:, ::4] = 11                      # a hub row straddling many gather chunks
    ins, tgt = sgns_ref.sg_windows(walks, R)
    noise = rng.integers(0, V, size=(len(ins), 2 * R, K))
    w_in = torch.as_tensor(w_in0).cuda()
    w_out = torch.as_tensor(w_out0).cuda()
    wk = torch.as_tensor(walks).cuda()
    nz = torch.as_tensor(noise).cuda()
    parts = _owner_parts(w_in, w_out, wk, R, K, W, noise=nz)
    # the single-device step over the same batch
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    acc = sgns_accumulate(w_in, w_out, g_in, g_out, K, walks=wk, context_radius=R, noise=nz)
    full_loss, gi_full, go_full = sgns_ref.sgns_grads_closed_form(w_in0, w_out0, ins, tgt, noise)
    scale = float(np.abs(gi_full).max())
    T = 2 * R * (1 + K)
    assert sum(p[3] for p in parts) == len(ins) * T        # every slot owned exactly once
    sum_gin = torch.zeros_like(w_in)
    sum_acc = torch.zeros(4, dtype=torch.float64, device='cuda')
    for r, (gi_r, go_r, acc_r, n_r, rows, keep) in enumerate(parts):
        loss_r, gi_o, go_o = sgns_ref.sgns_grads_closed_form(w_in0, w_out0, ins, tgt, noise,
                                                             owner=r, n_owners=W)
        np.testing.assert_allclose(gi_r.cpu().numpy(), gi_o, rtol=1e-4, atol=1e-6 * scale)
        rk = rows[keep].cpu().numpy()
        np.testing.assert_allclose(go_r[keep].cpu().numpy(), go_o[rk], rtol=1e-4,
                                   atol=1e-6 * scale)
        if (~keep).any():
            assert float(go_r[~keep].abs().max()) == 0.0         # padding rows untouched
        torch.testing.assert_close(go_r[keep], g_out[rows[keep]], rtol=1e-4,
                                   atol=1e-6 * scale)
        assert float(loss_terms(acc_r, tgt.size, K)['loss']) == pytest.approx(loss_r, rel=1e-4,
                                                                              abs=1e-6)
        sum_gin += gi_r
        sum_acc += acc_r
    torch.testing.assert_close(sum_gin, g_in, rtol=1e-4, atol=1e-6 * scale)
    torch.testing.assert_close(sum_acc, acc, rtol=1e-5, atol=1e-6)
    assert float(loss_terms(sum_acc, tgt.size, K)['loss']) == pytest.approx(full_loss, rel=1e-5)


def test_owner_device_noise_equals_replayed(hip_device):
    """noise=None draws the same Philox negatives as dw_sgns_walks_phase (keyed by the global
    centre), so the owners' parts of a device-noise step add up to that step."""
    rng = np.random.default_rng(3)
    V, d, R, K, L, n, W = 5000, 128, 5, 5, 30, 32, 4
    w_in0, w_out0 = sgns_ref.xavier_tables(V, d, seed=1)
    w_in, w_out = torch.as_tensor(w_in0).cuda(), torch.as_tensor(w_out0).cuda()
    wk = torch.as_tensor(rng.integers(1, V, size=(n, L)).astype(np.int32)).cuda()
    parts = _owner_parts(w_in, w_out, wk, R, K, W, seed=77, noise_offset=12345)
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    acc = sgns_accumulate(w_in, w_out, g_in, g_out, K, walks=wk, context_radius=R, seed=77,
                          noise_offset=12345)
    scale = float(g_in.abs().max())
    torch.testing.assert_close(sum(p[0] for p in parts), g_in, rtol=1e-4, atol=1e-6 * scale)
    torch.testing.assert_close(sum(p[2] for p in parts), acc, rtol=1e-5, atol=1e-6)
    for g_in_r, g_loc, _, _, rows, keep in parts:
        torch.testing.assert_close(g_loc[keep], g_out[rows[keep]], rtol=1e-4, atol=1e-6 * scale)


@pytest.mark.parametrize('d', [64, 128])
def test_owner_fused_slice_adam_equals_unfused(hip_device, d):
    from shallow_encoders.word2vec.sharding import adam_scalars, hip_adam
    rng = np.random.default_rng(d)
    V, R, K, L, n, W, lr = 4000, 2, 3, 16, 64, 3, 0.02
    S = -(-V // W)
    w_in = torch.as_tensor(sgns_ref.xavier_tables(V, d, seed=2)[0]).cuda()
    base = torch.randn((S, d), generator=torch.Generator().manual_seed(1)).cuda() * 0.1
    fused = [base.clone(), torch.zeros_like(base), torch.zeros_like(base), torch.zeros_like(base)]
    plain = [base.clone(), torch.zeros_like(base), torch.zeros_like(base), torch.zeros_like(base)]
    flags = torch.zeros(S, dtype=torch.uint8, device='cuda')
    for step in range(1, 4):
        wk = torch.as_tensor(rng.integers(0, V, size=(n, L)).astype(np.int32)).cuda()
        for tabs, fuse in ((fused, True), (plain, False)):
            w, g, m, v = tabs
            g_in = torch.zeros_like(w_in)
            sgns_owner_pass1(w_in, w, g_in, K, walks=wk, context_radius=R, owner=1, n_owners=W,
                             vocab_size=V, seed=step, noise_offset=0)
            spec = ({'m': m, 'v': v, 'flags': flags,
                     'scalars': adam_scalars(step, lr, (0.9, 0.999), 1e-8, 0.0)}
                    if fuse else None)
            sgns_owner_pass2(w_in, w, g, K, walks=wk, context_radius=R, out_adam=spec)
            if not fuse:
                hip_adam(w.view(-1), g.view(-1), m.view(-1), v.view(-1), step, lr,
                         (0.9, 0.999), 1e-8, 0.0, True)
    torch.cuda.synchronize()
    assert float(fused[1].abs().max()) == 0.0 and int(flags.max()) == 0
    assert_params_close(fused[0].cpu().numpy(), plain[0].cpu().numpy(), lr, max_frac=5e-3,
                        max_abs=2.05 * lr * 3)
    assert_no_row_drift(fused[0].cpu().numpy(), plain[0].cpu().numpy())
    np.testing.assert_allclose(fused[2].cpu().numpy(), plain[2].cpu().numpy(), rtol=1e-3,
                               atol=1e-6)


def test_owner_empty_batch_and_bad_index(hip_device):
    from shallow_encoders.word2vec.sharding import adam_scalars, hip_adam
    V, d, R, K, W = 1000, 64, 2, 2, 2
    S = V // W
    w_in = torch.randn((V, d), device='cuda')
    w = torch.randn((S, d), device='cuda')
    w2 = w.clone()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    m2, v2 = torch.zeros_like(w), torch.zeros_like(w)
    g = torch.zeros_like(w)
    flags = torch.zeros(S, dtype=torch.uint8, device='cuda')
    empty = torch.zeros((0, 10), dtype=torch.int32, device='cuda')
    g_in = torch.zeros_like(w_in)
    sgns_owner_pass1(w_in, w, g_in, K, walks=empty, context_radius=R, owner=0, n_owners=W,
                     vocab_size=V)
    n = sgns_owner_pass2(w_in, w, g, K, walks=empty, context_radius=R,
                         out_adam={'m': m, 'v': v, 'flags': flags,
                                   'scalars': adam_scalars(1, 0.1, (0.9, 0.999), 1e-8, 0.0)})
    assert n == 0
    hip_adam(w2.view(-1), torch.zeros_like(w2).view(-1), m2.view(-1), v2.view(-1), 1, 0.1,
             (0.9, 0.999), 1e-8, 0.0, True)
    torch.testing.assert_close(w, w2, rtol=0, atol=0)
    # an id outside [0, V) is reported through the status word, not a fault
    bad = torch.randint(0, V, (4, 10), dtype=torch.int32, device='cuda')
    bad[2, 5] = V + 3
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    sgns_owner_pass1(w_in, w, g_in, K, walks=bad, context_radius=R, owner=0, n_owners=W,
                     vocab_size=V, status=status)
    sgns_owner_pass2(w_in, w, torch.zeros_like(w), K, walks=bad, context_radius=R, status=status)
    with pytest.raises(IndexError):
        _native.check_status(status, 'owner sgns')
    # widths the 16-lane kernel does not cover are refused, not mis-computed
    with pytest.raises(Exception):
        sgns_owner_pass1(torch.zeros((V, 96), device='cuda'), torch.zeros((S, 96), device='cuda'),
                         torch.zeros((V, 96), device='cuda'), K, walks=bad[:1] % V,
                         context_radius=R, owner=0, n_owners=W, vocab_size=V)


# ---- two ranks on one GPU (gloo carries the collectives; RCCL refuses two ranks per device) ----
V2, D2, R2, K2, L2, NW2, STEPS2, LR2 = 700, 64, 2, 3, 12, 48, 3, 1e-3


def _walks_all():
    g = torch.Generator().manual_seed(8)
    return torch.randint(1, V2, (STEPS2, NW2, L2), generator=g, dtype=torch.int32)


def _owner_snapshot(t, V):
    """(w_in, w_out, m_in, v_in, m_out, v_out) as full (V, d) arrays, gathered from every rank
    (collective: every rank calls it at the same point). Lazy tables: the state with every
    deferred step applied, the tables themselves left lagging."""
    lag = []
    if hasattr(t, 'last_in'):
        lag = [t.params_in, t.m_in, t.v_in, t.last_in]
        if t.lazy_out:   # (the rows-major step's pending marks too: the flush settles them)
            lag += [t.w_out, t.m_out, t.v_out, t.last_out, t.pend_out]
        keep = [x.clone() for x in lag]
        dirty = getattr(t, '_pend_dirty', False)
        t.flush()
    m_out, v_out = t.out_state_full()
    if t.m_in.shape[0] == t.V_pad:             # replicated in-table state (lazy)
        m_in, v_in = t.m_in[:V], t.v_in[:V]
    else:                                      # node-range shards
        m_in, v_in = [], []
        for x, dst in ((t.m_in, m_in), (t.v_in, v_in)):
            parts = [torch.empty_like(x) for _ in range(t.world)]
            dist.all_gather(parts, x.contiguous())
            dst.append(torch.cat(parts)[:V])
        m_in, v_in = m_in[0], v_in[0]
    snap = tuple(x.cpu().numpy().copy() for x in (t.w_in, t.full_w_out(), m_in, v_in, m_out,
                                                   v_out))
    for dst, src in zip(lag, keep if lag else []):
        dst.copy_(src)
    if lag:
        t._pend_dirty = dirty
    return snap


def _init2():
    from shallow_encoders.word2vec.sharding import ShardedTables
    t0 = ShardedTables(V2, D2, 'cpu', lr=LR2, init_seed=4)
    return t0.w_in.numpy().copy(), t0.w_out.numpy().copy()


def _owner_run(rank, world, port, q):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from shallow_encoders.word2vec.sharding import OwnerTables, owner_step
        t = OwnerTables(V2, D2, 'cuda:0', lr=LR2, init_seed=4)
        walks = _walks_all()
        per = L2 - 2 * R2
        acc = torch.zeros(4, dtype=torch.float64, device='cuda:0')
        status = torch.zeros(1, dtype=torch.int32, device='cuda:0')
        snaps = []
        for s in range(STEPS2):
            owner_step(t, walks[s].cuda(), R2, K2, seed=11, noise_offset=s * NW2 * per,
                       grad_scale=1.0 / (NW2 * per * 2 * R2), loss_acc=acc, status=status)
            torch.cuda.synchronize()
            snaps.append(_owner_snapshot(t, V2))
        _native.check_status(status, 'owner_step')
        q.put((rank, t.w_in.cpu().numpy().copy(), t.full_w_out().cpu().numpy(),
               acc.cpu().numpy(), None, snaps))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # report, the parent asserts
        q.put((rank, None, None, None, repr(e), None))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_owner_tables_two_ranks_equal_single_process(hip_device):
    from shallow_encoders.word2vec.sharding import ShardedTables
    ref = ShardedTables(V2, D2, hip_device, lr=LR2, init_seed=4)
    walks = _walks_all()
    per = L2 - 2 * R2
    acc_ref = torch.zeros(4, dtype=torch.float64, device=hip_device)
    for s in range(STEPS2):
        sgns_accumulate(ref.w_in, ref.w_out, ref.g_in, ref.g_out, K2, walks=walks[s].cuda(),
                        context_radius=R2, seed=11, noise_offset=s * NW2 * per,
                        loss_acc=acc_ref)
        ref.step()
    torch.cuda.synchronize()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_owner_run, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    errs = [r[4] for r in res if r[4]]
    assert not errs, errs
    (_, i0, o0, a0, _, s0), (_, i1, o1, a1, _, s1) = res
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(o0, o1)
    np.testing.assert_allclose(a0 + a1, acc_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    for a, b in zip(s0, s1):                   # both ranks gathered the same state every step
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    # every step from the state before it, at the single-step bars (tests/stepcheck.py)
    from stepcheck import check_trajectory
    worst = check_trajectory('owner 2 ranks', _init2(), s0, _walks_all(), R2, K2, 11, LR2,
                             NW2 * per)
    print({k: round(v, 3) for k, v in sorted(worst.items())})


# ---- the touched-row in-table exchange: lazy exact Adam (dw_adam_rows, OwnerLazyTables) -------
@pytest.mark.parametrize('d,sched,S', [(128, False, 600), (64, True, 600), (96, False, 600),
                                       (128, False, 2500)])
def test_rows_adam_long_lag_bit_exact(hip_device, d, sched, S):
    """Replays of up to S missed g = 0 steps through the box history (sharding.hist_row /
    hist_header, as OwnerLazyTables writes it): the tail where the parameter provably no longer
    moves runs m and v alone (dw::frozen_el) — the same bits as one dense dw_adam_dense per
    step, and as the same replay with the freeze disabled (header F = +inf). Rows include
    p = -0 with m = -0 (never frozen), m = 0 and p = 0; sched: the lr changes along the run.
    With the betas constant the frozen steps take them from the header (no per-step loads); a
    wave whose m is +0 in every lane (here only the row that starts with m = 0) steps v alone.
    The kernels keep fp32 denormals, so m does not underflow to +0 by decay: with
    1 - beta1 = 0.1f it goes subnormal after ~900 steps and sticks at 4 units of 2^-149
    (S = 2500 reaches that; tests/test_oracle_adam.py, and tests/test_gpu_adam_ieee.py for the
    device against the IEEE oracle). The header's betas withheld (NaN) gives the per-step form —
    the same bits again."""
    import time
    from shallow_encoders.word2vec.sharding import hip_adam, hip_rows_adam, hist_header, hist_row
    g = torch.Generator().manual_seed(d)
    V = 256
    betas, eps = (0.9, 0.999), 1e-8
    lrs = [0.01 if (not sched or s < 300) else 0.005 for s in range(S + 1)]
    hist = np.zeros((S + 1, 8), dtype=np.float32)
    for s in range(1, S + 1):
        hist[s] = hist_row(s, lrs[s - 1], betas, eps, 0.0)
    hist[0] = hist_header(hist, S)
    assert np.isfinite(hist[0, 2])                  # the freeze is certified for these rows
    p0 = torch.randn((V, d), generator=g) * 0.05
    m0 = torch.randn((V, d), generator=g) * 1e-6
    v0 = torch.rand((V, d), generator=g) * 1e-9
    p0[0, :8] = -0.0
    m0[0, :8] = -0.0
    m0[1] = 0.0
    p0[2, :4] = 0.0
    last0 = torch.randint(0, 40, (V,), generator=g, dtype=torch.int32)
    ref = [t.cuda().clone() for t in (p0, m0, v0)]
    for s in range(1, S + 1):
        rows = torch.nonzero(last0 < s).flatten().cuda()
        pp, mm, vv = (t[rows].contiguous() for t in ref)
        hip_adam(pp.view(-1), torch.zeros_like(pp).view(-1), mm.view(-1), vv.view(-1), s,
                 lrs[s - 1], betas, eps, 0.0, False)
        for t, u in zip(ref, (pp, mm, vv)):
            t[rows] = u
    assert np.isfinite(hist[0, 4]) and np.isfinite(hist[0, 5])   # constant betas certified
    out = {}
    for freeze in (False, True, 'per_step'):
        h = hist.copy()
        if not freeze:
            h[0, 2] = np.inf
        if freeze == 'per_step':
            h[0, 4] = h[0, 5] = np.nan
        hd = torch.from_numpy(h).cuda()
        p, m, v = (t.cuda().clone() for t in (p0, m0, v0))
        last = last0.cuda().clone()
        torch.cuda.synchronize()
        a = time.perf_counter()
        hip_rows_adam(p, m, v, last, None, None, V, None, hd, S)
        torch.cuda.synchronize()
        out[freeze] = (time.perf_counter() - a, p, m, v)
        assert int(last.min()) == S
    print(f'd={d}: replay {out[False][0] * 1e3:.2f} ms, with the frozen tail '
          f'{out[True][0] * 1e3:.2f} ms')
    print(f'   frozen steps with per-step betas {out["per_step"][0] * 1e3:.2f} ms')
    for freeze in (True, False, 'per_step'):
        for name, a, b in zip('pmv', out[freeze][1:], ref):
            assert torch.equal(a, b), f'freeze={freeze} {name}: {int((a != b).sum())} differ'

@pytest.mark.parametrize('d,wd', [(64, 0.0), (96, 0.0), (128, 0.01)])
def test_rows_adam_replay_is_bit_exact(hip_device, d, wd):
    """dw_adam_rows replaying a row's missed steps (g = 0, per-step lr) gives exactly what one
    dense dw_adam_dense per step would have given; the gradient step on top matches too.
    wd = 0 replays through adam_elem_g0 (the zero-gradient form), wd > 0 through adam_elem."""
    from shallow_encoders.word2vec.sharding import adam_scalars, hip_adam, hip_rows_adam
    g = torch.Generator().manual_seed(d)
    V, S = 300, 7
    betas, eps = (0.9, 0.999), 1e-8
    lrs = [0.1, 0.1, 0.05, 0.05, 0.02, 0.01, 0.01, 0.01]       # step s uses lrs[s - 1]
    hist = torch.zeros((S + 2, 8))
    for s in range(1, S + 2):
        hist[s, :7] = torch.tensor(adam_scalars(s, lrs[s - 1], betas, eps, wd))
    hist = hist.cuda()
    p0 = torch.randn((V, d), generator=g)
    m0 = torch.randn((V, d), generator=g) * 1e-2
    v0 = torch.rand((V, d), generator=g) * 1e-3
    last0 = torch.randint(0, S + 1, (V,), generator=g, dtype=torch.int32)
    # reference: every row behind step s gets a dense g = 0 step s (hip_adam on the gathered rows)
    ref = [t.cuda().clone() for t in (p0, m0, v0)]
    for s in range(1, S + 1):
        rows = torch.nonzero(last0 < s).flatten().cuda()
        pp, mm, vv = (t[rows].contiguous() for t in ref)
        hip_adam(pp.view(-1), torch.zeros_like(pp).view(-1), mm.view(-1), vv.view(-1), s,
                 lrs[s - 1], betas, eps, wd, False)
        for t, u in zip(ref, (pp, mm, vv)):
            t[rows] = u
    p, m, v = (t.cuda().clone() for t in (p0, m0, v0))
    last = last0.cuda().clone()
    hip_rows_adam(p, m, v, last, None, None, V, None, hist, S)          # replay every row to S
    torch.cuda.synchronize()
    for a, b in zip((p, m, v), ref):
        assert torch.equal(a, b)
    assert int(last.min()) == S == int(last.max())
    # a gradient step S + 1 on some rows (listed, with a device count) vs the dense kernel
    rows = torch.tensor([3, 17, 18, 250, 299], dtype=torch.int32).cuda()
    n_dev = torch.tensor([5], dtype=torch.int64).cuda()
    gr = torch.randn((5, d), generator=g).cuda()
    hip_rows_adam(p, m, v, last, rows, n_dev, 5, gr, hist, S + 1)
    ri = rows.long()
    pp, mm, vv = (t[ri].contiguous() for t in ref)
    hip_adam(pp.view(-1), gr.clone().view(-1), mm.view(-1), vv.view(-1), S + 1, lrs[S], betas,
             eps, wd, False)
    torch.cuda.synchronize()
    assert torch.equal(p[ri], pp) and torch.equal(m[ri], mm) and torch.equal(v[ri], vv)
    assert (last[ri] == S + 1).all() and int((last == S + 1).sum()) == 5


def _lazy_vs_dense(device, walks_all, V, d, R, K, lr, world=1, rank=0, lazy_out=False,
                   snaps=None, wd=0.0, configure=None):
    """(lazy tables after the run, per-step record counts) over walks_all [steps, n, L];
    ``snaps``: a list receiving _owner_snapshot after every step; ``configure``: called on the
    fresh tables (e.g. to select the out slice's catch-up forms)."""
    from shallow_encoders.word2vec.sharding import OwnerLazyTables, owner_lazy_step
    t = OwnerLazyTables(V, d, device, lr=lr, init_seed=4, lazy_out=lazy_out, weight_decay=wd)
    if configure is not None:
        configure(t)
    n, L = walks_all.shape[1:]
    per = L - 2 * R
    acc = torch.zeros(4, dtype=torch.float64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    dev_walks = [walks_all[s].to(device) for s in range(walks_all.shape[0])]
    for s in range(walks_all.shape[0]):
        owner_lazy_step(t, dev_walks[s], R, K, seed=11, noise_offset=s * n * per,
                        grad_scale=1.0 / (n * per * 2 * R), loss_acc=acc, status=status)
        if snaps is not None:
            torch.cuda.synchronize()
            snaps.append(_owner_snapshot(t, V))
    torch.cuda.synchronize()
    _native.check_status(status, 'owner_lazy_step')
    return t, acc


@pytest.mark.parametrize('lazy_out,wd', [(False, 0.0), (True, 0.0), (True, 0.01)])
def test_owner_lazy_single_rank_equals_dense(hip_device, lazy_out, wd):
    """One rank: sparse batches (most rows untouched for several steps) through the lazy
    protocol equal dense training (ShardedTables + dw_adam_dense every step) after a flush;
    lazy_out: the out slice's Adam deferred too (dw_sgns_owner_pass2_lazy, k_lazy_boundary),
    with the records placed by the claim and the p-only catch-up (m, v replayed in the gather);
    with weight decay the catch-up replays p, m and v (m, v then read p)."""
    from shallow_encoders.word2vec.sharding import ShardedTables
    V, d, R, K, L, n, steps, lr = 5000, 64, 2, 3, 12, 16, 6, 0.01
    walks = torch.randint(1, V, (steps, n, L), generator=torch.Generator().manual_seed(3),
                          dtype=torch.int32)
    ref = ShardedTables(V, d, hip_device, lr=lr, init_seed=4, weight_decay=wd)
    per = L - 2 * R
    acc_ref = torch.zeros(4, dtype=torch.float64, device=hip_device)
    for s in range(steps):
        sgns_accumulate(ref.w_in, ref.w_out, ref.g_in, ref.g_out, K, walks=walks[s].cuda(),
                        context_radius=R, seed=11, noise_offset=s * n * per, loss_acc=acc_ref)
        ref.step()
    t, acc = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=lazy_out, wd=wd)
    if lazy_out:
        # placed, p-only catch-up and constant betas without weight decay (step 6: slot 0)
        assert t.out_flags() == (1 if wd else 7)
    lag = int((t.last_in[:V] < steps).sum())
    assert lag > V // 2                      # most rows were deferred before the flush
    if lazy_out:
        lag_out = int((t.last_out[:V] < steps).sum())
        assert lag_out > V // 4, lag_out     # out rows deferred too
        assert int(t.last_out.max()) == steps
    w_in = t.w_in.cpu().numpy()              # flush
    assert int(t.last_in.min()) == steps
    if lazy_out:
        assert int(t.last_out.min()) == steps
    torch.testing.assert_close(acc, acc_ref, rtol=1e-5, atol=1e-6)
    for got, exp in ((w_in, ref.w_in.cpu().numpy()), (t.full_w_out().cpu().numpy(),
                                                      ref.w_out.cpu().numpy())):
        assert_params_close(got, exp, lr, rtol=1e-5, atol=1e-6, max_frac=1e-3,
                            max_abs=2.05 * lr * steps)
        assert_no_row_drift(got, exp)


def _lazy_configure(lazy_out: bool, exact: bool):
    """_lazy_vs_dense's configure: the rows-major out step is asserted (lazy_out: placed records
    per owner slice, k_out_rows, the COEFIN centre pass) and the deterministic mode enabled."""
    def cfg(t):
        if lazy_out:
            assert t.rows_major_ok(R2, K2)
        if exact:
            t.enable_exact(1.0 / (NW2 * (L2 - 2 * R2) * 2 * R2))
    return cfg


def _lazy_run(rank, world, port, q, lazy_out=False, exact=False):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        snaps = []
        t, acc = _lazy_vs_dense('cuda:0', _walks_all(), V2, D2, R2, K2, LR2, snaps=snaps,
                                lazy_out=lazy_out, configure=_lazy_configure(lazy_out, exact))
        assert t.multi and t.lazy_out == lazy_out and t._rows_step == lazy_out
        q.put((rank, t.w_in.cpu().numpy().copy(), t.full_w_out().cpu().numpy(),
               acc.cpu().numpy(), None, snaps))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # report, the parent asserts
        q.put((rank, None, None, None, repr(e), None))


def _two_lazy_ranks(lazy_out: bool, exact: bool):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lazy_run, args=(r, 2, port, q, lazy_out, exact))
             for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    errs = [r[4] for r in res if r[4]]
    assert not errs, errs
    return res


@pytest.mark.timeout(600)
def test_owner_lazy_rows_major_two_ranks(hip_device):
    """the reference's small-batch path at N > 1 — OwnerLazyTables(lazy_out)
    on two ranks (gloo on one GPU) takes the rows-major out step per owner slice (each rank
    places and steps only its o % 2 rows; the COEFIN centre pass forms its partial centre
    gradients; the touched in rows all-reduced): both ranks gather the same state every step,
    the loss terms sum to one process's, and every step from the state before it is at the
    single-step bars (tests/stepcheck.py)."""
    res = _two_lazy_ranks(True, False)
    (_, i0, o0, a0, _, s0), (_, i1, o1, a1, _, s1) = res
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(o0, o1)
    for a, b in zip(s0, s1):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    from stepcheck import check_trajectory
    worst = check_trajectory('owner lazy rows-major 2 ranks', _init2(), s0, _walks_all(), R2,
                             K2, 11, LR2, NW2 * (L2 - 2 * R2))
    print({k: round(v, 3) for k, v in sorted(worst.items())})
    # the loss sums of the 3 steps against one process's: the float order of the out rows'
    # sums (the claim's atomics rank the records) moves g ~ 0 entries by Adam-normalised steps
    # after step 1, so the later steps' losses agree to ~1e-5 and the 0.5-threshold metric
    # counts not at all (bit-identity is the deterministic test below)
    _, acc1 = _lazy_vs_dense(hip_device, _walks_all(), V2, D2, R2, K2, LR2, lazy_out=True)
    np.testing.assert_allclose((a0 + a1)[:2], acc1.cpu().numpy()[:2], rtol=1e-4)


@pytest.mark.timeout(600)
def test_owner_lazy_rows_major_two_ranks_deterministic_equal_one_process(hip_device):
    """The deterministic mode at N > 1 on the lazy path: two ranks with the
    rows-major out step, the in rows' integer centre sums all-reduced as int64 and converted on
    every rank, end every step bit-identical to one process's deterministic lazy run — tables and
    Adam state (flushed snapshots) and the final tables."""
    snaps1 = []
    t1, _ = _lazy_vs_dense(hip_device, _walks_all(), V2, D2, R2, K2, LR2, lazy_out=True,
                           snaps=snaps1, configure=_lazy_configure(True, True))
    w_in1, w_out1 = t1.w_in.cpu().numpy().copy(), t1.full_w_out().cpu().numpy()
    res = _two_lazy_ranks(True, True)
    for rank, w_in, w_out, _, _, snaps in res:
        np.testing.assert_array_equal(w_in, w_in1)
        np.testing.assert_array_equal(w_out, w_out1)
        for k, (a, b) in enumerate(zip(snaps, snaps1)):
            for name, x, y in zip(('w_in', 'w_out', 'm_in', 'v_in', 'm_out', 'v_out'), a, b):
                diff = int((x != y).sum())
                assert diff == 0, f'rank {rank} step {k}: {name} differs in {diff} entries'


@pytest.mark.timeout(600)
def test_owner_lazy_two_ranks_equal_single_process(hip_device):
    from shallow_encoders.word2vec.sharding import ShardedTables
    ref = ShardedTables(V2, D2, hip_device, lr=LR2, init_seed=4)
    walks = _walks_all()
    per = L2 - 2 * R2
    acc_ref = torch.zeros(4, dtype=torch.float64, device=hip_device)
    for s in range(STEPS2):
        sgns_accumulate(ref.w_in, ref.w_out, ref.g_in, ref.g_out, K2, walks=walks[s].cuda(),
                        context_radius=R2, seed=11, noise_offset=s * NW2 * per, loss_acc=acc_ref)
        ref.step()
    torch.cuda.synchronize()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lazy_run, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    errs = [r[4] for r in res if r[4]]
    assert not errs, errs
    (_, i0, o0, a0, _, s0), (_, i1, o1, a1, _, s1) = res
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(o0, o1)
    np.testing.assert_allclose(a0 + a1, acc_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    for a, b in zip(s0, s1):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    from stepcheck import check_trajectory
    worst = check_trajectory('owner lazy 2 ranks', _init2(), s0, _walks_all(), R2, K2, 11, LR2,
                             NW2 * (L2 - 2 * R2))
    print({k: round(v, 3) for k, v in sorted(worst.items())})


@pytest.mark.parametrize('W,mode', [(1, 'acc'), (1, 'fused'), (1, 'lazy'), (3, 'acc'),
                                    (3, 'fused'), (3, 'lazy'), (1, 'bad')])
def test_owner_pass2_without_count_readback(hip_device, W, mode):
    """read_count=False (n_records NULL): no host synchronisation — the sort runs over the slot
    bound with the tail padded past every row and the gather is limited on the device
    (k_rec_pad). One owner keeps every slot, so the records and their chunking are those of the
    counted call: bit-exact, but for the hub row, whose records span several gather chunks and
    are summed by atomics in no fixed order (so two counted calls differ there as well). With
    W = 3 (or dropped bad ids) the tail is padded and the chunk size follows the bound: equal up
    to the boundary rows' summation order."""
    from shallow_encoders.word2vec.sharding import adam_scalars
    from shallow_encoders.word2vec.graphed import adam_history
    rng = np.random.default_rng(W * 7 + len(mode))
    V, d, R, K, L, n = 2500, 128, 3, 4, 20, 48
    S = -(-V // W)
    w_in = torch.as_tensor(sgns_ref.xavier_tables(V, d, seed=4)[0]).cuda()
    base = torch.randn((S, d), generator=torch.Generator().manual_seed(2)).cuda() * 0.1
    walks = torch.as_tensor(rng.integers(0, V, size=(n, L)).astype(np.int32)).cuda()
    walks[:, ::5] = 17                      # a hub row straddling gather chunks
    if mode == 'bad':
        walks[3, 7] = V + 5
    hist = torch.as_tensor(adam_history(4, 0.02, (0.9, 0.999), 1e-8, 0.0)).cuda()
    outs = []
    for read in (True, False):
        w, g = base.clone(), torch.zeros_like(base)
        m, v = torch.zeros_like(base), torch.zeros_like(base)
        flags = torch.zeros(S, dtype=torch.uint8, device='cuda')
        last = torch.zeros(S, dtype=torch.int32, device='cuda')
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        g_in = torch.zeros_like(w_in)
        sgns_owner_pass1(w_in, w, g_in, K, walks=walks, context_radius=R, owner=W - 1,
                         n_owners=W, vocab_size=V, seed=5, noise_offset=0, status=status)
        spec = {'acc': None, 'bad': None,
                'fused': {'m': m, 'v': v, 'flags': flags,
                          'scalars': adam_scalars(1, 0.02, (0.9, 0.999), 1e-8, 0.0)},
                'lazy': {'m': m, 'v': v, 'last': last, 'hist': hist, 'step': 1}}[mode]
        r = sgns_owner_pass2(w_in, w, g, K, walks=walks, context_radius=R, out_adam=spec,
                             status=status, read_count=read)
        torch.cuda.synchronize()
        assert (r is None) == (not read)
        outs.append((w, g, m, v, flags, last, int(status.item())))
    (w1, g1, m1, v1, f1, l1, s1), (w2, g2, m2, v2, f2, l2, s2) = outs
    assert s1 == s2 and ((s1 != 0) == (mode == 'bad'))
    assert torch.equal(f1, f2) and torch.equal(l1, l2)
    if W == 1 and mode != 'bad':
        rest = torch.ones(S, dtype=torch.bool, device='cuda')
        rest[17] = False
        for a, b in ((w1, w2), (g1, g2), (m1, m2), (v1, v2)):
            assert torch.equal(a[rest], b[rest])
    scale = float(g1.abs().max()) + 1e-30
    torch.testing.assert_close(g2, g1, rtol=1e-5, atol=1e-6 * scale)
    torch.testing.assert_close(m2, m1, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(w2, w1, rtol=1e-5, atol=1e-5 * 0.02)


@pytest.mark.parametrize('n_walks', [3, 150, 400])
def test_owner_prepare_touched_rows(hip_device, n_walks):
    """dw_sgns_owner_prepare's distinct centre nodes (sorted) and their count: the one-block path
    (<= 8,192 centres: k_occ_small) and the device-wide sort + unique above it; pass 1 with
    order_ready=True then equals pass 1 ordering its centres itself."""
    from shallow_encoders.word2vec.sgns import sgns_owner_prepare
    g = torch.Generator().manual_seed(n_walks)
    V, d, R, K, L = 700, 64, 3, 2, 30
    walks = torch.randint(1, V, (n_walks, L), generator=g, dtype=torch.int32)
    walks[:, ::7] = 5                                   # a repeated hub centre
    walks = walks.cuda()
    n_c = n_walks * (L - 2 * R)
    touched = torch.full((n_c,), -1, dtype=torch.int32, device='cuda')
    n_t = torch.zeros(1, dtype=torch.int64, device='cuda')
    sgns_owner_prepare(walks, R, K, V, V, touched=touched, n_touched=n_t)
    exp = torch.unique(walks[:, R:L - R].reshape(-1).long())
    k = int(n_t.item())
    assert k == exp.numel()
    assert torch.equal(touched[:k].long(), exp)
    w_in = torch.randn((V, d), generator=g).cuda() * 0.1
    w_out = torch.randn((V, d), generator=g).cuda() * 0.1
    res = []
    for ready in (True, False):
        if ready:
            sgns_owner_prepare(walks, R, K, V, V, touched=touched, n_touched=n_t)
        g_in = torch.zeros_like(w_in)
        acc = sgns_owner_pass1(w_in, w_out, g_in, K, walks=walks, context_radius=R, owner=0,
                               n_owners=1, vocab_size=V, seed=4, noise_offset=0,
                               order_ready=ready)
        res.append((g_in, acc))
    torch.cuda.synchronize()
    # (a hub's run of centres spans several waves: its row's atomics may add in either order)
    torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-12, atol=0)


@pytest.mark.parametrize('d', [64, 128])
def test_placed_records_equal_sorted_records(hip_device, d):
    """The one-rank lazy out slice with the records placed by the claim (no sort) and the p-only
    catch-up equals the form with the records sorted and the full catch-up: every row stepped at
    the same steps (last_out equal) and the tables equal up to the order a row's records are
    summed in (the claim's CAS order vs the sort's node order)."""
    V, R, K, L, n, steps, lr = 3000, 2, 4, 14, 24, 8, 0.02
    walks = torch.randint(1, V, (steps, n, L), generator=torch.Generator().manual_seed(17),
                          dtype=torch.int32)

    def sorted_full(t):
        t.place = False
        t._wd_seen = True   # full catch-up (the form weight decay needs)
    runs = []
    for cfg in (None, sorted_full):
        t, acc = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=True, configure=cfg)
        assert t.out_flags() == (7 if cfg is None else 0)
        runs.append((t.last_out.clone(), t.w_in.cpu().numpy(), t.full_w_out().cpu().numpy(),
                     acc.cpu().numpy()))
    (l0, i0, o0, a0), (l1, i1, o1, a1) = runs
    assert torch.equal(l0, l1)
    np.testing.assert_allclose(a0, a1, rtol=1e-6)
    for got, exp in ((i0, i1), (o0, o1)):
        assert_params_close(got, exp, lr, rtol=1e-5, atol=1e-6, max_frac=1e-3,
                            max_abs=2.05 * lr * steps)
        assert_no_row_drift(got, exp)


@pytest.mark.parametrize('d,wd,hub', [(64, 0.0, False), (128, 0.0, True), (128, 0.01, False),
                                      (256, 0.0, True)])
def test_rows_major_equals_gather_path(hip_device, d, wd, hub):
    """The rows-major lazy out step (dw_sgns_owner_out_rows: each touched out row replayed,
    its records' logits / coefficients, its gradient and Adam step in one pass, then the
    centre gradient from the coefficients) equals the catch-up -> pass 1 -> lazy gather path:
    the same rows stepped at the same steps (last_out), the losses to float64 order and the
    tables to the order a row's records are summed in (the claim's atomics). hub: a few nodes
    fill a third of the walks, so their rows hold hundreds of records and straddle chunks
    (float atomics into g_out, k_lazy_boundary's full replay)."""
    V, R, K, L, n, steps, lr = 4000, 2, 4, 14, 32, 8, 0.02
    g = torch.Generator().manual_seed(23)
    walks = torch.randint(1, V, (steps, n, L), generator=g, dtype=torch.int32)
    if hub:
        mask = torch.rand((steps, n, L), generator=g) < 0.33
        walks[mask] = torch.randint(1, 4, (int(mask.sum()),), generator=g, dtype=torch.int32)
    runs = []
    for rows_major in (True, False):
        def cfg(t, rows_major=rows_major):
            t.rows_major = rows_major
        t, acc = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=True, wd=wd,
                                configure=cfg)
        assert t._rows_step == rows_major
        runs.append((t.last_out.clone(), t.w_in.cpu().numpy(), t.full_w_out().cpu().numpy(),
                     acc.cpu().numpy()))
    (l0, i0, o0, a0), (l1, i1, o1, a1) = runs
    assert torch.equal(l0, l1)
    np.testing.assert_allclose(a0, a1, rtol=1e-6)
    # hub rows hold hundreds of records summed in the claim's (run-dependent) order; each
    # near-zero gradient entry then moves by up to a normalised Adam step: 1,026 of 1,024,000
    # entries (0.1002%) measured once at d = 256 — the exact comparison is the deterministic
    # test below
    frac = 2e-3 if hub else 1e-3
    for got, exp in ((i0, i1), (o0, o1)):
        assert_params_close(got, exp, lr, rtol=1e-5, atol=1e-6, max_frac=frac,
                            max_abs=2.05 * lr * steps)
        assert_no_row_drift(got, exp)


@pytest.mark.parametrize('d', [128, 256])
def test_rows_major_equals_gather_path_deterministic(hip_device, d):
    """test_rows_major_equals_gather_path's hub case in the deterministic mode (integer sums:
    no record order left): the rows-major step and the catch-up -> pass 1 -> lazy gather path
    give the same tables and Adam state bit for bit."""
    V, R, K, L, n, steps, lr = 4000, 2, 4, 14, 32, 8, 0.02
    g = torch.Generator().manual_seed(23)
    walks = torch.randint(1, V, (steps, n, L), generator=g, dtype=torch.int32)
    mask = torch.rand((steps, n, L), generator=g) < 0.33
    walks[mask] = torch.randint(1, 4, (int(mask.sum()),), generator=g, dtype=torch.int32)
    per = L - 2 * R
    runs = []
    for rows_major in (True, False):
        def cfg(t, rows_major=rows_major):
            t.rows_major = rows_major
            t.enable_exact(1.0 / (n * per * 2 * R))
        t, _ = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=True, configure=cfg)
        assert t._rows_step == rows_major
        t.flush()
        runs.append([x[:V].cpu().clone() for x in (t.params_in[0], t.m_in, t.v_in, t.w_out,
                                                   t.m_out, t.v_out, t.last_out)])
    names = ('w_in', 'm_in', 'v_in', 'w_out', 'm_out', 'v_out', 'last_out')
    for name, x, y in zip(names, *runs):
        diff = int((x != y).sum())
        assert diff == 0, f'{name}: {diff} entries differ between the two forms'


def test_owner_tables_refuse_unbuilt_width(hip_device):
    """d = 192 is a multiple of 64, but the owner passes' kernels (k_sgns_g16's owner and
    coefficient-input forms, k_out_rows) are built for d in {64, 128, 256, 512} only (ADVICE
    r04): the owner tables refuse other widths when they are made, before any step could leave
    the claim or counts changed, and the C ABI says why (no stale error text)."""
    from shallow_encoders.word2vec.sgns import sgns_owner_pass1
    from shallow_encoders.word2vec.sharding import OwnerLazyTables, OwnerTables
    for cls, kw in ((OwnerTables, {}), (OwnerLazyTables, {'lazy_out': True})):
        with pytest.raises(ValueError, match='owner layout needs d in'):
            cls(3000, 192, hip_device, lr=0.01, init_seed=4, **kw)
    V, d = 3000, 192
    w_in = torch.zeros((V, d), device=hip_device)
    walks = torch.randint(1, V, (4, 12), dtype=torch.int32).to(hip_device)
    with pytest.raises(_native.DWError, match=r'd in \{64, 128, 256, 512\} \(got 192\)'):
        sgns_owner_pass1(w_in, torch.zeros_like(w_in), torch.zeros_like(w_in), 3, walks=walks,
                         context_radius=2, owner=0, n_owners=1, vocab_size=V, seed=1,
                         noise_offset=0)


@pytest.mark.parametrize('d,wd', [(128, 0.0), (64, 0.01)])
def test_rows_major_bit_identical_without_collisions(hip_device, d, wd):
    """Where no two records of a step share an out row and no two centres share a node, nothing
    depends on the order of atomics, and the rows-major step equals the catch-up -> pass 1 ->
    lazy gather path bit for bit — the same logits (pass 1's 16-lane layout and FMA order),
    coefficients, gradient sums, replays and Adam steps. Walks of length 2R + 1 (one centre
    each) over distinct nodes, and none of a step's negatives (oracle.philox.device_noise, the
    device's draws) among its contexts or each other."""
    from oracle.philox import device_noise
    V, R, K, L, n, steps, lr = 2_000_000, 2, 2, 5, 16, 6, 0.02
    g = torch.Generator().manual_seed(5)
    walks = torch.empty((steps, n, L), dtype=torch.int32)
    for s in range(steps):
        neg = device_noise(11, s * n, n, 2 * R, K, V).ravel()   # _lazy_vs_dense's seed, offsets
        assert np.unique(neg).size == neg.size
        pool = torch.randperm(V - 1, generator=g)[:4 * n * L].add_(1)
        pool = pool[~torch.from_numpy(np.isin(pool.numpy(), neg))][:n * L]
        walks[s] = pool.view(n, L).to(torch.int32)
    runs = []
    for rows_major in (True, False):
        def cfg(t, rows_major=rows_major):
            t.rows_major = rows_major
        t, acc = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=True, wd=wd,
                                configure=cfg)
        assert t._rows_step == rows_major
        runs.append((t.last_out.clone(), t.w_in.cpu(), t.full_w_out().cpu(), acc.cpu()))
    (l0, i0, o0, a0), (l1, i1, o1, a1) = runs
    assert torch.equal(l0, l1)
    # (the loss terms are summed per lane in fp32, grouped differently by the two paths)
    torch.testing.assert_close(a0, a1, rtol=1e-6, atol=0)
    assert torch.equal(i0.view(torch.int32), i1.view(torch.int32))
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32))


@pytest.mark.parametrize('wd_head', [False, True])
def test_adam_reciprocal_division_bit_identical(hip_device, wd_head):
    """The replays' fast forms give the scaled IEEE sequences' bits: dw::div_bc2s (sqrt(v) /
    sqrt(bias_correction2) through the host's correctly rounded reciprocal) and the box replay
    (dw::replay_g0: sqrt and the division without range scaling while every operand stays in the
    box, from the step the history's row 0 names: sharding.hist_header) against a history
    without the reciprocal (every step on the scaled path), over 40 replayed steps of rows
    lagging 0-39 steps. Rows: v spread over 80 binary orders of magnitude
    per element (waves falling back at the start or at the end of a run), row-scaled v and m
    (m down to ~1e-33: runs ending under the box's 2^-100 restart on the scaled path), fresh
    rows (m = v = +0), -0 entries in m, v past 2^20. wd_head: weight decay in steps 1-10 (the
    header's box starts at step 11: rows last current before step 10 take the scaled path)."""
    import numpy as np
    from shallow_encoders.word2vec.sharding import hip_rows_adam, hist_header, hist_row
    g = torch.Generator().manual_seed(2)
    n, d, steps = 8192, 128, 40
    h2 = n // 2
    p0 = torch.randn((n, d), generator=g)
    m0 = torch.randn((n, d), generator=g) * 1e-3
    v0 = torch.rand((n, d), generator=g) * torch.pow(10.0, -40 * torch.rand((n, d), generator=g))
    v0[::97] = 0.0
    row_v = torch.pow(10.0, -20 * torch.rand((n - h2, 1), generator=g))
    row_m = torch.pow(10.0, -30 * torch.rand((n - h2, 1), generator=g))
    v0[h2:] = torch.rand((n - h2, d), generator=g) * row_v
    m0[h2:] *= row_m
    m0[h2::7] = 0.0                               # fresh rows
    v0[h2::7] = 0.0
    m0[h2 + 1::11, ::5] = -0.0
    v0[h2 + 2::13, 3] = 4e6                       # v past 2^20
    last0 = torch.randint(0, steps, (n,), generator=g, dtype=torch.int32)
    hist = np.stack([hist_row(max(s, 1), 0.01, (0.9, 0.999), 1e-8,
                              0.01 if wd_head and s <= 10 else 0.0)
                     for s in range(steps + 1)])
    outs = []
    for recip in (True, False):
        h = hist.copy()
        if not recip:
            h[:, 7] = 0.0
        h[0] = hist_header(h, steps)
        assert h[0].view(np.int32)[1] == (steps + 1 if not recip else 11 if wd_head else 1)
        p, m, v, last = (x.clone().to(hip_device) for x in (p0, m0, v0, last0))
        hip_rows_adam(p, m, v, last, None, None, n, None, torch.from_numpy(h).to(hip_device),
                      steps)
        torch.cuda.synchronize()
        outs.append((p.cpu(), m.cpu(), v.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))   # bits (signed zeros)
