"""Every Adam entry point of dw_adam.hip, bit for bit against oracle/adam_ref.py: an independent
numpy restatement of the documented fp32 operation sequence (IEEE, gradual underflow, signed
zeros), validated on the CPU by tests/test_oracle_adam.py. The other Adam tests compare one HIP
kernel with another; a defect the kernels share (the device's denormal mode, a sqrt or division
that is not correctly rounded, an error in dw::adam_mv / adam_p) passes those and fails here.

All comparisons are on the uint32 words of every element of p, m and v (signed zeros count); where
an input holds NaN the NaN positions are compared, and the bits of everything else."""
import numpy as np
import pytest
import torch

from oracle import adam_ref as ar

pytestmark = pytest.mark.gpu

F32 = np.float32
SUB = 2.0 ** -149
EPS = 1e-8


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _assert_words(what, got, want):
    """got (a device tensor or an array) equals want word for word; NaNs by position."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, dtype=F32)
    assert got.dtype == F32 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f'{what}: NaN positions differ in {int((gn != wn).sum())}'
    diff = (ar.bits(got) != ar.bits(want)) & ~wn
    if diff.any():
        i = np.flatnonzero(diff.ravel())[0]
        raise AssertionError(
            f'{what}: {int(diff.sum())} of {diff.size} words differ; first at {i}: device '
            f'{got.ravel()[i]!r} ({ar.bits(got).ravel()[i]:#010x}), oracle '
            f'{want.ravel()[i]!r} ({ar.bits(want).ravel()[i]:#010x})')


def _signs(rng, n):
    return rng.choice(np.array([-1.0, 1.0]), n)


# ---- a. dw_adam_dense / dw_adam_dense_to (k_adam) ------------------------------------------------
N_GRID = 4 * (256 * 2 * 3 + 17) + 3      # three blocks' worth of U = 2 groups, a part, a tail


def _mixed_state(n, seed):
    """(p, g, m, v): values that take every branch of sqrt, the divisions and div_bc2s, mixed
    within a wave; elements [1024, 2048) (and [256, 512)) are tame, so that whole waves also take
    the reciprocal division."""
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=n) * 0.05).astype(F32)
    g = (10.0 ** rng.uniform(-45, 4, n) * _signs(rng, n)).astype(F32)
    m = (10.0 ** rng.uniform(-45, 2, n) * _signs(rng, n)).astype(F32)
    v = (10.0 ** rng.uniform(-45, 30, n)).astype(F32)
    kind = rng.integers(0, 16, n)
    v[kind == 0] = 0.0
    v[kind == 1] = np.inf
    m[kind == 2] = 0.0
    m[kind == 3] = -0.0
    g[kind == 4] = 0.0
    g[kind == 5] = -0.0
    g[kind == 6] = (1e18 * _signs(rng, n))[kind == 6]          # g^2 overflows
    g[kind == 7] = (rng.integers(1, 4000, n) * SUB)[kind == 7]
    p[kind == 8] = 0.0
    p[kind == 9] = -0.0
    m[kind == 10] = (rng.integers(1, 4000, n) * SUB * _signs(rng, n))[kind == 10]
    v[kind == 11] = (rng.integers(1, 4000, n) * SUB)[kind == 11]
    for lo, hi in ((256, 512), (1024, 2048)):
        k = max(0, min(hi, n) - lo)
        if k:
            v[lo:lo + k] = 10.0 ** rng.uniform(-30, 10, k)
            v[lo:lo + k:5] = 0.0
            g[lo:lo + k] = rng.normal(size=k) * 1e-3
            m[lo:lo + k] = rng.normal(size=k) * 1e-4
    if n > 1000:
        g[7] = np.nan
        m[900] = np.nan
    return p, g, m, v


@pytest.mark.parametrize('beta2', [0.999, 0.98])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, N_GRID])
def test_dense_adam_equals_oracle(hip_device, n, beta2):
    """k_adam's scalar tail, float4 body and U = 2 grid-stride loop (the grid capped to 1 and 3
    blocks, out of place), with and without weight decay and zero_grad, at steps where
    sqrt(bias_correction2) is small and near 1. dw_adam_dense_to always divides through the
    host's reciprocal (beta2 = 0.98 has no device proof of it: the oracle's quotient decides)."""
    from shallow_encoders.word2vec.sharding import hip_adam, hip_adam_to, hist_row
    betas = (0.9, beta2)
    p0, g0, m0, v0 = _mixed_state(n, 100 + n)
    for wd in (0.0, 0.01):
        for step in (1, 2, 1000):
            h = hist_row(step, 0.01, betas, EPS, wd)
            assert (h[7] != 0) == (beta2 == 0.999)
            want = ar.adam_step(p0, g0, m0, v0, h)
            for zero in (False, True):
                runs = [('in place', None, 0)]
                if n == N_GRID:
                    runs += [(f'to, max_blocks {b}', True, b) for b in (0, 1, 3)]
                for name, to, max_blocks in runs:
                    what = f'n={n} wd={wd} step={step} zero={zero} {name}'
                    p, g, m, v = (_dev(x) for x in (p0, g0, m0, v0))
                    if to:
                        dst = torch.full_like(p, 7.0)
                        hip_adam_to(p, dst, g, m, v, step, 0.01, betas, EPS, wd, zero,
                                    max_blocks)
                        torch.cuda.synchronize()
                        _assert_words(what + ' source', p, p0)      # the source is only read
                        p = dst
                    else:
                        hip_adam(p, g, m, v, step, 0.01, betas, EPS, wd, zero)
                        torch.cuda.synchronize()
                    for nm, a, b in zip('pmv', (p, m, v), want):
                        _assert_words(f'{what} {nm}', a, b)
                    if zero:
                        assert not ar.bits(g.cpu().numpy()).any(), what + ': g not cleared'
                    else:
                        _assert_words(what + ' g', g, g0)


# ---- b. DW_EXACT_ADAM (k_adam_fixed) -------------------------------------------------------------
@pytest.mark.parametrize('zero', [False, True])
@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_fixed_point_adam_equals_oracle(hip_device, wd, zero):
    """The dense Adam reading a registered deterministic-mode accumulator: g = from_fixed(acc),
    then the same step; the accumulator cleared under zero_grad, the float buffer never touched."""
    from shallow_encoders.word2vec import exact
    from shallow_encoders.word2vec.sharding import hip_adam, hist_row
    n = 4 * 300 + 3                       # two blocks of the float4 body and a tail
    rng = np.random.default_rng(5)
    p0, _, m0, v0 = _mixed_state(n, 6)
    acc0 = (rng.integers(1, 2 ** 62, n) >> rng.integers(0, 62, n)) * rng.choice([-1, 1], n)
    acc0[:8] = [0, 1, -1, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 61 + 12345, 0, 0]
    acc0[-3:] = [-1, 0, 2 ** 60 + 1]
    acc0[400:440] = 0                     # whole float4 groups with nothing to clear
    assert (np.abs(acc0) > 2 ** 53).sum() > 10
    g0 = np.full(n, 3.25, dtype=F32)      # the float buffer: neither read nor written
    p, g, m, v = (_dev(x) for x in (p0, g0, m0, v0))
    fx = exact.FixedAccumulator(g, 1.0, adam=True)
    try:
        fx.acc.copy_(_dev(acc0, np.int64))
        h = hist_row(3, 0.01, (0.9, 0.999), EPS, wd)
        want = ar.adam_step(p0, ar.from_fixed(acc0, fx.frac), m0, v0, h)
        hip_adam(p, g, m, v, 3, 0.01, (0.9, 0.999), EPS, wd, zero)
        torch.cuda.synchronize()
    finally:
        fx.release()
    for nm, a, b in zip('pmv', (p, m, v), want):
        _assert_words(f'fixed wd={wd} zero={zero} {nm}', a, b)
    _assert_words('the float gradient buffer', g, g0)
    np.testing.assert_array_equal(fx.acc.cpu().numpy(), np.zeros_like(acc0) if zero else acc0)


# ---- c. dw_adam_rows replays: a long lag through underflow ---------------------------------------
V_ROWS, S_LONG = 64, 3000
G_BOX, G_SUBN, G_UNITS = slice(0, 12), slice(12, 24), slice(24, 36)
R_MPOS, R_MNEG, R_PZERO, R_NEGZ, R_MIX = 36, 37, 38, 39, 40
DONE = slice(60, 64)                     # rows already at S


def _history(S, betas, lr_at, wd=0.0):
    from shallow_encoders.word2vec.sharding import hist_header, hist_row
    hist = np.zeros((S + 1, 8), dtype=F32)
    for s in range(1, S + 1):
        hist[s] = hist_row(s, lr_at(s), betas, EPS, wd)
    hist[0] = hist_header(hist, S)
    return hist


def _long_lag_state(d, seed):
    rng = np.random.default_rng(seed)
    V = V_ROWS
    p = (rng.normal(size=(V, d)) * 0.05).astype(F32)
    m = (rng.normal(size=(V, d)) * 1e-6).astype(F32)
    v = (rng.uniform(size=(V, d)) * 1e-9).astype(F32)                 # the ordinary rows
    v[G_BOX] = 2.0 ** rng.uniform(-95, -90, (12, d))                  # leave the box mid-run
    v[G_SUBN] = 2.0 ** rng.uniform(-126, -120, (12, d))               # go subnormal
    v[G_UNITS] = rng.integers(1, 5000, (12, d)) * SUB                 # subnormal from the start
    m[R_MPOS] = 0.0                                                   # the v-alone loop
    m[R_MNEG] = -0.0
    v[R_PZERO] = 2.0 ** rng.uniform(-95, -92, d)                      # p = +0 with m != 0 never
    p[R_PZERO, ::3] = 0.0                                             # freezes: the late fallback
    p[R_NEGZ, :8] = -0.0
    m[R_NEGZ, :8] = -0.0
    p[R_NEGZ, 8:12] = 0.0
    m[R_NEGZ + 2] = 0.0
    v[R_MIX, ::7] = rng.integers(1, 5000, v[R_MIX, ::7].shape) * SUB  # mixed within a wave
    v[R_MIX + 1, ::5] = 2.0 ** -93
    v[R_MIX + 3, 1::2] = 0.0
    last = rng.integers(0, 40, V)
    last[DONE] = S_LONG
    return p, m, v, last


def _header_forms(hist):
    """name -> row 0: as written, and the forms a replay must survive with the same bits."""
    from shallow_encoders.word2vec.sharding import HIST_BOX_TAG
    h0 = hist[0]
    never, vary, zeros = h0.copy(), h0.copy(), np.zeros(8, dtype=F32)
    never[2] = np.inf
    vary[4] = vary[5] = np.nan
    zeros.view(np.uint32)[0] = HIST_BOX_TAG       # the pre-freeze layout: tag, box_from, zeros
    zeros.view(np.uint32)[1] = h0.view(np.uint32)[1]
    return {'certified': h0.copy(), 'F=inf': never, 'betas NaN': vary,
            'no tag': np.zeros(8, dtype=F32), 'tag + zeros': zeros}


@pytest.mark.parametrize('d,sched,beta1', [(128, False, 0.9), (96, False, 0.9), (65, False, 0.9),
                                           (2, False, 0.9), (96, True, 0.9), (65, False, 0.5),
                                           (2, False, 0.9999)])
def test_rows_adam_long_lag_equals_oracle(hip_device, d, sched, beta1):
    """3000 missed g = 0 steps a row: v leaves the box, goes subnormal and reaches the fixed
    points of the multiplication, m sticks at 4 units of 2^-149 — under every header form. d: two
    waves of pairs, pairs with dead lanes, the odd-d path, a single pair. sched: the lr changes at
    steps 300 and 2000. beta1 = 0.5: m halves and does reach +0 (a tie to even); it satisfies
    beta1 (1 + 2^-20) <= sqrt(beta2), so its header still certifies a finite F. beta1 = 0.9999
    exceeds sqrt(beta2): sharding.hist_header itself writes F = +inf.
    The "tag + zeros" header (F = 0, betas 0 as read) froze every p != 0 before dw::hist_freeze
    refused such an F: 3840 of 8192 p words differed at d = 128, 2880 of 6144 at d = 96, 60 of
    128 at d = 2; the odd d = 65 (no frozen tail) was equal."""
    from shallow_encoders.word2vec.sharding import hip_rows_adam
    S = S_LONG
    betas = (beta1, 0.999)
    lr_at = (lambda s: 0.01 if s < 300 else (0.004 if s < 2000 else 0.02)) if sched \
        else (lambda s: 0.01)
    hist = _history(S, betas, lr_at)
    assert hist[0].view(np.int32)[1] == 1                       # every step is in the box
    if beta1 > np.sqrt(0.999):
        assert np.isposinf(hist[0, 2])
    else:
        assert np.isfinite(hist[0, 2]) and hist[0, 2] > 0       # the freeze is certified
    p0, m0, v0, last0 = _long_lag_state(d, 7 * d + int(sched))
    mid = ar.replay_g0(p0, m0, v0, hist, last0, 40)
    pS, mS, vS = ar.replay_g0(*mid, hist, np.maximum(last0, 40), S)
    # the regimes, on the oracle's own trajectory
    v40, b2 = mid[2], F32(hist[1, 1])
    assert ((v40[G_BOX] >= 2.0 ** -96) & (vS[G_BOX] < 2.0 ** -96)).any()     # left the box late
    assert ((v40[R_PZERO] >= 2.0 ** -96) & (vS[R_PZERO] < 2.0 ** -96)
            & (p0[R_PZERO] == 0) & (m0[R_PZERO] != 0)).any()
    assert ((vS[G_SUBN] > 0) & (vS[G_SUBN] < 2.0 ** -126)).any()              # subnormal v
    assert ((vS[G_UNITS] > 0) & (vS[G_UNITS] * b2 == vS[G_UNITS])).any()      # v's fixed point
    assert (vS[G_UNITS] <= F32(500 * SUB)).all()
    if beta1 == 0.9:
        assert (np.abs(mS[G_UNITS]) == F32(4 * SUB)).any()                    # m's fixed point
        assert (mS[:R_MPOS] != 0).all()                                       # m never reaches 0
    if beta1 == 0.5:
        assert not ar.bits(mS[:DONE.start]).any()                             # m did reach +0
    assert not ar.bits(mS[[R_MPOS, R_MNEG]]).any()
    for x, y in zip((pS, mS, vS), (p0, m0, v0)):
        assert np.array_equal(ar.bits(x[DONE]), ar.bits(y[DONE]))
    for name, h0 in _header_forms(hist).items():
        h = hist.copy()
        h[0] = h0
        p, m, v = (_dev(x) for x in (p0, m0, v0))
        last = _dev(last0, np.int32)
        hip_rows_adam(p, m, v, last, None, None, V_ROWS, None, _dev(h), S)
        torch.cuda.synchronize()
        for nm, a, b in zip('pmv', (p, m, v), (pS, mS, vS)):
            _assert_words(f'd={d} header "{name}" {nm}', a, b)
        assert (last == S).all()


# ---- d. dw_adam_rows gradient step (STEP, BY_ROW) -------------------------------------------------
@pytest.mark.parametrize('by_row', [False, True])
@pytest.mark.parametrize('d,wd', [(128, 0.0), (65, 0.0), (96, 0.01)])
def test_rows_adam_gradient_step_equals_oracle(hip_device, d, wd, by_row):
    """Listed rows with a device count below n_rows_max and one id past the table: the replay to
    step - 1 (lags 0, 1, 37), then the step with the row's gradient (+-0 and subnormals in it)."""
    from shallow_encoders.word2vec.sharding import hip_rows_adam
    V, step = 40, 60
    rng = np.random.default_rng(d + by_row)
    hist = _history(step, (0.9, 0.999), lambda s: 0.01 if s < 30 else 0.003, wd)
    p0 = rng.normal(size=(V, d)).astype(F32)
    m0 = (rng.normal(size=(V, d)) * 1e-2).astype(F32)
    v0 = (rng.uniform(size=(V, d)) * 1e-3).astype(F32)
    p0[5, :3] = [0.0, -0.0, 0.0][:min(3, d)]
    listed = np.array([3, 17, 1000, 5, 9, 20, 21, 22], dtype=np.int32)   # 1000: past the table
    n_dev, n_max = 6, 8                                                   # 21, 22: past the count
    used = np.array([3, 17, 5, 9, 20])
    last0 = rng.integers(0, step, V)
    last0[[3, 17, 5, 9, 20]] = [step - 1, step - 2, step - 38, step - 1, step - 2]   # the lags
    last0[21] = 4
    G = rng.normal(size=(V if by_row else n_max, d)).astype(F32)
    G[:, ::4] = 0.0
    G[:, 1::8] = -0.0
    G[:, 2::8] = (rng.integers(1, 3000, G[:, 2::8].shape) * SUB
                  * _signs(rng, G[:, 2::8].shape)).astype(F32)
    g_of = {r: G[r] if by_row else G[i] for i, r in enumerate(listed[:n_dev]) if r < V}
    assert sorted(g_of) == sorted(used)
    pw, mw, vw = ar.replay_g0(p0, m0, v0, hist, np.where(np.isin(np.arange(V), used), last0,
                                                          step), step - 1)
    for r in used:
        pw[r], mw[r], vw[r] = ar.adam_step(pw[r], g_of[r], mw[r], vw[r], hist[step])
    p, m, v, g = (_dev(x) for x in (p0, m0, v0, G))
    last = _dev(last0, np.int32)
    hip_rows_adam(p, m, v, last, _dev(listed), _dev(np.array([n_dev]), np.int64), n_max, g,
                  _dev(hist), step, grad_by_row=by_row)
    torch.cuda.synchronize()
    for nm, a, b in zip('pmv', (p, m, v), (pw, mw, vw)):
        _assert_words(f'{nm}', a, b)            # the whole table: no other row was written
    lw = last0.copy()
    lw[used] = step
    np.testing.assert_array_equal(last.cpu().numpy(), lw)
    Gw = G.copy()
    if by_row:
        Gw[used] = 0.0                          # the used gradient rows are cleared, all bits
    _assert_words('gradient rows', g, Gw)


# ---- e. pending rows (dw::settle_pending) through dw_adam_rows(pending=...) ------------------------
@pytest.mark.parametrize('late_box', [False, True])
@pytest.mark.parametrize('lag', [0, 5, 300])
@pytest.mark.parametrize('d', [128, 65])
def test_rows_adam_settles_pending_rows(hip_device, d, lag, late_box):
    """A row the rows-major out step left pending holds (m, v) of step a and p of a - 1: the
    flush applies the parameter half of a, then the g = 0 steps — the oracle's full step a and
    its replay. Rows whose (m, v) are inside the box take the unscaled branch, rows outside it
    (v < 2^-96, |m| < 2^-100, v > 2^20) and every row under a header whose box starts after a
    (late_box) the scaled one."""
    from shallow_encoders import _native
    from shallow_encoders.word2vec.sharding import hip_rows_adam
    V, a = 32, 400
    S = a + lag
    rng = np.random.default_rng(10 * d + lag)
    hist = _history(S, (0.9, 0.999), lambda s: 0.01)
    assert hist[0].view(np.int32)[1] == 1
    if late_box:
        hist[0].view(np.int32)[1] = a + 1       # still true of every row from a + 1 on
    p0 = (rng.normal(size=(V, d)) * 0.05).astype(F32)
    mp = (rng.normal(size=(V, d)) * 1e-4).astype(F32)
    vp = (rng.uniform(size=(V, d)) * 1e-7).astype(F32)
    g = (rng.normal(size=(V, d)) * 1e-2).astype(F32)
    g[:, ::5] = 0.0
    p0[2, :2] = [0.0, -0.0]
    small_v, small_m, big_v, mixed = [8, 9], [10, 11], [12, 13], 14
    for r in small_v:                            # v below 2^-96
        vp[r], g[r] = 2.0 ** rng.uniform(-110, -100, d), rng.normal(size=d) * 1e-20
    for r in small_m:                            # |m| below 2^-100
        mp[r], g[r] = rng.normal(size=d) * 1e-34, rng.normal(size=d) * 1e-34
    for r in big_v:                              # v above 2^20
        g[r] = rng.normal(size=d) * 1e5 + 3e4
    vp[mixed, ::9] = 2.0 ** -105                 # one outside element sends its wave
    g[mixed, ::9] = 1e-25
    pend0 = np.ones(V, dtype=np.uint8)
    last0 = np.full(V, a)
    pend0[[20, 21, 22]] = 0                      # not pending: plain replays from their steps
    last0[[20, 21, 22]] = [a - 7, S, max(a - 300, 0)]
    ha = hist[a]
    m0, v0 = ar.adam_mv(p0, g, mp, vp, ha)       # the moment half of step a, everywhere
    m0[~pend0.astype(bool)], v0[~pend0.astype(bool)] = mp[pend0 == 0], vp[pend0 == 0]
    inside = ((v0 == 0) | ((v0 >= 2.0 ** -96) & (v0 <= 2.0 ** 20))) & \
        ((m0 == 0) | ((np.abs(m0) >= 2.0 ** -100) & (np.abs(m0) <= 2.0 ** 60)))
    assert inside[[0, 1, 2, 3]].all() and (v0[small_v] < 2.0 ** -96).all()
    assert (np.abs(m0[small_m]) < 2.0 ** -100).any() and (v0[big_v] > 2.0 ** 20).any()
    assert 0 < (~inside[mixed]).sum() < d
    listed = np.array([0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 20, 21, 22, 77, 5, 6], np.int32)
    n_dev = 15                                   # 77: past the table; 5, 6: past the count
    used = listed[:n_dev][listed[:n_dev] < V]
    pw, mw, vw = p0.copy(), m0.copy(), v0.copy()
    settle = used[pend0[used] == 1]
    pw[settle] = ar.adam_p(p0[settle], m0[settle], v0[settle], ha)
    lw = np.where(np.isin(np.arange(V), used), last0, S)
    pw, mw, vw = ar.replay_g0(pw, mw, vw, hist, lw, S)
    full = ar.adam_step(p0[settle], g[settle], mp[settle], vp[settle], ha)   # = one full step a
    first = ar.replay_g0(*full, hist, np.full(settle.size, a), S)
    for x, y in zip(first, (pw, mw, vw)):
        assert np.array_equal(ar.bits(x), ar.bits(y[settle]))
    p, m, v = (_dev(x) for x in (p0, m0, v0))
    last, pend = _dev(last0, np.int32), _dev(pend0)
    hd = _dev(hist)
    hip_rows_adam(p, m, v, last, _dev(listed), _dev(np.array([n_dev]), np.int64), listed.size,
                  None, hd, S, pending=pend)
    torch.cuda.synchronize()
    for nm, x, y in zip('pmv', (p, m, v), (pw, mw, vw)):
        _assert_words(f'd={d} lag={lag} late_box={late_box} {nm}', x, y)
    lastw, pendw = last0.copy(), pend0.copy()
    lastw[used] = np.maximum(last0[used], S)
    pendw[used] = 0
    np.testing.assert_array_equal(last.cpu().numpy(), lastw)
    np.testing.assert_array_equal(pend.cpu().numpy(), pendw)    # cleared on the listed rows only
    # a gradient step on pending rows is refused with its status, and nothing is launched
    before = [t.clone() for t in (p, m, v, last, pend)]
    with pytest.raises(_native.DWError, match=r'\(-1\).*pending rows are settled'):
        hip_rows_adam(p, m, v, last, _dev(listed), None, listed.size,
                      torch.zeros((listed.size, d), device=p.device), hd, S, pending=pend)
    torch.cuda.synchronize()
    for x, y in zip(before, (p, m, v, last, pend)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
