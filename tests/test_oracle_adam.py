"""oracle/adam_ref.py on its own (CPU): the fp32 fused multiply-add against exact rational
arithmetic, the underflow fixed points of the g = 0 recurrences, signed zeros and inf, and the
formula against torch.optim.Adam at the project's single-step bars. The GPU kernels are compared
with this oracle bit for bit (tests/test_gpu_adam_ieee.py); the oracle stands on these tests."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import adam_ref as ar

F32 = np.float32
SUB = 2.0 ** -149                       # the smallest fp32 subnormal


def _hist_row(step, lr, betas, eps, wd):
    from shallow_encoders.word2vec.sharding import hist_row
    return hist_row(step, lr, betas, eps, wd)


def _rn32(x: Fraction) -> float:
    """The fp32 value nearest to the nonzero rational x, ties to even, gradual underflow,
    overflow to inf — in exact integer arithmetic."""
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)               # the spacing of fp32 at x
    n, r = divmod(x, q)
    n = int(n)
    if r > q / 2 or (r == q / 2 and n % 2 == 1):
        n += 1
    y = n * q
    if y >= Fraction(2) ** 128:
        return sign * float('inf')
    return sign * float(y)                               # exact: y is an fp32 value


def _check_fma(a, b, c):
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=F32) for x in (a, b, c)))
    keep = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    a, b, c = a[keep], b[keep], c[keep]
    assert a.size
    got = ar.fma32(a, b, c)
    want = np.empty_like(got)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        if exact == 0:      # IEEE's sign of an exact zero sum: float64 follows the same rule
            want[i] = F32(np.float64(a[i]) * np.float64(b[i]) + np.float64(c[i]))
        else:
            want[i] = _rn32(exact)
    return int((ar.bits(got) != ar.bits(want)).sum())


def _random_f32(rng, n):
    """Finite fp32 values with uniformly random sign, exponent and mantissa (subnormals and
    zeros included)."""
    u = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    x = u.view(F32)
    return x[np.isfinite(x)]


def test_fma32_equals_exact_rational_rounding():
    rng = np.random.default_rng(1)
    # the whole range: most sums are dominated by one operand, many over- or underflow
    a, b, c = (_random_f32(rng, 6000)[:5000] for _ in range(3))
    assert _check_fma(a, b, c) == 0
    # operands of similar size, so that the addition matters
    a = _random_f32(rng, 6000)[:5000]
    b = (rng.uniform(0.5, 2.0, 5000) * rng.choice([-1, 1], 5000)).astype(F32)
    with np.errstate(all='ignore'):
        c = (a * b * rng.uniform(-2.0, 2.0, 5000).astype(F32)).astype(F32)
    assert _check_fma(a, b, c) == 0
    # cancellation: c = -RN(a b), the result is the product's rounding error (often subnormal
    # or an exact zero)
    a = (rng.uniform(1.0, 2.0, 4000) * 2.0 ** rng.integers(-70, 20, 4000)).astype(F32)
    b = (rng.uniform(1.0, 2.0, 4000) * 2.0 ** rng.integers(-70, 20, 4000)).astype(F32)
    c = -(a * b)
    assert _check_fma(a, b, c) == 0
    # the kernels' lerp at g = 0, fma(w1, -m, m), over 1e-45 .. 1e3 and on the subnormals
    m = (10.0 ** rng.uniform(-45, 3, 4000) * rng.choice([-1, 1], 4000)).astype(F32)
    w1 = np.full(4000, 0.1, dtype=F32)
    assert _check_fma(w1, -m, m) == 0
    k = np.arange(-600, 601).astype(np.float64) * SUB
    assert _check_fma(np.full(k.size, 0.1, dtype=F32), -k.astype(F32), k.astype(F32)) == 0
    # results of +-0
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, SUB, 0.1], dtype=F32)
    y = np.array([1.0, 1.0, -1.0, -1.0, 0.0, -0.0, 0.25, -0.0], dtype=F32)
    w = np.array([0.0, 0.0, -0.0, -0.0, -0.0, 0.0, -0.0, 0.0], dtype=F32)
    assert _check_fma(z, y, w) == 0
    got = ar.bits(ar.fma32(z, y, w))
    np.testing.assert_array_equal(got >> 31, [0, 0, 1, 0, 0, 0, 0, 0])


def test_fma32_double_rounding_cases():
    """Sums that a float64 addition followed by a cast would round wrongly: the exact value
    sits within a float64 ulp of an fp32 tie while the float64 sum lands on the tie."""
    rng = np.random.default_rng(2)
    n = 500
    # c + c 2^-24 (1 + 2^-60): just above the tie over c; (1 + x)(1 - x + x^2) = 1 + x^3
    cm = rng.integers(2 ** 23, 2 ** 24, n)
    ce = rng.integers(-60, 60, n)
    c = (cm * 2.0 ** ce).astype(F32)                      # ulp(c) = 2^ce, half of it c's tie
    half = (2.0 ** (ce - 1)).astype(F32)
    a_up = np.full(n, 1.0 + 2.0 ** -12, dtype=F32) * half
    b_up = np.full(n, 1.0 - 2.0 ** -12 + 2.0 ** -24, dtype=F32)
    a_dn = np.full(n, 1.0 + 2.0 ** -23, dtype=F32) * half   # (1 + y)(1 - y) = 1 - y^2
    b_dn = np.full(n, 1.0 - 2.0 ** -23, dtype=F32)
    for a, b, up in ((a_up, b_up, True), (a_dn, b_dn, False)):
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))
        tie = c.astype(np.float64) + 2.0 ** (ce - 1.0)
        np.testing.assert_array_equal(naive, tie)         # the float64 sum is on the tie
        assert _check_fma(a, b, c) == 0
        got = ar.fma32(a, b, c)
        want = np.nextafter(c, F32(np.inf)) if up else c
        np.testing.assert_array_equal(ar.bits(got), ar.bits(want))
        # ... and the cast of the float64 sum (ties to even) gets the odd half of them wrong
        assert (ar.bits(naive.astype(F32)) != ar.bits(got)).sum() > n // 4
        # the mirrored signs
        assert _check_fma(-a, b, -c) == 0
    # 3 M 2^e with 3 M odd and 25 bits long: the product is a tie; c = +-2^-80 decides
    M = rng.integers(2 ** 23, (2 ** 25) // 3, n) | 1
    M = M[3 * M < 2 ** 25]
    b = M.astype(np.float64).astype(F32)
    a = np.full(b.size, 3.0, dtype=F32)
    for tiny in (2.0 ** -80, -2.0 ** -80, 0.0, SUB, -SUB):
        assert _check_fma(a, b, np.full(b.size, tiny, dtype=F32)) == 0
    up = ar.fma32(a, b, F32(2.0 ** -80))
    dn = ar.fma32(a, b, F32(-2.0 ** -80))
    np.testing.assert_array_equal(ar.bits(up), ar.bits(dn) + 1)
    # the same a binade above the subnormals' edge and inside them
    for sc in (2.0 ** -149, 2.0 ** -140):
        bs = (M.astype(np.float64) * sc).astype(F32)       # exact: M 2^-149 is subnormal
        assert _check_fma(np.full(bs.size, 0.5, dtype=F32), bs, F32(0.0)) == 0
        assert _check_fma(np.full(bs.size, 0.75, dtype=F32), bs, bs) == 0


def test_g0_fixed_points_under_gradual_underflow():
    """Under IEEE arithmetic m does not decay to +0: with 1 - beta1 = 0.1f, 5 units of 2^-149
    go to 4 and 4 stay; v stays for v <= 500 units under beta2 = 0.999f."""
    h = _hist_row(1000, 0.01, (0.9, 0.999), 1e-8, 0.0)
    assert h[0] == F32(0.1) and h[1] == F32(0.999)
    k = np.arange(0, 2000, dtype=np.float64)
    m = (k * SUB).astype(F32)
    v = (k * SUB).astype(F32)
    p = np.ones_like(m)
    _, m1, v1 = ar.adam_step_g0(p, m, v, h)
    km, kv = m1.astype(np.float64) / SUB, v1.astype(np.float64) / SUB
    assert km[5] == 4 and km[4] == 4 and km[1] == 1 and km[0] == 0
    np.testing.assert_array_equal(km[:5], k[:5])          # 0 .. 4 units map to themselves
    np.testing.assert_array_equal(kv[:501], k[:501])      # v <= 500 units stays
    assert kv[501] == 500 and (kv[501:] < k[501:]).all()
    assert (km[5:] < k[5:]).all()
    _, m2, _ = ar.adam_step_g0(p, -m, v, h)
    np.testing.assert_array_equal(ar.bits(m2[1:]), ar.bits(-m1[1:]))
    # a long run from an ordinary state ends on those fixed points, not on zero
    hist = np.zeros((3001, 8), dtype=F32)
    for s in range(1, 3001):
        hist[s] = _hist_row(s, 0.01, (0.9, 0.999), 1e-8, 0.0)
    p0 = np.full((1, 4), 0.05, dtype=F32)
    m0 = np.array([[1e-6, -1e-6, 3e-9, 0.0]], dtype=F32)
    v0 = np.array([[2.0 ** -125, 2.0 ** -123, 4000 * SUB, 0.0]], dtype=F32)
    _, mS, vS = ar.replay_g0(p0, m0, v0, hist, np.zeros(1, dtype=np.int64), 3000)
    np.testing.assert_array_equal(mS.astype(np.float64) / SUB, [[4, -4, 4, 0]])
    kv = vS.astype(np.float64)[0] / SUB
    # (0.999^3000 is only ~0.05: the first two go subnormal, the third reaches the fixed points)
    assert (kv[:2] >= 1).all() and (kv[:2] < 2.0 ** 23).all()
    assert 1 <= kv[2] <= 500 and kv[3] == 0


def test_replay_composes_and_g0_form_equals_full_step():
    from shallow_encoders.word2vec.sharding import hist_row
    rng = np.random.default_rng(3)
    S = 60
    for wd in (0.0, 0.01):
        hist = np.zeros((S + 1, 8), dtype=F32)
        for s in range(1, S + 1):
            hist[s] = hist_row(s, 0.01 if s < 30 else 0.002, (0.9, 0.999), 1e-8, wd)
        p = rng.normal(size=(9, 5)).astype(F32)
        m = (rng.normal(size=(9, 5)) * 1e-3).astype(F32)
        v = (rng.uniform(size=(9, 5)) * 1e-6).astype(F32)
        m[0, :2] = [0.0, -0.0]
        last = rng.integers(0, 20, 9)
        last[3] = S
        last[4] = S + 5
        a = ar.replay_g0(p, m, v, hist, last, S)
        mid = ar.replay_g0(p, m, v, hist, last, 25)
        b = ar.replay_g0(*mid, hist, np.maximum(last, 25), S)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
        for x, y in zip(a, (p, m, v)):                     # rows already current: untouched
            np.testing.assert_array_equal(ar.bits(x[3:5]), ar.bits(y[3:5]))
        # row by row, step by step through the full step with g = +0
        for r in (0, 1, 2):
            q = (p[r], m[r], v[r])
            for s in range(int(last[r]) + 1, S + 1):
                q = ar.adam_step(q[0], np.zeros(5, dtype=F32), q[1], q[2], hist[s])
            for x, y in zip(a, q):
                np.testing.assert_array_equal(ar.bits(x[r]), ar.bits(y))


def test_zeros_and_inf():
    h = _hist_row(3, 0.01, (0.9, 0.999), 1e-8, 0.0)
    nz, pz = F32(-0.0), F32(0.0)
    # m = -0 becomes +0 in one g = 0 step; y = nstep (m / denom) is then -0 (nstep < 0)
    p, m, v = ar.adam_step_g0([pz, nz, F32(1.5), nz], [nz, nz, nz, pz], [1e-9] * 4, h)
    np.testing.assert_array_equal(ar.bits(m), [0, 0, 0, 0])
    # p + (-0): +0 stays +0, -0 stays -0, 1.5 stays — a zero m never moves p, sign included
    np.testing.assert_array_equal(ar.bits(p), ar.bits(np.array([pz, nz, 1.5, nz], dtype=F32)))
    # the g = 0 form and the full step with g = +0 agree on every sign combination (gg - m is
    # +0 for m = +0 where -m is -0: fma's result is +0 either way, dw::adam_elem_g0's comment)
    for pv in (pz, nz):
        for mv in (pz, nz):
            a = ar.adam_step_g0([pv], [mv], [1e-9], h)
            b = ar.adam_step([pv], [pz], [mv], [1e-9], h)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
            assert ar.bits(a[0])[0] == ar.bits(pv) and ar.bits(a[1])[0] == 0
    # under a positive nstep (a negative lr) y is +0, and -0 + +0 = +0: p = -0 does move
    hneg = h.copy()
    hneg[4] = -hneg[4]
    p3, _, _ = ar.adam_step_g0([nz], [nz], [1e-9], hneg)
    assert ar.bits(p3)[0] == 0
    # v = +inf: denom = inf, m / denom = +-0, p unchanged; v stays inf
    pin = np.array([0.25, -3.0, pz], dtype=F32)
    p4, m4, v4 = ar.adam_step(pin, [1.0, -2.0, 0.5], [0.1, -0.1, 0.2], [np.inf] * 3, h)
    np.testing.assert_array_equal(ar.bits(p4), ar.bits(pin))
    assert np.isinf(v4).all()
    # v = +0 and m = +0: denom = eps, p unchanged
    p5, _, v5 = ar.adam_step_g0([0.5], [0.0], [0.0], h)
    assert p5[0] == F32(0.5) and ar.bits(v5)[0] == 0
    # from_fixed
    acc = np.array([0, 1, -1, 2 ** 53 + 1, -(2 ** 60) - 12345], dtype=np.int64)
    g = ar.from_fixed(acc, 40)
    want = [F32(float(Fraction(int(a), 2 ** 40))) for a in acc]     # Fraction -> double is RN
    np.testing.assert_array_equal(ar.bits(g), ar.bits(np.array(want, dtype=F32)))
    assert ar.bits(g)[0] == 0


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_oracle_agrees_with_torch_adam_at_the_single_step_bars(wd):
    """torch.optim.Adam(foreach=False) on the CPU, a few steps, rtol 1e-5 / atol 1e-6 (the bars
    of tests/stepcheck.py): a wrong formula fails this. It is not a bit-level reference: torch's
    CPU kernels do not round as this sequence does (20 steps on a 37 x 96 tensor differed from
    it in about a tenth of the words of p, m and v: 22,175 of 213,120)."""
    import torch
    rng = np.random.default_rng(4)
    lr, betas, eps = 0.01, (0.9, 0.999), 1e-8
    p = rng.normal(size=(37, 96)).astype(F32)
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    for s in range(1, 6):
        g = (rng.normal(size=p.shape) * 0.1).astype(F32)
        g[rng.uniform(size=p.shape) < 0.3] = 0.0
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = ar.adam_step(p, g, m, v, _hist_row(s, lr, betas, eps, wd))
        st = opt.state[tp]
        for name, a, b in (('p', p, tp.detach().numpy()), ('m', m, st['exp_avg'].numpy()),
                           ('v', v, st['exp_avg_sq'].numpy())):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=f'{name} step {s}')
