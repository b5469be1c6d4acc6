"""Every dispatch path of the fused SGNS step against the float64 closed form
(oracle.sgns_ref.sgns_grads_closed_form_pooled), at the smallest shapes that reach it.

A call is routed by the width d, the rows per centre T = C (1 + K), the input form (walks, pairs,
pooled), the scatter (sorted records or atomics), the batch size and the walk-aggregation mode:
  * k_sgns_g16<F4, ., CHR>: sorted scatter, d in {64, 128, 256, 512} (F4 = d / 64), T <= 64;
  * k_sgns<VPL, MASKED, FROM_WALKS, RECORDS>: everything else (VPL = ceil(d / 64) rounded up to
    1, 2, 4, 8; MASKED unless d = 64 VPL); T > 256 and every pooled call take the atomic form.

Bars (the project's float64 bar of test_fused_sgns_random_case_vs_oracle, test_gpu_exact.py and
test_gpu_sgns_walk_agg.py): gradients rtol 1e-4, atol 1e-6 * max |g_in| of the reference; the
three losses rel 1e-5; the recall / precision counts exact up to the number of logits inside
sgns_ref.SIGMOID_HALF_BAND (asserted 0 wherever the case is small enough to choose so).

Every case asserts in float64, before the GPU is touched, that no logit lies within 1e-3 of a
clamp boundary +-ln(10^6 - 1): a float32 dot product is off by at most d 2^-24 sum |c_i o_i|
(< 1e-5 at |x| ~ 14, d <= 512), so no term can be clamped on one side and not on the other. The
seeds are fixed and were chosen so; all of that part runs without a device
(`_reference(case)`)."""
import functools
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from oracle import philox as ph
from oracle import sgns_ref

from shallow_encoders import _native
from shallow_encoders.word2vec import sgns
from shallow_encoders.word2vec.sgns import loss_terms, set_walk_agg, sgns_accumulate

pytestmark = pytest.mark.gpu

SEED, OFFSET = 29, 4100          # device negatives (noise=None)


@dataclass(frozen=True)
class Case:
    form: str                    # 'pairs' | 'walks' | 'pooled'
    d: int
    K: int
    B: int = 0                   # pairs / pooled: centres, contexts per centre
    C: int = 0
    n: int = 0                   # walks: n walks of length L, radius R
    L: int = 0
    R: int = 0
    P: int = 1                   # pooled: input rows per centre
    V: int = 257
    npool: int = 24              # ids are drawn from this many rows (0: from all V)
    big: bool = False            # clamp tables (see _build)
    pool: str = 'mix'            # pooled: 'mix' | 'same' (one id P times) | 'shared'
    device_noise: bool = False   # the negatives are the device Philox draws
    seed: int = 0

    @property
    def T(self):
        return (self.C if self.form != 'walks' else 2 * self.R) * (1 + self.K)


def _build(case):
    """Tables and ids of a case (numpy). Ids come from a pool of ``npool`` rows that always
    holds rows 0 and V - 1 (the table's first and last bytes), so rows repeat across centres
    and within one centre's slots. ``big``: two thirds of the pool's rows, in both tables, are
    sign * norm * u + Xavier noise with norm in {3, 4, 5} and u one unit vector — logits between
    two of them are +-9 ... +-25 (both clamp branches at |x| > 13.8 and the saturated end), the
    rest Xavier; centre 0 is made a +5 row whose context 0 is a -5 row and whose negative 0 a +5
    row that nothing else touches (two output rows that only clamped terms touch), its context 1
    a +5 row and negative 1 a -5 row (x = +-25 on the unclamped side: `sy - 1.0f` = 0)."""
    c = case
    rng = np.random.default_rng([c.seed, c.d, c.T, c.B + c.n, c.P])
    w_in, w_out = sgns_ref.xavier_tables(c.V, c.d, seed=c.seed + c.d)
    if c.npool:
        pool = np.concatenate([[0, c.V - 1], rng.permutation(np.arange(1, c.V - 1))[:c.npool - 2]])
    else:
        pool = np.arange(c.V)
    draw = lambda *shape: pool[rng.integers(0, len(pool), shape)]  # noqa: E731
    out = {}
    if c.form == 'walks':
        walks = draw(c.n, c.L).astype(np.int32)
        inputs, targets = sgns_ref.sg_windows(walks, c.R)
        out['walks'] = walks
    else:
        inputs, targets = draw(c.B, c.P), draw(c.B, c.C)
        if c.pool == 'same':
            inputs[:] = inputs[:, :1]
        elif c.pool == 'shared':
            inputs[:, -1] = pool[2]
    B, C = targets.shape
    if c.device_noise:
        noise = ph.device_noise(SEED, OFFSET, B, C, c.K, c.V).reshape(B, C, c.K)
    else:
        noise = draw(B, C, c.K)
    if c.big:
        assert c.form != 'walks' and c.K >= 1 and c.npool >= 16
        u = rng.standard_normal(c.d)
        u /= np.linalg.norm(u)
        bigrows = pool[2:2 + 2 * c.npool // 3]
        spare = np.setdiff1d(np.arange(c.V), pool)[:5]     # rows no drawn id touches
        for tbl in (w_in, w_out):
            for r in bigrows:
                tbl[r] += (rng.choice([-1.0, 1.0]) * rng.choice([3.0, 4.0, 5.0]) * u) \
                    .astype(np.float32)
        w_in[spare[0]] += (5.0 * u).astype(np.float32)
        w_out[spare[1]] += (-5.0 * u).astype(np.float32)
        w_out[spare[2]] += (5.0 * u).astype(np.float32)
        w_out[spare[3]] += (5.0 * u).astype(np.float32)
        w_out[spare[4]] += (-5.0 * u).astype(np.float32)
        inputs[0, :] = spare[0]
        targets[0, 0], noise[0, 0, 0] = spare[1], spare[2]      # s = -25, t = +25: clamped
        targets[0, 1], noise[0, 0, 1] = spare[3], spare[4]      # s = +25, t = -25: saturated
        if c.P > 1:   # three contexts in four hold one row P times: pooled logits reach +-25
            same = np.arange(c.B) % 4 != 2
            inputs[same] = inputs[same, :1]
        out['only_clamped'] = spare[1:3]
    out.update(w_in=w_in, w_out=w_out, inputs=inputs, targets=targets, noise=noise)
    return out


@functools.lru_cache(maxsize=None)
def _reference(case, exact_band=True):
    """(data, float64 reference) of a case, computed once and shared by the tests that use it;
    asserts the clamp margin and (``exact_band``) that no logit is inside the sigmoid's
    half band — CPU only."""
    data = _build(case)
    ref = sgns_ref.sgns_grads_closed_form_pooled(data['w_in'], data['w_out'], data['inputs'],
                                                 data['targets'], data['noise'])
    _assert_bands(ref, exact_band)
    return data, ref


def _assert_bands(ref, exact_band=True):
    assert ref['clamp_margin'] >= 1e-3, ref['clamp_margin']
    if exact_band:
        assert ref['band_s'] == 0 and ref['band_t'] == 0, (ref['band_s'], ref['band_t'])


def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to('cuda', dtype)


def _status():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


def _kwargs(case, data, scatter):
    """sgns_accumulate's keyword arguments of the case's form."""
    kw = dict(scatter=scatter)
    if case.device_noise:
        kw.update(noise=None, seed=SEED, noise_offset=OFFSET)
    elif case.K > 0:
        kw.update(noise=_dev(data['noise'], torch.int64))
    if case.form == 'walks':
        kw.update(walks=_dev(data['walks'], torch.int32), context_radius=case.R)
    else:
        ins = data['inputs'] if case.form == 'pooled' else data['inputs'].reshape(-1)
        kw.update(inputs=_dev(ins, torch.int64), targets=_dev(data['targets'], torch.int64))
    return kw


def _launch(case, data, scatter, *, status=None):
    """One sgns_accumulate of the case's form; returns (g_in, g_out, acc)."""
    w_in, w_out = _dev(data['w_in']), _dev(data['w_out'])
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    acc = sgns_accumulate(w_in, w_out, g_in, g_out, case.K, status=status,
                          **_kwargs(case, data, scatter))
    torch.cuda.synchronize()
    return g_in, g_out, acc


def _compare(case, ref, g_in, g_out, acc, what=''):
    M = ref['s'].size
    t = loss_terms(acc, M, case.K)
    got = {k: float(v) for k, v in t.items()}
    gi, go = g_in.cpu().numpy(), g_out.cpu().numpy()
    scale = float(np.abs(ref['g_in']).max())
    with np.errstate(divide='ignore', invalid='ignore'):
        ea_in = np.nanmax(np.where(ref['A_in'] > 0, np.abs(gi - ref['g_in']) / ref['A_in'], 0))
        ea_out = np.nanmax(np.where(ref['A_out'] > 0, np.abs(go - ref['g_out']) / ref['A_out'], 0))
    print(f'{what} {case}: max|dg_in|/scale {np.abs(gi - ref["g_in"]).max() / scale:.3g} '
          f'max|dg_out|/scale {np.abs(go - ref["g_out"]).max() / scale:.3g} '
          f'max err/A in {ea_in:.3g} out {ea_out:.3g} '
          f'loss {got["loss"]:.9g} ref {ref["loss"]:.9g} acc {acc.tolist()}')
    for k in ('loss', 'positive-loss', 'negative-loss'):
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, got[k], ref[k])
    a = acc.cpu().numpy()
    assert abs(a[2] - ref['recall_count']) <= ref['band_s'], (a[2], ref['recall_count'])
    assert abs(a[3] - ref['neg_hit_count']) <= ref['band_t'], (a[3], ref['neg_hit_count'])
    if ref['band_s'] == 0 and ref['band_t'] == 0:   # (loss_terms rounds the ratios to float32)
        assert got['recall'] == pytest.approx(ref['recall'], abs=1e-6)
        assert got['precision'] == pytest.approx(ref['precision'], abs=1e-6)
    np.testing.assert_allclose(gi, ref['g_in'], rtol=1e-4, atol=1e-6 * scale)
    np.testing.assert_allclose(go, ref['g_out'], rtol=1e-4, atol=1e-6 * scale)
    return gi, go


def _check(case, scatter, exact_band=True):
    data, ref = _reference(case, exact_band)
    status = _status()
    g_in, g_out, acc = _launch(case, data, scatter, status=status)
    assert int(status.item()) == 0
    return data, ref, _compare(case, ref, g_in, g_out, acc, scatter)


@pytest.fixture
def walk_agg_mode():
    """set_walk_agg for one test, auto (or the environment's mode) restored afterwards."""
    try:
        yield set_walk_agg
    finally:
        set_walk_agg({'0': 0, '1': 1}.get(os.environ.get('DW_SGNS_WALK_AGG', ''), -1))


# ---- a. width sweep, 64-lane kernel --------------------------------------------------------------
@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
@pytest.mark.parametrize('d', [1, 2, 63, 65, 100, 129, 192, 257, 320, 384, 511])
def test_width_sweep_k_sgns(hip_device, d, scatter):
    """k_sgns<VPL, MASKED = true, pairs, RECORDS = (scatter == 'sorted')> at every masked width
    next to a full one: d = 1, 2, 63 (VPL 1), 65, 100 (VPL 2), 129 and the multiples of 64 the
    16-lane kernel refuses, 192 (VPL 4), 257, 320, 384, 511 (VPL 8). B = 7 centres of T = 6 rows
    (two blocks of four waves, the second with a single idle wave) is the smallest batch with
    more than one block; rows 0 and V - 1 are among the ids, so a lane past d would read or
    write the neighbouring row or past the table."""
    _check(Case('pairs', d, K=2, B=7, C=2, seed=1), scatter)


# ---- b. width sweep, 16-lane kernel --------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 5, 17])
@pytest.mark.parametrize('d', [64, 128, 256, 512])
def test_width_sweep_g16_pairs(hip_device, walk_agg_mode, d, B):
    """k_sgns_g16<F4 = d / 64, pairs, CHR = 8 / F4> (d = 512: F4 = 8, CHR = 1), T = 16 rows: one
    id per lane of a group. B = 1, 3: groups of a wave idle; B = 5: a second wave with one
    centre (B not divisible by 4: the group tail); B = 17: a second block."""
    walk_agg_mode(0)
    _check(Case('pairs', d, K=3, B=B, C=4, seed=2), 'sorted')


@pytest.mark.parametrize('agg', [0, 1])
@pytest.mark.parametrize('d', [64, 128, 256, 512])
def test_width_sweep_g16_walks(hip_device, walk_agg_mode, d, agg):
    """k_sgns_g16<F4, walks, CHR, OWNER = false, ., ., AGG = agg> at n = 3 walks of L = 9, R = 2,
    K = 2 (15 centres of T = 12 rows): without the walk aggregation, and with it wherever the
    library's predicate takes the shape (k_walk_agg's one and two and four column slices)."""
    case = Case('walks', d, K=2, n=3, L=9, R=2, seed=3)
    walk_agg_mode(agg)
    assert sgns.walk_agg_active(3, 9, 2, 2, d) == bool(agg)
    _check(case, 'sorted')


# ---- c. rows per centre --------------------------------------------------------------------------
# T = C (1 + K): one row; one and two 12-row chunks minus / plus one (T mod 12 in {11, 0, 1});
# 63 / 64 / 65 around the g16 limit and the 64-row group; 75 and 76 (a second group of 11 and of
# 12 rows); 128, 130; 255 / 256 / 258 around the records limit; 320 (five groups, atomic only).
T_SHAPES = {1: (1, 0), 2: (1, 1), 11: (1, 10), 12: (4, 2), 13: (1, 12), 63: (9, 6), 64: (4, 15),
            65: (5, 12), 75: (3, 24), 76: (4, 18), 128: (8, 15), 130: (10, 12), 255: (15, 16),
            256: (16, 15), 258: (6, 42), 320: (10, 31)}


@pytest.mark.parametrize('d', [64, 100])
@pytest.mark.parametrize('T', sorted(T_SHAPES))
def test_rows_per_centre_pairs(hip_device, d, T):
    """Pairs, B = 5, T from 1 (C = 1, K = 0) to 320, both scatters. d = 64: the last g16 shapes
    (T <= 64, sorted) and k_sgns<1, false> beyond and for atomics; d = 100: k_sgns<2, true>
    throughout. T > 64 runs k_sgns's row-group loop more than once (64 % 12 = 4: every full
    group ends in a ragged chunk; the last group is ragged by T mod 64 mod 12 in {0, 1, 4, 11});
    T > 256 (RECORDS_MAX_ROWS) must take the atomic path when 'sorted' is asked for."""
    C, K = T_SHAPES[T]
    case = Case('pairs', d, K=K, B=5, C=C, seed=4)
    assert case.T == T
    assert sgns._use_records('sorted', C, K, case.V) == (T <= 256)
    _, _, (gi_s, go_s) = _check(case, 'sorted')
    _, ref, (gi_a, go_a) = _check(case, 'atomic')
    scale = float(np.abs(ref['g_in']).max())
    np.testing.assert_allclose(gi_s, gi_a, rtol=1e-4, atol=1e-6 * scale)
    np.testing.assert_allclose(go_s, go_a, rtol=1e-4, atol=1e-6 * scale)


@pytest.mark.parametrize('R,K', [(1, 3), (1, 15), (4, 7), (8, 3), (4, 15), (8, 7), (8, 15),
                                 (8, 19)])
@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
def test_rows_per_centre_walks(hip_device, R, K, scatter):
    """Walks form at d = 128, n = 2 walks of L = 2R + 3 (3 centres each): T = 2R (1 + K) =
    8, 32, 64 (twice) on g16 (sorted) / k_sgns<2, false, walks> (atomic); 128 (twice) and 256 on
    k_sgns<2, false, walks, records>; 320 > RECORDS_MAX_ROWS on the atomic fallback."""
    _check(Case('walks', 128, K=K, n=2, L=2 * R + 3, R=R, seed=5), scatter)


# ---- d. grid stride ------------------------------------------------------------------------------
def _grid_case(kernel):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_block = 4 if kernel == 'k_sgns' else 16
    return Case('pairs', 65 if kernel == 'k_sgns' else 64, K=1, B=8 * cu * per_block + 5, C=2,
                V=4099, npool=0, seed=6)


@pytest.mark.parametrize('kernel', ['k_sgns', 'g16'])
def test_second_grid_stride_trip(hip_device, kernel):
    """Both pass-1 grids are capped at 8 blocks per CU: B = 8 CU * 4 + 5 centres (k_sgns, one
    centre per wave, d = 65) and 8 CU * 16 + 5 (g16, four per wave, d = 64) are the smallest
    batches whose last five centres are a second trip of the grid-stride loop — the loss partials
    carried in registers across trips. V = 4,099: every row collects about 30 records, so the
    sorted path's rows span its chunks. With ~10^5 logits a few may lie inside the sigmoid's half
    band; the metric counts may differ by that many (asserted)."""
    _check(_grid_case(kernel), 'sorted', exact_band=False)


# ---- e. clamp and saturation ---------------------------------------------------------------------
CLAMP_CASES = [Case('pairs', 64, K=3, B=17, C=4, big=True, seed=7),
               Case('pairs', 128, K=3, B=17, C=4, big=True, seed=7),
               Case('pairs', 100, K=3, B=17, C=4, big=True, seed=7),
               Case('pooled', 48, K=3, B=17, C=4, P=3, big=True, seed=7)]


@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
@pytest.mark.parametrize('case', CLAMP_CASES, ids=lambda c: f'{c.form}-d{c.d}')
def test_clamp_and_saturation(hip_device, case, scatter):
    """row_coef's three dead ends — sigmoid(s) < 1e-6 (positive, s < -13.8), sigmoid(-t) < 1e-6
    (negative, t > 13.8) and `sy - 1.0f` at x ~ 20 — on g16 (d = 64, 128, sorted), k_sgns (d =
    100; d = 64, 128 atomic) and the pooled path (P = 3, d = 48; always atomic). At least 5% of
    the positive and of the negative terms are clamped and some logit exceeds +-20 (asserted on
    the float64 logits); a clamped term's loss is ln 10^6 and its gradient absent, so the two
    output rows that only clamped terms touch stay bit-zero."""
    data, ref = _reference(case)
    assert ref['clamped_s'].mean() >= 0.05 and ref['clamped_t'].mean() >= 0.05
    assert ref['s'][0, 0] < -20 and ref['t'][0, 0, 0] > 20       # engineered: clamped
    assert ref['s'][0, 1] > 20 and ref['t'][0, 0, 1] < -20       # engineered: saturated
    only = data['only_clamped']
    assert not ref['A_out'][only].any()
    _, _, (gi, go) = _check(case, scatter)
    assert not go[only].view(np.int32).any()


# ---- f. pooled (CBOW) ----------------------------------------------------------------------------
POOLED = [(2, 2, 1, 0), (2, 10, 6, 3), (48, 3, 6, 3), (64, 2, 6, 70), (64, 10, 1, 3),
          (100, 3, 6, 70), (100, 2, 1, 0), (128, 2, 6, 3), (128, 10, 6, 0), (300, 3, 1, 70),
          (300, 2, 6, 3), (512, 10, 6, 3), (512, 3, 1, 70)]


@pytest.mark.parametrize('d,P,B,K', POOLED)
def test_pooled_pairs(hip_device, d, P, B, K):
    """dw_sgns_pooled_pairs = k_sgns<VPL, MASKED, pairs, atomic> with n_in = P > 1: VPL 1 masked
    (2, 48), full (64), VPL 2 masked (100) and full (128), VPL 8 masked (300) and full (512);
    C = 1, so T = 1, 4 and 71 rows (71: the pooled path's second row group); B = 1 and 6."""
    _check(Case('pooled', d, K=K, B=B, C=1, P=P, seed=18), 'sorted')


@pytest.mark.parametrize('pool', ['same', 'shared'])
@pytest.mark.parametrize('d', [64, 100])
def test_pooled_repeated_ids(hip_device, d, pool):
    """'same': every pooled row holds one id P = 3 times (the mean is the row, its gradient
    arrives three times as a third); 'shared': one id is in every centre's context."""
    _check(Case('pooled', d, K=3, B=6, C=1, P=3, pool=pool, seed=9), 'sorted')


# ---- g. device negatives -------------------------------------------------------------------------
@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
@pytest.mark.parametrize('d', [64, 65])
@pytest.mark.parametrize('C,K', [(3, 1), (3, 3), (3, 4), (2, 1)])
def test_device_negatives(hip_device, C, K, d, scatter):
    """noise=None: the kernels draw the negatives (Philox, two per call) — C K = 3 and 9 (odd: the
    last call half used), 12 and 2 (even), in g16 (d = 64 sorted, one draw per lane and row) and
    k_sgns (d = 65, and d = 64 atomic). The reference runs on oracle.philox.device_noise; the
    materialised sgns.device_noise equals it exactly."""
    case = Case('pairs', d, K=K, B=6, C=C, device_noise=True, seed=10)
    data, _, _ = _check(case, scatter)
    ids = sgns.device_noise(6, C, K, case.V, SEED, OFFSET, hip_device)
    assert np.array_equal(ids.cpu().numpy(), data['noise'])


def test_device_negatives_walks(hip_device):
    """The walks form's draws (g16, row_id<true>) at C K = 2 * 3 odd-per-context K."""
    _check(Case('walks', 64, K=3, n=2, L=5, R=1, device_noise=True, seed=11), 'sorted')


# ---- h. unsupported width ------------------------------------------------------------------------
@pytest.mark.parametrize('form,scatter', [('pairs', 'sorted'), ('pairs', 'atomic'),
                                          ('walks', 'sorted'), ('pooled', 'sorted')])
def test_width_513_is_refused(hip_device, form, scatter):
    """d = 513 has no instantiation (VPL <= 8): every form raises the library's
    DW_E_UNSUPPORTED message before any kernel runs, and the gradient buffers keep their bits."""
    case = Case(form, 513, K=2, B=3, C=2, n=2, L=5, R=1, P=2 if form == 'pooled' else 1, seed=12)
    data = _build(case)
    w_in, w_out = _dev(data['w_in']), _dev(data['w_out'])
    g_in, g_out = torch.full_like(w_in, 1.5), torch.full_like(w_out, -2.5)
    acc = torch.zeros(4, dtype=torch.float64, device='cuda')
    with pytest.raises(_native.DWError, match=r'\(-3\): dw_sgns: dim 513 > 512 is not supported'):
        sgns_accumulate(w_in, w_out, g_in, g_out, case.K, loss_acc=acc,
                        **_kwargs(case, data, scatter))
    torch.cuda.synchronize()
    assert bool((g_in == 1.5).all()) and bool((g_out == -2.5).all()) and not acc.any()


# ---- i. bad ids ----------------------------------------------------------------------------------
# Every guard replaces the id before an address is formed from it (read in dw_sgns.hip): k_sgns
# tests `centre_ok` (pooled: inputs_ok over all P ids) before `crow` is used and skips the centre,
# `my_ok` turns a bad row id into row 0 with `mine` false (no loss term, coefficient 0, a zero
# record); k_sgns_g16 reads `ok_c ? cid : 0`, stores -1 for a bad row id and loads row 0 with a
# zero vector for it. So: status DW_S_BAD_INDEX, the offending centre (or slot) contributes
# nothing, the mean still divides by B C, and every other term is unchanged.
def _bad_id_check(case, scatter, corrupt, exact_band=True):
    data, _ = _reference(case, exact_band)
    B, C = data['targets'].shape
    keep_s, keep_t = np.ones((B, C), bool), np.ones((B, C, case.K), bool)
    bad = {k: v.copy() for k, v in data.items()}
    corrupt(bad, keep_s, keep_t)
    ref = sgns_ref.sgns_grads_closed_form_pooled(data['w_in'], data['w_out'], data['inputs'],
                                                 data['targets'], data['noise'], keep_s, keep_t)
    _assert_bands(ref, exact_band)
    status = _status()
    g_in, g_out, acc = _launch(case, bad, scatter, status=status)
    with pytest.raises(IndexError):
        _native.check_status(status, 'sgns')
    assert int(status.item()) == _native.DW_S_BAD_INDEX
    _compare(case, ref, g_in, g_out, acc, f'bad id, {scatter}')


@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
def test_bad_centre_k_sgns_across_grid_trips(hip_device, scatter):
    """k_sgns<2, true, pairs>: centre 3 = V (its wave `continue`s and must still take centre
    3 + 8 CU * 4 on its second trip) and the last centre = -1 (a second-trip centre): the batch
    of test_second_grid_stride_trip, the smallest with a second trip."""
    case = _grid_case('k_sgns')

    def corrupt(bad, keep_s, keep_t):
        for b, v in ((3, case.V), (case.B - 1, -1)):
            bad['inputs'][b, 0] = v
            keep_s[b], keep_t[b] = False, False
    _bad_id_check(case, scatter, corrupt, exact_band=False)


@pytest.mark.parametrize('bad_id', ['V', -1])
def test_bad_centre_g16(hip_device, bad_id):
    """k_sgns_g16<1, pairs, 8>: one bad centre among the four of a wave (B = 5, centre 2)."""
    case = Case('pairs', 64, K=3, B=5, C=4, seed=13)

    def corrupt(bad, keep_s, keep_t):
        bad['inputs'][2, 0] = case.V if bad_id == 'V' else -1
        keep_s[2], keep_t[2] = False, False
    _bad_id_check(case, 'sorted', corrupt)


@pytest.mark.parametrize('bad_id', ['V', -1])
@pytest.mark.parametrize('d,scatter', [(64, 'sorted'), (100, 'sorted'), (100, 'atomic')])
def test_bad_context(hip_device, d, scatter, bad_id):
    """One bad context id (slot j = 1 of centre 1) on g16 (d = 64) and k_sgns (d = 100): only
    that positive term is dropped, the centre's other 15 rows stay."""
    case = Case('pairs', d, K=3, B=5, C=4, seed=14)

    def corrupt(bad, keep_s, keep_t):
        bad['targets'][1, 1] = case.V if bad_id == 'V' else -1
        keep_s[1, 1] = False
    _bad_id_check(case, scatter, corrupt)


@pytest.mark.parametrize('bad_id', ['V', -1])
@pytest.mark.parametrize('scatter', ['sorted', 'atomic'])
def test_bad_negative_in_second_row_group(hip_device, scatter, bad_id):
    """T = 76 (C = 4, K = 18) at d = 64 runs k_sgns<1, false> with a second row group of 12
    rows; negative k = 10 of context 3 is row t = 3 * 19 + 11 = 68 >= 64, lane 4 of that group."""
    case = Case('pairs', 64, K=18, B=5, C=4, seed=15)

    def corrupt(bad, keep_s, keep_t):
        bad['noise'][4, 3, 10] = case.V if bad_id == 'V' else -1
        keep_t[4, 3, 10] = False
    _bad_id_check(case, scatter, corrupt)


@pytest.mark.parametrize('bad_id', ['V', -1])
def test_bad_pooled_input(hip_device, bad_id):
    """Pooled (P = 3, d = 48): one bad id among a centre's inputs drops the whole centre
    (inputs_ok), its two valid input rows included."""
    case = Case('pooled', 48, K=3, B=6, C=1, P=3, seed=16)

    def corrupt(bad, keep_s, keep_t):
        bad['inputs'][4, 1] = case.V if bad_id == 'V' else -1
        keep_s[4], keep_t[4] = False, False
    _bad_id_check(case, 'sorted', corrupt)
