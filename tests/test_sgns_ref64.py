"""oracle.sgns_ref.sgns_grads_closed_form_pooled (the float64 closed form the GPU lattice tests
compare against) checked on the CPU against float64 torch.autograd of the reference chain
``ns_loss(pooled_logits(...))`` (model.py:102-107 + loss.py:14-22), and against the existing
P = 1 closed form bit for bit.

The autograd bar is float64 reassociation only: rtol 1e-11, atol 1e-15 (the gradients are
~1e-2 / M; 1e-15 is below one float64 ulp of a term)."""
import numpy as np
import pytest
import torch

from oracle import sgns_ref


def _case(P, seed, V=41, d=7, B=9, C=3, K=4, repeat=False, clamp=False):
    """Tables and ids of one case. ``clamp``: rows 0..5 of both tables are +-5 u plus noise (u a
    unit vector), so logits between them are about +-25: both clamp branches and the saturated
    end; ``repeat``: every pooled row holds some id twice (P >= 2) and ids repeat across rows."""
    rng = np.random.default_rng(seed)
    w_in = rng.uniform(-0.4, 0.4, (V, d))
    w_out = rng.uniform(-0.4, 0.4, (V, d))
    hi = V
    if clamp:
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        for r in range(6):
            w_in[r] = (5.0 if r % 2 else -5.0) * u + 0.01 * rng.standard_normal(d)
            w_out[r] = (5.0 if r % 3 else -5.0) * u + 0.01 * rng.standard_normal(d)
        hi = 9    # ids mostly among the large rows
    inputs = rng.integers(0, hi, (B, P))
    if repeat and P >= 2:
        inputs[:, -1] = inputs[:, 0]
        inputs[1] = inputs[0]
    if clamp:     # some contexts of large rows only, so whole-context logits reach +-25
        inputs[::2] = inputs[::2, :1]
    targets = rng.integers(0, hi, (B, C))
    noise = rng.integers(0, hi, (B, C, K))
    return w_in, w_out, inputs, targets, noise


def _autograd(w_in, w_out, inputs, targets, noise):
    win = torch.tensor(w_in, dtype=torch.float64, requires_grad=True)
    wout = torch.tensor(w_out, dtype=torch.float64, requires_grad=True)
    inp, tgt, nz = (torch.as_tensor(x, dtype=torch.long) for x in (inputs, targets, noise))
    B, C = tgt.shape
    pos = sgns_ref.pooled_logits(win, wout, inp, tgt)
    neg = sgns_ref.pooled_logits(win, wout, inp, nz.reshape(B, -1)).view(B, C, -1)
    loss = sgns_ref.ns_loss(pos, neg)
    loss['loss'].backward()
    return ({k: float(v.detach()) for k, v in loss.items()}, win.grad.numpy(), wout.grad.numpy(),
            pos.detach().numpy(), neg.detach().numpy())


@pytest.mark.parametrize('clamp', [False, True])
@pytest.mark.parametrize('repeat', [False, True])
@pytest.mark.parametrize('P', [1, 2, 3, 10])
def test_pooled_closed_form_equals_float64_autograd(P, repeat, clamp):
    case = _case(P, seed=100 * P + 10 * repeat + clamp, repeat=repeat, clamp=clamp)
    r = sgns_ref.sgns_grads_closed_form_pooled(*case)
    loss, gi, go, pos, neg = _autograd(*case)
    if clamp:    # both clamp branches, and unclamped terms on both sides of zero
        assert r['clamped_s'].any() and r['clamped_t'].any()
        assert (~r['clamped_s']).any() and (~r['clamped_t']).any()
        assert r['s'].max() > 20 and r['t'].min() < -20
        assert r['clamp_margin'] > 1e-3
    else:
        assert not r['clamped_s'].any() and not r['clamped_t'].any()
    np.testing.assert_allclose(r['s'], pos, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r['t'], neg, rtol=1e-12, atol=1e-15)
    for k in ('loss', 'positive-loss', 'negative-loss'):
        assert r[k] == pytest.approx(loss[k], rel=1e-12)
    np.testing.assert_allclose(r['g_in'], gi, rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(r['g_out'], go, rtol=1e-11, atol=1e-15)
    # a clamped term has loss ln 10^6 and no gradient: the rows only such terms touch stay zero
    M = case[3].size
    n_cl = int(r['clamped_s'].sum()) + int(r['clamped_t'].sum())
    unclamped = -np.log(np.maximum(1 / (1 + np.exp(-r['s'])), 1e-6))[~r['clamped_s']].sum() \
        - np.log(np.maximum(1 / (1 + np.exp(r['t'])), 1e-6))[~r['clamped_t']].sum()
    assert r['loss'] * M == pytest.approx(unclamped + n_cl * np.log(1e6), rel=1e-12)
    # the absolute sums bound the gradients elementwise and vanish with them
    assert (np.abs(r['g_in']) <= r['A_in'] * (1 + 1e-12)).all()
    assert (np.abs(r['g_out']) <= r['A_out'] * (1 + 1e-12)).all()
    # the metric counts: the reference thresholds sigmoid(x) >= .5, that is x >= 0
    assert r['recall_count'] == int((pos >= 0).sum())
    assert r['neg_hit_count'] == int((neg >= 0).sum())
    assert r['recall'] == r['recall_count'] / M
    assert r['precision'] == 1.0 - r['neg_hit_count'] / (M * neg.shape[2])


@pytest.mark.parametrize('clamp', [False, True])
def test_pooled_form_with_one_input_is_the_skipgram_form_bit_for_bit(clamp):
    w_in, w_out, inputs, targets, noise = _case(1, seed=5 + clamp, clamp=clamp)
    loss, gi, go = sgns_ref.sgns_grads_closed_form(w_in, w_out, inputs, targets, noise)
    for ins in (inputs, inputs.reshape(-1)):
        r = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, ins, targets, noise)
        assert r['loss'] == loss
        assert np.array_equal(r['g_in'], gi) and np.array_equal(r['g_out'], go)


def test_a_row_listed_twice_in_one_context_receives_the_gradient_twice():
    w_in, w_out, inputs, targets, noise = _case(3, seed=9)
    inputs[:] = np.array([[4, 4, 11]])           # every context: row 4 twice, row 11 once
    r = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs, targets, noise)
    np.testing.assert_allclose(r['g_in'][4], 2 * r['g_in'][11], rtol=1e-13)
    assert np.abs(r['g_in'][11]).max() > 0
    touched = np.zeros(len(w_in), bool)
    touched[[4, 11]] = True
    assert not r['g_in'][~touched].any()


def test_kept_masks_drop_terms_and_keep_the_mean():
    """A dropped centre / slot contributes nothing; M stays B C (the bad-index contract)."""
    w_in, w_out, inputs, targets, noise = _case(2, seed=3)
    B, C = targets.shape
    K = noise.shape[2]
    full = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs, targets, noise)
    # dropping centre 2 == the batch without it, rescaled by (B - 1) / B
    ks, kt = np.ones((B, C), bool), np.ones((B, C, K), bool)
    ks[2], kt[2] = False, False
    r = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs, targets, noise, ks, kt)
    rest = np.arange(B) != 2
    sub = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs[rest], targets[rest],
                                                 noise[rest])
    f = (B - 1) / B
    np.testing.assert_allclose(r['g_in'], f * sub['g_in'], rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(r['g_out'], f * sub['g_out'], rtol=1e-12, atol=1e-18)
    assert r['loss'] == pytest.approx(f * sub['loss'], rel=1e-12)
    assert r['recall_count'] == sub['recall_count']
    # dropping one negative slot removes exactly its term
    kt = np.ones((B, C, K), bool)
    kt[1, 2, 3] = False
    r = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs, targets, noise, None, kt)
    dt = 1 / (1 + np.exp(-full['t'][1, 2, 3])) / (B * C)
    h = w_in[inputs[1]].mean(0)
    exp_out = full['g_out'].copy()
    exp_out[noise[1, 2, 3]] -= dt * h
    exp_in = full['g_in'].copy()
    for p in inputs[1]:
        exp_in[p] -= dt * w_out[noise[1, 2, 3]] / 2
    np.testing.assert_allclose(r['g_out'], exp_out, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(r['g_in'], exp_in, rtol=1e-12, atol=1e-18)


def test_no_negatives():
    """K = 0 (the ABI allows it): no negative terms, precision 1 as sgns.loss_terms forms it."""
    w_in, w_out, inputs, targets, _ = _case(2, seed=4)
    B, C = targets.shape
    r = sgns_ref.sgns_grads_closed_form_pooled(w_in, w_out, inputs, targets,
                                               np.zeros((B, C, 0), np.int64))
    assert r['negative-loss'] == 0.0 and r['precision'] == 1.0 and r['t'].shape == (B, C, 0)
    assert r['loss'] == r['positive-loss'] > 0
