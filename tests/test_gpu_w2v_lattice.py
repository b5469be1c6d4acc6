"""The autograd-path kernels of the reference API at their own lattice: SkipGram.forward /
CBOW.forward (k_logits, one wave per row, a `for e = lane; e < d; e += 64` element loop) with
their backward (k_logits_bwd) against float64 autograd of oracle.sgns_ref.pooled_logits, and
sgns.renorm_ (k_renorm_keys + sort + k_renorm_rows) against torch.embedding_renorm_ on the CPU
and a float64 restatement.

Bars: those of test_cbow_forward_backward_vs_oracle (logits rtol 1e-5 / atol 1e-7, gradients
rtol 1e-4 / atol 1e-7) and of the max_norm fixture test (rtol 1e-6 / atol 1e-7)."""
import numpy as np
import pytest
import torch

from oracle import sgns_ref

from shallow_encoders import _native
from shallow_encoders.word2vec.model import CBOW, SkipGram
from shallow_encoders.word2vec.sgns import renorm_

pytestmark = pytest.mark.gpu

V = 61


@pytest.mark.parametrize('B', [1, 9])
@pytest.mark.parametrize('N', [1, 7])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('d', [1, 63, 64, 65, 300])
def test_logits_forward_backward_vs_float64(hip_device, d, P, N, B):
    """k_logits / k_logits_bwd: d = 1 (one live lane), 63 / 64 / 65 (the element loop's last
    trip partial, exact, one element into a second trip), 300 (five trips); P = 1 through
    SkipGram, P = 3 through CBOW with one id twice in a context; N = 1 and 7 output rows; B = 1
    and 9 (a third block of four waves with one row). Ids repeat across rows (12 distinct) and
    include rows 0 and V - 1."""
    rng = np.random.default_rng([d, P, N, B])
    w_in0, w_out0 = sgns_ref.xavier_tables(V, d, seed=d)
    pool = np.concatenate([[0, V - 1], rng.permutation(np.arange(1, V - 1))[:10]])
    inputs = pool[rng.integers(0, len(pool), (B, P))]
    if P > 1:
        inputs[:, -1] = inputs[:, 0]
    outputs = pool[rng.integers(0, len(pool), (B, N))]
    model = (SkipGram if P == 1 else CBOW)(V, d).to(hip_device)
    with torch.no_grad():
        model.input_weight.copy_(torch.as_tensor(w_in0))
        model.output_weight.copy_(torch.as_tensor(w_out0))
    ins, outs = torch.as_tensor(inputs), torch.as_tensor(outputs)
    wt = torch.as_tensor(rng.uniform(-1, 1, (B, N)))
    logits = model(ins, outs, proba=False)
    (logits * wt.float().to(hip_device)).sum().backward()
    win = torch.tensor(w_in0, dtype=torch.float64, requires_grad=True)
    wout = torch.tensor(w_out0, dtype=torch.float64, requires_grad=True)
    ref = sgns_ref.pooled_logits(win, wout, ins, outs)
    (ref * wt.float().double()).sum().backward()
    got = logits.detach().cpu().numpy()
    print('max |logit err|', np.abs(got - ref.detach().numpy()).max(), 'max |g_in err|',
          np.abs(model.input_weight.grad.cpu().numpy() - win.grad.numpy()).max(), 'max |g_out err|',
          np.abs(model.output_weight.grad.cpu().numpy() - wout.grad.numpy()).max())
    np.testing.assert_allclose(got, ref.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(model.input_weight.grad.cpu().numpy(), win.grad.numpy(),
                               rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(model.output_weight.grad.cpu().numpy(), wout.grad.numpy(),
                               rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(model(ins, outs, proba=True).detach().cpu().numpy(),
                               torch.sigmoid(ref).detach().numpy(), rtol=1e-5, atol=1e-7)


MAX_NORM = 1.0


def _renorm_table(d, seed):
    """(V, d) float32 rows of norm 0.3, 0.9 (well below max_norm 1), 1.5 and 4 (well above) in
    turn, random directions — none within 1e-5 max_norm of max_norm (the band where the float
    summation order may decide; asserted by the caller in float64)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((V, d))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    w *= np.array([0.3, 0.9, 1.5, 4.0])[np.arange(V) % 4][:, None]
    return w.astype(np.float32)


@pytest.mark.parametrize('bad', [False, True])
@pytest.mark.parametrize('n_ids,two_d', [(1, False), (5, False), (6, True), (1000, False),
                                         (1000, True)])
@pytest.mark.parametrize('d', [1, 2, 63, 64, 65, 300])
def test_renorm_vs_torch_and_float64(hip_device, d, n_ids, two_d, bad):
    """renorm_ at d = 1, 2, 63, 64, 65, 300 (k_renorm_rows' element loop), ids 1-D and 2-D
    (n x 2, so 6 ids where the 1-D list has 5), 1, 5 and 1000 of them. 1000 ids over at most
    V = 61 rows: every listed row is listed many times and must be scaled ONCE, to norm
    max_norm n / (n + 1e-7) with n its norm before. Rows well below max_norm and rows not listed
    keep their bits; with ``bad`` the list also holds one id V, which is reported (IndexError)
    while every other id is treated as before."""
    rng = np.random.default_rng([d, n_ids, two_d])
    w0 = _renorm_table(d, seed=d)
    norm64 = np.linalg.norm(w0.astype(np.float64), axis=1)
    assert (np.abs(norm64 - MAX_NORM) >= 1e-5 * MAX_NORM).all()
    ids = rng.integers(0, V - 8, n_ids)              # the last 8 rows are never listed
    if n_ids >= 5:
        ids[:5] = [0, 2, 2, 3, 2]                    # rows below and above, one above repeated
    valid = ids.copy()
    if bad:
        if n_ids == 1:
            valid = ids[:0]
            ids = np.array([V])
        else:
            ids[1] = V
            valid = np.delete(ids, 1)
    shape = (-1, 2) if two_d else (-1,)
    w = torch.as_tensor(w0).to(hip_device)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    renorm_(w, torch.as_tensor(ids.reshape(shape)).to(hip_device), MAX_NORM, status=status)
    if bad:
        with pytest.raises(IndexError):
            _native.check_status(status, 'embedding renorm')
        with pytest.raises(IndexError):           # the default: renorm_ checks its own status
            renorm_(torch.as_tensor(w0).to(hip_device),
                    torch.as_tensor(ids.reshape(shape)).to(hip_device), MAX_NORM)
    else:
        assert int(status.item()) == 0
    got = w.cpu().numpy()
    exp = torch.as_tensor(w0.copy())
    if valid.size:
        torch.embedding_renorm_(exp, torch.as_tensor(valid), MAX_NORM, 2.0)
    np.testing.assert_allclose(got, exp.numpy(), rtol=1e-6, atol=1e-7)
    listed = np.zeros(V, bool)
    listed[valid] = True
    scaled = listed & (norm64 > MAX_NORM)
    exp64 = w0.astype(np.float64)
    exp64[scaled] *= (MAX_NORM / (norm64[scaled] + 1e-7))[:, None]
    np.testing.assert_allclose(got, exp64, rtol=1e-6, atol=1e-7)
    assert np.array_equal(got[~scaled].view(np.int32), w0[~scaled].view(np.int32))
    if scaled.any():
        after = np.linalg.norm(got[scaled].astype(np.float64), axis=1)
        np.testing.assert_allclose(after, MAX_NORM * norm64[scaled] / (norm64[scaled] + 1e-7),
                                   rtol=1e-6)
    if n_ids >= 5:
        assert scaled[2] and scaled[3] and not scaled[0]
