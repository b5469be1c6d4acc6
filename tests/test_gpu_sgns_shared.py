"""dw_sgns_walks_shared on the MI355X against the float64 restatement (tests/shared_ref.py),
against the existing per-pair kernel where the two coincide (lambda = 1), and through
Word2VecTrainer(shared_negatives=...), the config path and the karate downstream tasks.

Tables are Xavier at V = 50 with seeds chosen (and checked here, on the CPU, before each
comparison) so that no restated logit is within 1e-4 of zero or within 1 of the clamp boundary
+-ln 1e6: the two count terms then match exactly. Everything else is compared at the project's
SGNS bars, rtol 1e-5 and atol 1e-6 max|ref|."""
import functools
import random

import numpy as np
import pytest
import torch

import noise_ref
import shared_ref
from oracle import philox as ph
from oracle import sgns_ref
from shallow_encoders import _native
from shallow_encoders.word2vec.model import SkipGram
from shallow_encoders.word2vec.optim import Adam
from shallow_encoders.word2vec.sgns import sgns_accumulate, sgns_shared_accumulate
from shallow_encoders.word2vec.trainer import Word2VecTrainer
from test_gpu_sgns import assert_params_close

pytestmark = pytest.mark.gpu

V = 50
RTOL, ATOL_REL = 1e-5, 1e-6
# xavier_tables(V, d, seed) whose V x V logits all have |x| >= 1e-4 (and |x| < 1)
TABLE_SEED = {64: 5, 128: 12, 256: 3}


@functools.lru_cache(maxsize=None)
def _tables(d):
    w_in, w_out = sgns_ref.xavier_tables(V, d, TABLE_SEED[d])
    x = w_in.astype(np.float64) @ w_out.astype(np.float64).T
    assert np.abs(x).min() >= 1e-4 and np.abs(x).max() < 1.0
    return w_in, w_out


def _batch(n, L, S, seed, lo=0, hi=V):
    rng = np.random.default_rng(seed)
    return (rng.integers(lo, hi, (n, L)).astype(np.int32),
            rng.integers(lo, hi, (n, S)).astype(np.int64))


def _dev(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _run(dev, walks, ids, w_in, w_out, R, K, calls=1, scale=None):
    wi, wo = _dev(w_in, dev), _dev(w_out, dev)
    g_in, g_out = torch.zeros_like(wi), torch.zeros_like(wo)
    acc = torch.zeros(4, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    wk, sh = _dev(walks, dev), _dev(ids, dev)
    for _ in range(calls):
        sgns_shared_accumulate(wi, wo, g_in, g_out, K, walks=wk, context_radius=R, shared_ids=sh,
                               grad_scale=scale, loss_acc=acc, status=status)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), g_in.cpu().numpy(), g_out.cpu().numpy(), int(status.item())


def _check_margins(ref):
    assert ref['min_abs_logit'] >= 1e-4, ref['min_abs_logit']
    assert ref['clamp_dist'] >= 1.0, ref['clamp_dist']


def _assert_matches(got, ref, mult=1):
    acc, g_in, g_out = got[:3]
    print('acc', acc.tolist(), 'ref', (mult * ref['acc']).tolist())
    for name, g, r in (('g_in', g_in, mult * ref['g_in']), ('g_out', g_out, mult * ref['g_out'])):
        err = np.abs(g - r)
        print(name, 'max err', err.max(), 'max ref', np.abs(r).max())
        np.testing.assert_allclose(g, r, rtol=RTOL, atol=ATOL_REL * float(np.abs(r).max()),
                                   err_msg=name)
    np.testing.assert_allclose(acc[:2], mult * ref['acc'][:2], rtol=RTOL)
    # the counts, exactly: acc[3] is a sum over blocks of lambda * count in float64, so the
    # count is recovered by the division (lambda need not be a binary fraction)
    assert acc[2] == mult * ref['counts'][0]
    n3 = acc[3] / ref['lam']
    assert abs(n3 - round(n3)) < 1e-6 and round(n3) == mult * ref['counts'][1]


# ---- lambda = 1: the existing kernel fed the repeated ids ---------------------------------------
@pytest.mark.parametrize('R,K,S', [(2, 16, 64), (1, 16, 32)])
@pytest.mark.parametrize('scatter', ['atomic', 'sorted'])
def test_equals_the_per_pair_kernel_at_lambda_one(hip_device, R, K, S, scatter):
    d, n, L = 128, 5, 21
    w_in, w_out = _tables(d)
    walks, ids = _batch(n, L, S, seed=R)
    ids[0, :4] = ids[0, 4]
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, R, K)
    assert ref['lam'] == 1.0
    _check_margins(ref)
    got = _run(hip_device, walks, ids, w_in, w_out, R, K)
    assert got[3] == 0
    _assert_matches(got, ref)
    wi, wo = _dev(w_in, hip_device), _dev(w_out, hip_device)
    g_in, g_out = torch.zeros_like(wi), torch.zeros_like(wo)
    noise = _dev(shared_ref.repeated_noise(walks, ids, R, K), hip_device)
    acc = sgns_accumulate(wi, wo, g_in, g_out, K, walks=_dev(walks, hip_device), context_radius=R,
                          noise=noise, scatter=scatter)
    torch.cuda.synchronize()
    acc = acc.cpu().numpy()
    np.testing.assert_allclose(got[0][:2], acc[:2], rtol=RTOL)
    np.testing.assert_array_equal(got[0][2:], acc[2:])
    for a, b in ((got[1], g_in.cpu().numpy()), (got[2], g_out.cpu().numpy())):
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL_REL * float(np.abs(b).max()))


# ---- lambda != 1 against the restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(d, L, R, S, n):
    w_in, w_out = _tables(d)
    walks, ids = _batch(n, L, S, seed=L + S)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, R, 5)
    _check_margins(ref)
    return walks, ids, ref


@pytest.mark.parametrize('n', [1, 3, 70])
@pytest.mark.parametrize('S', [32, 96])
@pytest.mark.parametrize('L,R', [(12, 2), (41, 3), (128, 5)])   # 8, 35 (a tile edge), 118 centres
@pytest.mark.parametrize('d', [64, 128, 256])
def test_equals_restatement(hip_device, d, L, R, S, n):
    walks, ids, ref = _case(d, L, R, S, n)
    assert ref['lam'] == 2 * R * 5 / S != 1.0
    got = _run(hip_device, walks, ids, *_tables(d), R, 5)
    assert got[3] == 0
    _assert_matches(got, ref)


def test_more_walks_than_blocks(hip_device):
    """More walks than the capped grid has blocks (4 per CU): blocks take several walks, and
    reuse their LDS ids and coefficient tile."""
    n_cu = torch.cuda.get_device_properties(hip_device).multi_processor_count
    n = 4 * n_cu + 37
    w_in, w_out = _tables(64)
    walks, ids = _batch(n, 12, 32, seed=9)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, 2, 5)
    _check_margins(ref)
    _assert_matches(_run(hip_device, walks, ids, w_in, w_out, 2, 5), ref)


def test_largest_shape(hip_device):
    """L = 128 with S = 128, d = 256: the largest LDS tile (128 x 256 coefficients)."""
    w_in, w_out = _tables(256)
    walks, ids = _batch(2, 128, 128, seed=4)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, 1, 5)   # R = 1: 126 centres
    _check_margins(ref)
    _assert_matches(_run(hip_device, walks, ids, w_in, w_out, 1, 5), ref)


def test_collisions(hip_device):
    """Every walk visits the same 3 nodes and the shared ids are those nodes too, with repeats:
    3 rows of g_in and g_out take every term of every block, positive and negative."""
    w_in, w_out = _tables(128)
    rng = np.random.default_rng(2)
    nodes = np.array([7, 19, 33])
    walks = nodes[rng.integers(0, 3, (40, 20))].astype(np.int32)
    ids = nodes[rng.integers(0, 3, (40, 64))].astype(np.int64)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, 3, 5)
    _check_margins(ref)
    got = _run(hip_device, walks, ids, w_in, w_out, 3, 5)
    _assert_matches(got, ref)
    untouched = np.setdiff1d(np.arange(V), nodes)
    assert not got[1][untouched].view(np.int32).any() and not got[2][untouched].view(np.int32).any()


def test_accumulates(hip_device):
    """Two calls double g and loss_acc; rows that no term touches stay bit-zero."""
    w_in, w_out = _tables(64)
    walks, ids = _batch(6, 15, 32, seed=11, lo=0, hi=30)     # rows 30.. are never touched
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, 2, 5)
    _check_margins(ref)
    got = _run(hip_device, walks, ids, w_in, w_out, 2, 5, calls=2)
    _assert_matches(got, ref, mult=2)
    assert not got[1][30:].view(np.int32).any() and not got[2][30:].view(np.int32).any()
    centres = np.unique(walks[:, 2:-2])
    rest = np.setdiff1d(np.arange(V), centres)               # g_in: only centre rows
    assert not got[1][rest].view(np.int32).any()


def test_clamp(hip_device):
    """Out rows 40..44 (walk nodes only) give every centre a logit near -25, rows 45..49 (shared
    ids only) one near +25: their terms are cut by the clamp — loss ln 1e6 each, no gradient."""
    d, R, K, S, L, n = 64, 2, 5, 32, 14, 4
    w_in, w_out = sgns_ref.xavier_tables(V, d, seed=3)
    w_in[:, 0], w_out[:, 0] = 1.0, 0.0
    w_out[40:45, 0], w_out[45:, 0] = -25.0, 25.0
    rng = np.random.default_rng(6)
    walks = rng.integers(0, 45, (n, L)).astype(np.int32)
    walks[:, 1::3] = rng.integers(40, 45, walks[:, 1::3].shape)
    ids = rng.integers(0, 40, (n, S)).astype(np.int64)
    ids[:, ::4] = rng.integers(45, 50, ids[:, ::4].shape)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, R, K)
    _check_margins(ref)
    xp, xn = ref['pos_logits'], ref['neg_logits']
    x = np.abs(np.r_[xp, xn])
    assert not ((x > 12) & (x < 16)).any() and x[x > 16].min() > 20
    cut_pos, cut_neg = int((xp < -20).sum()), int((xn > 20).sum())
    assert cut_pos > 50 and cut_neg > 50 and cut_pos + cut_neg == (x > 16).sum()
    # the restatement's sums hold ln 1e6 for each cut term (lambda-weighted for the negatives)
    rest_pos = np.log1p(np.exp(-xp[xp > -20])).sum()
    rest_neg = np.log1p(np.exp(xn[xn < 20])).sum()
    ln1e6 = -np.log(1e-6)
    np.testing.assert_allclose(ref['acc'][0], rest_pos + cut_pos * ln1e6, rtol=1e-12)
    np.testing.assert_allclose(ref['acc'][1], ref['lam'] * (rest_neg + cut_neg * ln1e6),
                               rtol=1e-12)
    got = _run(hip_device, walks, ids, w_in, w_out, R, K)
    _assert_matches(got, ref)
    assert not got[2][40:].view(np.int32).any()              # exactly zero gradient


def test_out_of_range_ids(hip_device):
    """A walk id and a shared id outside [0, V) set DW_S_BAD_INDEX; the rest of the batch is
    the restatement's result without their terms."""
    w_in, w_out = _tables(64)
    walks, ids = _batch(5, 16, 32, seed=13)
    walks[1, 7] = V + 4          # a centre and a context of walk 1
    walks[3, 0] = -1             # a context only
    ids[2, 5] = V
    ids[4, 31] = -7
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, 2, 5)
    assert ref['bad']
    _check_margins(ref)
    got = _run(hip_device, walks, ids, w_in, w_out, 2, 5)
    assert got[3] == _native.DW_S_BAD_INDEX
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    _assert_matches(got, ref)
    with pytest.raises(IndexError):
        _native.check_status(torch.tensor([got[3]], dtype=torch.int32), 'shared step')


def test_wrapper_refuses_bad_shapes(hip_device):
    w_in, w_out = _tables(64)
    walks, ids = _batch(2, 12, 48, seed=1)
    with pytest.raises(_native.DWError, match='multiple of 32'):
        _run(hip_device, walks, ids, w_in, w_out, 2, 5)
    with pytest.raises(ValueError, match='n_walks \\* S'):
        _run(hip_device, walks, ids.reshape(-1)[:-1], w_in, w_out, 2, 5)


# ---- the trainer ------------------------------------------------------------------------------
# lr: torch.optim.Adam's default. assert_params_close's atol is 1e-6 absolute on a parameter, and
# an Adam step moves an entry whose gradient carries relative error rho by about lr * rho, so the
# float32 summation noise the gradient bars allow on near-cancelling entries (rho up to ~1e-3
# where |g| is 1e-3 of the largest entry) stays inside it at lr = 1e-3; an error in the plumbing
# (ids, offsets, a missing or misdirected term) still moves entries by ~lr, 1000 atol.
T_D, T_R, T_K, T_L, T_S, T_SEED, T_LR = 64, 2, 5, 12, 32, 5, 1e-3
DEG = np.r_[0.0, np.random.default_rng(1).integers(1, 18, V - 1)].astype(np.float64)
DEG[7] = DEG[20] = 0.0


def _trainer(noise, dev, shared, **kw):
    torch.manual_seed(3)
    model = SkipGram(V, T_D).to(dev)
    opt = Adam(model.parameters(), lr=T_LR)
    tr = Word2VecTrainer(model, opt, None, neg_samples=T_K, vocab_size=V, noise=noise,
                         seed=T_SEED, context_radius=T_R, shared_negatives=shared, **kw)
    tr.manual_grads = True
    return tr, model, opt


@pytest.mark.parametrize('noise', ['device', 'unigram'])
def test_trainer_steps_equal_manual_loop(hip_device, noise):
    """Three steps of Word2VecTrainer(shared_negatives=32) == ids from the restated streams at
    the running centre counter -> restatement gradients -> torch.optim.Adam."""
    rng = np.random.default_rng(0)
    batches = [rng.integers(1, V, (n, T_L)).astype(np.int32) for n in (20, 13, 20)]
    kw = dict(noise_weights=torch.as_tensor(DEG)) if noise == 'unigram' else {}
    tr, model, opt = _trainer(noise, hip_device, T_S, **kw)
    w0 = [p.detach().cpu().numpy().copy() for p in (model.input_weight, model.output_weight)]
    ref = sgns_ref.TorchAdamRef(w0[0], w0[1], lr=T_LR)
    host = noise_ref.alias_table(DEG ** 0.75) if noise == 'unigram' else None
    off = 0
    for wk in batches:
        loss = tr.training_step(_dev(wk, hip_device))
        opt.step()
        opt.zero_grad()
        n = wk.shape[0]
        if noise == 'unigram':
            ids = noise_ref.alias_noise(host, T_SEED, off, n, 1, T_S)
            assert not np.isin(ids, [0, 7, 20]).any()        # no zero-weight id
        else:
            ids = ph.device_noise(T_SEED, off, n, 1, T_S, V)
        key = ('shared', n, T_S)
        np.testing.assert_array_equal(tr._noise_bufs[key].cpu().numpy(), ids)
        r = shared_ref.shared_ref(wk, ids.reshape(n, T_S), *ref.tables(), T_R, T_K)
        M = n * (T_L - 2 * T_R) * 2 * T_R
        np.testing.assert_allclose(float(loss['loss']), (r['acc'][0] + r['acc'][1]) / M,
                                   rtol=1e-5)
        ref.step(r['g_in'].astype(np.float32), r['g_out'].astype(np.float32))
        off += n * (T_L - 2 * T_R)
        assert tr._noise_offset == off
    torch.cuda.synchronize()
    exp = ref.tables()
    for p, e in zip((model.input_weight, model.output_weight), exp):
        assert_params_close(p.detach().cpu().numpy(), e, T_LR)
    assert len([k for k in tr._noise_bufs if k[0] == 'shared']) == 2   # one buffer per shape


def test_trainer_first_step_errors(hip_device, monkeypatch):
    tr, model, opt = _trainer('device', hip_device, T_S)
    wk = _dev(np.ones((4, T_L), np.int32), hip_device)
    with pytest.raises(ValueError, match='pairs'):
        tr.training_step((torch.ones(8, 1, dtype=torch.long), torch.ones(8, 4, dtype=torch.long)))
    with pytest.raises(ValueError, match='walk_length'):
        tr.training_step(_dev(np.ones((4, 129), np.int32), hip_device))
    tr48, _, _ = _trainer('device', hip_device, 48)
    with pytest.raises(ValueError, match='multiple of 32'):
        tr48.training_step(wk)
    torch.manual_seed(0)
    tr96 = Word2VecTrainer(SkipGram(V, 96).to(hip_device), None, None, neg_samples=T_K,
                           vocab_size=V, noise='device', context_radius=T_R, shared_negatives=32)
    tr96.manual_grads = True
    with pytest.raises(ValueError, match='dim'):
        tr96.training_step(wk)
    monkeypatch.setenv('DW_DETERMINISTIC', '1')
    with pytest.raises(ValueError, match='deterministic'):
        tr.training_step(wk)
    monkeypatch.delenv('DW_DETERMINISTIC')
    assert tr._noise_offset == 0                             # a refused step draws nothing
    assert np.isfinite(float(tr.training_step(wk)['loss']))


def test_graph_replay_is_not_eligible(hip_device):
    from shallow_encoders.graph.datasets import KarateClubDataset
    from shallow_encoders.word2vec.graphed import GraphedTrainerStep
    random.seed(0)
    ds = KarateClubDataset(walks_per_node=2, walk_length=T_L, method='deepwalk', rng='philox',
                           seed=1, device=hip_device)
    n = len(ds.csr.row_ptr) - 1                              # vocabulary rows (0 is <unk>)

    def make(shared):
        model = SkipGram(n, 64).to(hip_device)
        tr = Word2VecTrainer(model, Adam(model.parameters(), lr=0.05), None, neg_samples=T_K,
                             vocab_size=n, noise='device', context_radius=T_R,
                             shared_negatives=shared)
        tr.manual_grads = True
        return tr
    assert GraphedTrainerStep.eligible(make(0), ds)
    assert not GraphedTrainerStep.eligible(make(32), ds)


# ---- quality ------------------------------------------------------------------------------------
# The baseline's own spread over seeds 0-4 for this protocol (max - min of the downstream tool's
# mean accuracies; measured once on MI355X): node accuracy .9882 .9912 .9897
# .9838 .9912, edge accuracy .7775 .7459 .7627 .7596 .7135.
NODE_MARGIN = 0.0074
EDGE_MARGIN = 0.0640


def _karate(tmp_path, tag, shared, seed=0):
    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    out = str(tmp_path / tag)
    over = [f'path.output_dir={out}', f'output_dir={out}', 'model.embedding_size=64',
            'datamodule.additional_parameters.rng=philox',
            f'datamodule.additional_parameters.seed={seed}', 'train.noise=device',
            f'train.seed={seed}', f'train.shared_negatives={shared}']
    random.seed(seed)
    train_tool.main(['--config-name', 'sge_sg_karate_club'] + over)
    return downstream.main(['--config-name', 'sge_sg_karate_club'] + over + [
        'downstream.node_classification.n_experiments=20',
        'downstream.node_classification.visualize=false',
        'downstream.edge_classification.n_experiments=100'])


def test_quality_karate(tmp_path, hip_device):
    """sge_sg_karate_club at d = 64 (Philox walks, device noise), trained with per-pair negatives
    and with 32 shared negatives per walk, then the downstream tool on each: the shared run's node
    and edge accuracies are not below the baseline's by more than the baseline's own spread
    over seeds 0-4 (NODE_MARGIN = 0.0074, EDGE_MARGIN = 0.0640). Measured with seed 0: baseline
    node .9882 / edge .7775, shared .9882 / .7462 (shared over seeds 0-4: node .9882-.9956, edge
    .7240-.7785)."""
    base = _karate(tmp_path, 'base', 0)
    shared = _karate(tmp_path, 'shared', 32)
    print('baseline', base, 'shared', shared)
    assert shared['node_accuracy'] >= base['node_accuracy'] - NODE_MARGIN, (base, shared)
    assert shared['edge_accuracy'] >= base['edge_accuracy'] - EDGE_MARGIN, (base, shared)
