"""The SGD kernels (csrc/dw_sgd.hip) against tests/sgd_ref.py bit for bit, and the trainer's SGD
touched-rows step against the same run under the real torch.optim.SGD on the device."""
import numpy as np
import pytest
import torch

import sgd_ref
from shallow_encoders import _native
from shallow_encoders.word2vec import optim
from shallow_encoders.word2vec.model import SkipGram
from shallow_encoders.word2vec.trainer import Word2VecTrainer
from sgd_ref import mixed_grads

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32)


def dense_call(p, g, buf, lr, first, zero, momentum=0.0, dampening=0.0, weight_decay=0.0,
               nesterov=False):
    _native.call('dw_sgd_dense', _native.ptr(p), _native.ptr(g), _native.ptr(buf), p.numel(),
                 -float(lr), float(weight_decay), float(momentum), 1.0 - float(dampening),
                 int(nesterov), int(first), int(zero), _native.stream(p.device))


def rows_call(p, g, ids, claim, lr, status):
    V, d = p.shape
    _native.call('dw_sgd_rows', _native.ptr(p), _native.ptr(g), V, d, _native.ptr(ids),
                 ids.element_size(), ids.numel(), _native.ptr(claim), -float(lr),
                 _native.ptr(status), _native.stream(p.device))


# ---- dw_sgd_dense -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(sgd_ref.OPTION_SETS))
def test_dense_equals_restatement_bit_for_bit(hip_device, name):
    """3 steps (first_step, then the momentum chain; lr changed before the third) at sizes that
    are all tail (1, 3), whole vectors (257 * 100) and several blocks plus a tail (2^16 + 5),
    with and without zero_grad: p and the momentum buffer equal sgd_ref on every entry."""
    opts = sgd_ref.OPTION_SETS[name]
    mom = bool(opts.get('momentum'))
    for n in (1, 3, 257 * 100, 2 ** 16 + 5):
        for zero in (1, 0):
            rng = np.random.default_rng(n + zero)
            p_ref, buf_ref = (rng.standard_normal(n) * 0.1).astype(np.float32), None
            p = torch.from_numpy(p_ref.copy()).to(hip_device)
            buf = torch.full((n,), float('nan'), device=hip_device) if mom else None
            for step in range(3):
                lr = 0.05 if step < 2 else 0.0125
                g_host = mixed_grads(rng, n)
                g = torch.from_numpy(g_host.copy()).to(hip_device)
                dense_call(p, g, buf, lr, step == 0, zero, **opts)
                p_ref, buf_ref = sgd_ref.sgd_step(p_ref, g_host, buf_ref, lr, **opts)
                np.testing.assert_array_equal(bits(p), bits(p_ref), err_msg=f'{n} {zero} {step}')
                if mom:
                    np.testing.assert_array_equal(bits(buf), bits(buf_ref))
                if zero:
                    assert not bits(g).any()          # +0 everywhere
                else:
                    np.testing.assert_array_equal(bits(g), bits(g_host))


def test_dense_takes_unaligned_buffers_and_empty_ones(hip_device):
    """A view 4 bytes into an allocation (no 16-B accesses possible) and n_elem = 0."""
    rng = np.random.default_rng(0)
    n = 1027
    p_host = rng.standard_normal(n + 1).astype(np.float32)
    g_host = mixed_grads(rng, n + 1)
    p = torch.from_numpy(p_host.copy()).to(hip_device)
    g = torch.from_numpy(g_host.copy()).to(hip_device)
    dense_call(p[1:], g[1:], None, 0.1, True, 1)
    exp, _ = sgd_ref.sgd_step(p_host[1:], g_host[1:], None, 0.1)
    np.testing.assert_array_equal(bits(p[1:]), bits(exp))
    assert bits(p[:1]) == bits(p_host[:1]) and bits(g[:1]) == bits(g_host[:1])
    assert not bits(g[1:]).any()
    dense_call(p[:0], g[:0], None, 0.1, True, 1)       # nothing to do, nothing launched
    torch.cuda.synchronize()


# ---- dw_sgd_rows --------------------------------------------------------------------------------
V_ROWS = 257      # the last claim word is partial (257 = 8 * 32 + 1)


def id_lists():
    rng = np.random.default_rng(11)
    few = rng.choice(V_ROWS, 40, replace=False)
    return {
        'empty': np.zeros(0, np.int64),
        'one': np.array([131]),
        'all_equal': np.full(777, 200),
        'ends': np.array([0, 256]),
        # duplicates race for their claims across lanes, waves and blocks
        'dups': few[rng.integers(0, 40, 10_000)],
        'every_row': rng.permutation(V_ROWS),
    }


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('d', [2, 3, 100, 128, 260])
def test_rows_equal_restatement_bit_for_bit(hip_device, d, dtype):
    """d = 128 and 100: 16-B accesses (100: 25 live lanes); 260: two trips over the row; 2: 8-B;
    3: 4-B (no wider access keeps every row aligned)."""
    lr = 0.3
    rng = np.random.default_rng(d)
    p_host = rng.standard_normal((V_ROWS, d)).astype(np.float32)
    g_host = mixed_grads(rng, (V_ROWS, d))
    g_host[7] = 0                                       # a row without a gradient
    g_host[9, 0] = -0.0
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    claim = torch.zeros((V_ROWS + 31) // 32, dtype=torch.int32, device=hip_device)
    dense_p = torch.from_numpy(p_host.copy()).to(hip_device)
    dense_call(dense_p, torch.from_numpy(g_host.copy()).to(hip_device), None, lr, True, 1)
    dense_p = dense_p.cpu().numpy()
    for name, ids_host in id_lists().items():
        ids = torch.from_numpy(np.asarray(ids_host, dtype=np.int64)).to(hip_device, dtype)
        runs = []
        for _ in range(2):                              # a second run from the same inputs
            p = torch.from_numpy(p_host.copy()).to(hip_device)
            g = torch.from_numpy(g_host.copy()).to(hip_device)
            rows_call(p, g, ids, claim, lr, status)
            runs.append((p.cpu().numpy(), g.cpu().numpy()))
            assert not claim.cpu().numpy().any(), name  # left zero
        (p1, g1), (p2, g2) = runs
        exp_p, exp_g = sgd_ref.sgd_rows(p_host, g_host, ids_host, lr)
        np.testing.assert_array_equal(bits(p1), bits(exp_p), err_msg=name)
        np.testing.assert_array_equal(bits(p1), bits(p2), err_msg=name)
        np.testing.assert_array_equal(bits(g1), bits(g2), err_msg=name)
        listed = np.unique(ids_host).astype(np.int64)
        rest = np.setdiff1d(np.arange(V_ROWS), listed)
        np.testing.assert_array_equal(bits(p1[listed]), bits(dense_p[listed]), err_msg=name)
        np.testing.assert_array_equal(bits(p1[rest]), bits(p_host[rest]), err_msg=name)
        np.testing.assert_array_equal(bits(g1[rest]), bits(g_host[rest]), err_msg=name)
        assert not bits(g1[listed]).any(), name         # +0 everywhere
        np.testing.assert_array_equal(bits(g1), bits(exp_g), err_msg=name)
    assert int(status.item()) == 0


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_rows_skip_and_report_an_id_out_of_range(hip_device, dtype):
    d, lr = 100, 0.3
    rng = np.random.default_rng(1)
    p_host = rng.standard_normal((V_ROWS, d)).astype(np.float32)
    g_host = mixed_grads(rng, (V_ROWS, d)) + np.float32(1e-3)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    claim = torch.zeros((V_ROWS + 31) // 32, dtype=torch.int32, device=hip_device)
    ids_host = np.array([3, V_ROWS, -1, 2 ** 31 - 1, 3])
    p = torch.from_numpy(p_host.copy()).to(hip_device)
    g = torch.from_numpy(g_host.copy()).to(hip_device)
    rows_call(p, g, torch.from_numpy(ids_host).to(hip_device, dtype), claim, lr, status)
    assert int(status.item()) == _native.DW_S_BAD_INDEX
    with pytest.raises(IndexError):
        _native.check_status(status, 'test')
    exp_p, exp_g = sgd_ref.sgd_rows(p_host, g_host, [3], lr)
    np.testing.assert_array_equal(bits(p), bits(exp_p))  # row 3 moved, nothing else
    np.testing.assert_array_equal(bits(g), bits(exp_g))
    assert not claim.cpu().numpy().any()


def test_rows_step_replays_in_a_graph(hip_device):
    """One dw_sgd_rows call captured with a fixed id list, replayed twice (the gradient buffer
    refilled between the replays), against two eager calls: the same bits."""
    d, lr = 128, 0.2
    rng = np.random.default_rng(2)
    p_host = rng.standard_normal((V_ROWS, d)).astype(np.float32)
    grads = [torch.from_numpy(mixed_grads(rng, (V_ROWS, d))).to(hip_device) for _ in range(2)]
    ids = torch.from_numpy(id_lists()['dups']).to(hip_device, torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    claim = torch.zeros((V_ROWS + 31) // 32, dtype=torch.int32, device=hip_device)
    eager = torch.from_numpy(p_host.copy()).to(hip_device)
    for k in range(2):
        rows_call(eager, grads[k].clone(), ids, claim, lr, status)
    p = torch.from_numpy(p_host.copy()).to(hip_device)
    g = torch.zeros_like(p)
    s = torch.cuda.Stream(hip_device)
    s.wait_stream(torch.cuda.current_stream(hip_device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rows_call(p, g, ids, claim, lr, status)
    torch.cuda.synchronize(hip_device)
    assert torch.equal(p.cpu(), torch.from_numpy(p_host))   # capturing ran nothing
    for k in range(2):
        g.copy_(grads[k])
        graph.replay()
        torch.cuda.synchronize(hip_device)
    np.testing.assert_array_equal(bits(p), bits(eager))
    assert not claim.cpu().numpy().any() and int(status.item()) == 0


# ---- the trainer --------------------------------------------------------------------------------
SEED = 5


@pytest.fixture(scope='module')
def rmat12(hip_device):
    from shallow_encoders.graph.rmat import rmat_graph
    return rmat_graph(12, 40_000, 0, device=hip_device)


def run_trainer(csr, dev, make_opt, d, n_walks, L, R, K, lr=0.5):
    """5 steps with an lr change before the fourth; returns (model, opt, losses, walk batches)."""
    from shallow_encoders.graph.random_walk_generator import DeepWalk
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    V = csr.vocab_size
    torch.manual_seed(11)
    model = SkipGram(V, d).cuda()
    init = [p.detach().clone() for p in (model.input_weight, model.output_weight)]
    opt = make_opt(model.parameters(), lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    tr = Word2VecTrainer(model, opt, sched, neg_samples=K, vocab_size=V, noise='device',
                         seed=SEED, context_radius=R)
    tr.manual_grads = True
    losses, batches = [], []
    for step in range(5):
        if step == 3:
            sched.step()
        starts = torch.randint(1, V, (n_walks,), generator=torch.Generator().manual_seed(step),
                               dtype=torch.int32).to(dev)
        walks = walker.walk_batch(starts, walk_id0=step * n_walks)
        batches.append(walks)
        out = tr.training_step(walks)
        opt.step()
        opt.zero_grad()
        losses.append(out['loss'])
    torch.cuda.synchronize()
    tr.on_train_epoch_end()                              # (checks the rows steps' status word)
    return model, opt, [float(x) for x in losses], batches, init


def assert_same_training(ours, theirs):
    (mo, _, lo, _, _), (mt, _, lt, _, _) = ours, theirs
    np.testing.assert_allclose(lo, lt, rtol=1e-4)
    for a, b in ((mo.input_weight, mt.input_weight), (mo.output_weight, mt.output_weight)):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(),
                                   rtol=1e-5, atol=1e-6)   # every entry


def torch_sgd(**kw):
    return lambda params, lr: torch.optim.SGD(params, lr=lr, **kw)


def hip_sgd(**kw):
    return lambda params, lr: optim.SGD(params, lr=lr, **kw)


@pytest.mark.parametrize('d', [8, 128])
def test_trainer_small_batch_goes_by_rows(hip_device, rmat12, d):
    """4 walks, L = 12, R = 2, K = 2: 32 centres and 48 + 256 = 304 out ids, below V = 4,097."""
    from shallow_encoders.word2vec.sgns import device_noise
    shape = dict(n_walks=4, L=12, R=2, K=2)
    ours = run_trainer(rmat12, hip_device, hip_sgd(), d, **shape)
    theirs = run_trainer(rmat12, hip_device, torch_sgd(), d, **shape)
    assert_same_training(ours, theirs)
    model, opt, _, batches, init = ours
    V = rmat12.vocab_size
    assert V == 4097
    assert opt.last_apply == {model.input_weight: 'rows', model.output_weight: 'rows'}
    assert float(model.input_weight.grad.abs().max()) == 0.0
    assert float(model.output_weight.grad.abs().max()) == 0.0
    # rows outside the listed ids never moved
    n_centres = 4 * (12 - 2 * 2)
    in_ids = torch.cat([w[:, 2:10].reshape(-1) for w in batches]).long()
    noise = [device_noise(n_centres, 4, 2, V, SEED, k * n_centres, hip_device).reshape(-1)
             for k in range(5)]
    out_ids = torch.cat([w.reshape(-1).long() for w in batches] + noise)
    for p, p0, ids in ((model.input_weight, init[0], in_ids), (model.output_weight, init[1], out_ids)):
        rest = torch.ones(V, dtype=torch.bool, device=hip_device)
        rest[ids] = False
        assert int(rest.sum()) > V // 2
        assert torch.equal(p.detach()[rest], p0[rest])
        assert not torch.equal(p.detach()[~rest], p0[~rest])


@pytest.mark.parametrize('d', [8, 128])
def test_trainer_large_batch_goes_dense(hip_device, rmat12, d):
    """300 walks of L = 30, R = 3, K = 4: 7,200 centres and 181,800 out ids, both >= V."""
    shape = dict(n_walks=300, L=30, R=3, K=4)
    ours = run_trainer(rmat12, hip_device, hip_sgd(), d, **shape)
    theirs = run_trainer(rmat12, hip_device, torch_sgd(), d, **shape)
    assert_same_training(ours, theirs)
    model, opt = ours[:2]
    assert opt.last_apply == {model.input_weight: 'dense', model.output_weight: 'dense'}
    assert float(model.input_weight.grad.abs().max()) == 0.0
    assert float(model.output_weight.grad.abs().max()) == 0.0


def test_trainer_momentum_runs_through_step(hip_device, rmat12):
    """Momentum (with nesterov and weight decay): the unfused SGNS step, then step() (dense)."""
    kw = dict(momentum=0.9, nesterov=True, weight_decay=1e-4)
    shape = dict(n_walks=300, L=30, R=3, K=4, lr=0.1)
    ours = run_trainer(rmat12, hip_device, hip_sgd(**kw), 128, **shape)
    theirs = run_trainer(rmat12, hip_device, torch_sgd(**kw), 128, **shape)
    assert_same_training(ours, theirs)
    model, opt = ours[:2]
    assert opt.last_apply == {model.input_weight: 'dense', model.output_weight: 'dense'}
    assert float(model.output_weight.grad.abs().max()) == 0.0
    for po, pt in zip(model.parameters(), theirs[0].parameters()):
        np.testing.assert_allclose(opt.state[po]['momentum_buffer'].cpu().numpy(),
                                   theirs[1].state[pt]['momentum_buffer'].cpu().numpy(),
                                   rtol=1e-5, atol=1e-6)


def test_deterministic_mode_refuses_the_touched_rows_step(hip_device, rmat12, monkeypatch):
    monkeypatch.setenv('DW_DETERMINISTIC', '1')
    with pytest.raises(NotImplementedError, match='no deterministic mode'):
        run_trainer(rmat12, hip_device, hip_sgd(), 8, n_walks=4, L=12, R=2, K=2)
