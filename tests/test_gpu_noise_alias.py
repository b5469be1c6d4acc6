"""Unigram^0.75 negative sampling on the MI355X: the device alias sampler
(dw_sgns_noise_alias) against its restatement (tests/noise_ref.py) bit for bit, under a bound
step block, and through Word2VecTrainer(noise='unigram'), the graph-replayed step and the config
path. Training comparisons run in the deterministic mode (DW_DETERMINISTIC=1: integer gradient
sums), where equal negatives give equal bits."""
import random

import numpy as np
import pytest
import torch

import noise_ref
from oracle import philox as ph
from shallow_encoders import _native
from shallow_encoders.word2vec.model import SkipGram
from shallow_encoders.word2vec.optim import Adam
from shallow_encoders.word2vec.sgns import device_noise, unigram_noise, unigram_table
from shallow_encoders.word2vec.trainer import Word2VecTrainer

pytestmark = pytest.mark.gpu


def _zipf(V, zeros):
    w = np.arange(1, V + 1, dtype=np.float64) ** -1.2
    w[:zeros] = 0.0
    return w


def _draw(weights, B, C, K, seed, off, dev):
    """(device ids, restated ids) for the table of ``weights`` (power 1: the weights as given)."""
    table = unigram_table(torch.as_tensor(weights), power=1.0, device=dev)
    host = noise_ref.alias_table(weights)
    np.testing.assert_array_equal(table.cpu().numpy(), host)
    got = unigram_noise(B, C, K, table, seed, off, dev)
    assert got.shape == (B, C, K) and got.dtype == torch.int64
    return got.cpu().numpy(), noise_ref.alias_noise(host, seed, off, B, C, K)


@pytest.mark.parametrize('case', ['odd_slots', 'high_word', 'v1', 'equal_1m'])
def test_sampler_equals_restatement(case, hip_device):
    if case == 'odd_slots':      # C*K = 9: every centre ends on a lone slot (8-B stores)
        w = np.array([0.0, 3.0, 1.0, 0.0, 10.0, 2.5, 0.5])
        got, want = _draw(w, 5, 3, 3, 77, 3, hip_device)
        assert not np.isin(got, [0, 3]).any()
    elif case == 'high_word':    # centres 2^32 - 100 .. 2^32 + 199: the counter's high word moves
        w = _zipf(4097, 64)
        got, want = _draw(w, 300, 4, 5, 0x1234567890ABCDEF, 2 ** 32 - 100, hip_device)
        assert got.min() >= 64
    elif case == 'v1':
        got, want = _draw(np.array([2.5]), 9, 2, 3, 1, 0, hip_device)
        assert not got.any()
    else:                        # equal weights: the uniform device stream itself
        V = 1_048_577
        got, want = _draw(np.ones(V), 64, 4, 5, 9, 2 ** 40 + 5, hip_device)
        uni = device_noise(64, 4, 5, V, 9, 2 ** 40 + 5, hip_device).cpu().numpy()
        np.testing.assert_array_equal(got, uni)
        np.testing.assert_array_equal(got, ph.device_noise(9, 2 ** 40 + 5, 64, 4, 5, V))
    np.testing.assert_array_equal(got, want)


def test_out_buffer_and_multi_block_grid_stride(hip_device):
    """More Philox calls than the capped grid has lanes (2,048 blocks of 256): the grid-stride
    loop covers the rest; a caller's buffer is filled in place, a wrong one refused."""
    w = _zipf(4097, 64)
    table = unigram_table(torch.as_tensor(w), power=1.0, device=hip_device)
    B, C, K = 70_000, 4, 4                       # 560,000 calls > 524,288 lanes
    buf = torch.full((B * C * K,), -1, dtype=torch.int64, device=hip_device)
    got = unigram_noise(B, C, K, table, 3, 11, hip_device, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    host = noise_ref.alias_table(w)
    np.testing.assert_array_equal(got.cpu().numpy(), noise_ref.alias_noise(host, 3, 11, B, C, K))
    with pytest.raises(ValueError):
        unigram_noise(B, C, K, table, 3, 11, hip_device, out=buf[:-1])
    # an out buffer that is only 8-B aligned takes the 8-B stores: the same ids
    odd = torch.empty(5 * 2 * 4 + 1, dtype=torch.int64, device=hip_device)[1:]
    assert odd.data_ptr() % 16 == 8
    np.testing.assert_array_equal(
        unigram_noise(5, 2, 4, table, 3, 11, hip_device, out=odd).cpu().numpy(),
        noise_ref.alias_noise(host, 3, 11, 5, 2, 4))


def test_fill_reads_the_bound_step_block(hip_device):
    """With a dw_step_scalars block bound the centre counter is the block's, not the
    argument's (a captured step draws each replay's own negatives)."""
    from shallow_encoders.word2vec.graphed import _STEP_DTYPE
    w = _zipf(4097, 64)
    table = unigram_table(torch.as_tensor(w), power=1.0, device=hip_device)
    X = 2 ** 33 + 12345
    blk = np.zeros(1, dtype=_STEP_DTYPE)
    blk['noise_offset'] = X
    block = torch.from_numpy(np.frombuffer(blk.tobytes(), dtype=np.uint8).copy()).to(hip_device)
    try:
        _native.call('dw_step_scalars_bind', block.data_ptr())
        got = unigram_noise(33, 4, 5, table, 21, 999, hip_device)
    finally:
        _native.call('dw_step_scalars_bind', None)
    torch.cuda.synchronize()
    host = noise_ref.alias_table(w)
    np.testing.assert_array_equal(got.cpu().numpy(), noise_ref.alias_noise(host, 21, X, 33, 4, 5))
    unbound = unigram_noise(33, 4, 5, table, 21, 999, hip_device)
    np.testing.assert_array_equal(unbound.cpu().numpy(),
                                  noise_ref.alias_noise(host, 21, 999, 33, 4, 5))


# ---- the trainer ---------------------------------------------------------------------------
V, D, R, K, L, SEED = 35, 16, 2, 3, 10, 5
DEG = np.r_[0.0, np.random.default_rng(1).integers(1, 18, V - 1)].astype(np.float64)


def _trainer(noise, dev, **kw):
    torch.manual_seed(3)
    model = SkipGram(V, D).to(dev)
    opt = Adam(model.parameters(), lr=0.05)
    tr = Word2VecTrainer(model, opt, None, neg_samples=K, vocab_size=V, noise=noise, seed=SEED,
                         context_radius=R, **kw)
    tr.manual_grads = True
    return tr, model, opt


def _tables(model):
    return [p.detach().cpu().numpy().view(np.int32).copy()
            for p in (model.input_weight, model.output_weight)]


def test_trainer_unigram_steps_equal_replayed_restated_negatives(hip_device, monkeypatch):
    """noise='unigram' steps == the same steps fed the restated negatives (noise='torch'
    machinery, _noise_override), bit for bit in the deterministic mode: the trainer draws from
    weights^0.75 with its seed and its running centre counter."""
    monkeypatch.setenv('DW_DETERMINISTIC', '1')
    rng = np.random.default_rng(0)
    batches = [torch.as_tensor(rng.integers(1, V, size=(n, L)).astype(np.int32)).to(hip_device)
               for n in (20, 20, 13, 20)]
    tr, model, opt = _trainer('unigram', hip_device, noise_weights=torch.as_tensor(DEG))
    losses = []
    for wk in batches:
        losses.append(tr.training_step(wk)['loss'])
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    assert tr._noise_offset == sum(b.shape[0] for b in batches) * (L - 2 * R)
    got = _tables(model)

    host = noise_ref.alias_table(DEG ** 0.75)
    np.testing.assert_array_equal(tr._noise_table.cpu().numpy(), host)
    tr2, model2, opt2 = _trainer('torch', hip_device)
    off, losses2 = 0, []
    for wk in batches:
        n_c = wk.shape[0] * (L - 2 * R)
        ids = noise_ref.alias_noise(host, SEED, off, n_c, 2 * R, K)
        assert ids.min() >= 1
        tr2._noise_override = torch.as_tensor(ids).to(hip_device)
        losses2.append(tr2.training_step(wk)['loss'])
        opt2.step()
        opt2.zero_grad()
        off += n_c
    tr2._noise_override = None
    torch.cuda.synchronize()
    for a, b in zip(got, _tables(model2)):
        np.testing.assert_array_equal(a, b)
    # (the loss sums are float64 atomics over blocks: equal up to their order)
    np.testing.assert_allclose([float(x) for x in losses], [float(x) for x in losses2],
                               rtol=1e-6)


def _karate_run(graph: bool, dev):
    from shallow_encoders.graph.datasets import KarateClubDataset
    from shallow_encoders.word2vec.graphed import GraphedTrainerStep
    random.seed(0)   # the start-node shuffle
    ds = KarateClubDataset(walks_per_node=8, walk_length=L, method='deepwalk', rng='philox',
                           seed=1, device=dev)
    deg = np.diff(ds.csr.row_ptr).astype(np.float64)
    tr, model, opt = _trainer('unigram', dev, noise_weights=torch.as_tensor(deg))
    assert GraphedTrainerStep.eligible(tr, ds)
    B = 16

    def eager():
        tr.training_step(ds.next_walk_batch(B, check=False))
        opt.step()
        opt.zero_grad()
    eager()                                   # creates the Adam state, workspaces, noise buffer
    if graph:
        gs = GraphedTrainerStep(tr, ds, B, 4, unroll=4, scatter='records')
        assert gs._noise_ref is tr._noise_bufs[(B * (L - 2 * R), 2 * R)]
        terms = gs.replay()
        torch.cuda.synchronize()
        _native.check_status(gs.status, 'graphed unigram steps')
        assert np.isfinite(float(terms['loss']))
    else:
        for _ in range(4):
            eager()
    eager()                                   # and the eager loop goes on where the graph ended
    torch.cuda.synchronize()
    return _tables(model), tr._noise_offset, ds._index, tr._noise_bufs[(B * (L - 2 * R), 2 * R)]


def test_graphed_unigram_steps_equal_eager(hip_device, monkeypatch):
    """A 4-step GraphedTrainerStep replay == 4 eager steps, bit for bit (deterministic mode):
    the fill is captured inside each step under that step's bound block, into the persistent
    buffer, so each replayed step trains on its own negatives."""
    monkeypatch.setenv('DW_DETERMINISTIC', '1')
    t_e, off_e, idx_e, buf_e = _karate_run(False, hip_device)
    t_g, off_g, idx_g, buf_g = _karate_run(True, hip_device)
    assert off_e == off_g == 6 * 16 * (L - 2 * R) and idx_e == idx_g == 96
    for a, b in zip(t_e, t_g):
        np.testing.assert_array_equal(a, b)
    assert torch.equal(buf_e, buf_g)          # the last step's negatives


def test_config_path_builds_the_degree_law(hip_device):
    from shallow_encoders.config_parser import load_config
    c = load_config('sge_sg_karate_club',
                    overrides=['train.noise=unigram', 'train.seed=4', 'model.embedding_size=8',
                               'datamodule.additional_parameters.walks_per_node=2'])
    random.seed(0)
    ds = c.datamodule.instantiate_dataset()
    tr = c.instantiate_trainer(dataset=ds, device=hip_device)
    assert tr._noise_mode == 'unigram'
    csr = ds.dataset.csr
    n = len(ds.vocab)
    wdeg = np.array([(csr.weights[csr.row_ptr[i]:csr.row_ptr[i + 1]].sum() if csr.weighted
                      else csr.row_ptr[i + 1] - csr.row_ptr[i]) for i in range(n)], np.float64)
    law = wdeg ** 0.75
    mass = noise_ref.table_mass(tr._noise_table_host.numpy())
    np.testing.assert_allclose(mass, law / law.sum(), rtol=0, atol=1e-9)
    assert mass[0] == 0.0
    ids = tr._noise(4000, 4, hip_device)
    assert ids.shape == (4000, 4, 1)
    ids = ids.cpu().numpy()
    assert ids.min() >= 1 and ids.max() < n
    np.testing.assert_array_equal(
        ids, noise_ref.alias_noise(tr._noise_table_host.numpy(), 4, 0, 4000, 4, 1))
    # the law, loosely (16,000 draws: 5 sigma of a binomial count per id)
    counts = np.bincount(ids.ravel(), minlength=n)
    p = law / law.sum()
    assert np.all(np.abs(counts - ids.size * p) <= 5 * np.sqrt(ids.size * p * (1 - p)) + 1)
    tr.manual_grads = True
    loss = tr.training_step(next(iter(ds.walk_batches(64))))
    assert np.isfinite(float(loss['loss']))
