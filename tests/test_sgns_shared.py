"""Shared negatives per walk (dw_sgns_walks_shared), the parts that need no GPU: the float64
restatement (tests/shared_ref.py) against the oracle's closed form where the two coincide, the
entry point's argument checks through ctypes, the trainer's constructor errors and the config."""
import numpy as np
import pytest
import torch

import shared_ref
from oracle import sgns_ref
from shallow_encoders import _native
from shallow_encoders.word2vec.model import SkipGram
from shallow_encoders.word2vec.trainer import Word2VecTrainer


@pytest.mark.parametrize('n,L,R,K', [(3, 9, 2, 8), (2, 7, 1, 16), (1, 12, 3, 2)])
def test_restatement_equals_oracle_at_lambda_one(n, L, R, K):
    """S = 2R K (lambda = 1): the shared step is the reference's step fed the [B', 2R, K] tensor
    that repeats each walk's S ids for every one of its centres."""
    V, d, S = 23, 16, 2 * R * K
    rng = np.random.default_rng(n * 100 + L)
    w_in, w_out = sgns_ref.xavier_tables(V, d, seed=L)
    w_in, w_out = w_in * 20, w_out * 20          # logits of order 1
    walks = rng.integers(0, V, (n, L))
    ids = rng.integers(0, V, (n, S))
    ids[0, :3] = ids[0, 3]                        # repeats among the shared ids
    ids[-1, -1] = walks[-1, R]                    # a shared id that is a walk node (a centre)
    ref = shared_ref.shared_ref(walks, ids, w_in, w_out, R, K)
    assert ref['lam'] == 1.0 and not ref['bad']
    ins, tgt = sgns_ref.sg_windows(walks, R)
    noise = shared_ref.repeated_noise(walks, ids, R, K)
    loss, g_in, g_out = sgns_ref.sgns_grads_closed_form(w_in, w_out, ins, tgt, noise)
    M = n * (L - 2 * R) * 2 * R
    np.testing.assert_allclose((ref['acc'][0] + ref['acc'][1]) / M, loss, rtol=1e-13)
    np.testing.assert_allclose(ref['g_in'], g_in, rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(ref['g_out'], g_out, rtol=1e-11, atol=1e-15)
    # the counts, restated independently
    c = w_in.astype(np.float64)[ins.reshape(-1)]
    s = np.einsum('bd,bjd->bj', c, w_out.astype(np.float64)[tgt])
    t = np.einsum('bd,bjkd->bjk', c, w_out.astype(np.float64)[noise])
    assert ref['acc'][2] == (s >= 0).sum() and ref['acc'][3] == (t >= 0).sum()


def test_restatement_weights_the_negatives_and_drops_bad_ids():
    V, d, R, K, S, L = 17, 8, 2, 5, 32, 11
    rng = np.random.default_rng(5)
    w_in, w_out = (20 * t for t in sgns_ref.xavier_tables(V, d, seed=1))
    walks = rng.integers(0, V, (2, L))
    ids = rng.integers(0, V, (2, S))
    a = shared_ref.shared_ref(walks, ids, w_in, w_out, R, K)
    b = shared_ref.shared_ref(walks, ids, w_in, w_out, R, 2 * K)
    assert a['lam'] == 2 * R * K / S == 0.625
    np.testing.assert_allclose(b['acc'][[1, 3]], 2 * a['acc'][[1, 3]], rtol=1e-14)
    np.testing.assert_array_equal(b['acc'][[0, 2]], a['acc'][[0, 2]])
    # a bad shared id: the same as the batch with that column removed from the sums
    bad = ids.copy()
    bad[1, 4] = V + 3
    c = shared_ref.shared_ref(walks, bad, w_in, w_out, R, K)
    assert c['bad'] and np.isfinite(c['g_in']).all()
    h = w_in.astype(np.float64)[walks[1, R:L - R]]
    x = h @ w_out.astype(np.float64)[ids[1, 4]]
    drop = a['lam'] * (-np.log(np.maximum(1 / (1 + np.exp(x)), 1e-6))).sum()
    np.testing.assert_allclose(a['acc'][1] - c['acc'][1], drop, rtol=1e-10)


# ---- the entry point's argument checks (no device call is made) --------------------------------
def _call(L=20, R=2, K=5, S=32, V=100, d=64, n=4):
    lib = _native.load()
    rc = lib.dw_sgns_walks_shared(None, n, L, R, K, S, V, d, None, None, None, None, None, 1.0,
                                  None, None, None)
    return rc, lib.dw_last_error_string()


@pytest.mark.parametrize('kw,msg', [
    (dict(d=96), b'dim must be 64, 128 or 256 (got 96)'),
    (dict(S=48), b'n_shared must be a multiple of 32 in [32, 128] (got 48)'),
    (dict(S=160), b'n_shared must be a multiple of 32 in [32, 128] (got 160)'),
    (dict(L=129), b'walk_length 129 > 128'),
    (dict(L=4, R=2), b'walk_length 4 < 2R+1'),
    (dict(V=2 ** 31), b'vocab_size must be in [1, 2^31)'),
])
def test_abi_rejects_unsupported_shapes_without_a_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert msg in err, err


def test_abi_takes_a_supported_shape_up_to_the_pointers():
    """The limits pass; the null tables are what is refused then (still no device call)."""
    for kw in (dict(), dict(L=128, S=128, d=256), dict(L=5, R=2, S=32, d=64)):
        rc, err = _call(**kw)
        assert rc == _native.DW_E_INVALID_ARG and b'null pointer' in err, (kw, err)


def test_shape_check_of_the_host_side_agrees():
    from shallow_encoders.word2vec.sgns import shared_shape_error
    assert shared_shape_error(80, 5, 64, 128, 2 ** 20) is None
    assert shared_shape_error(128, 5, 128, 256, 2 ** 31 - 1) is None
    for bad in [(129, 5, 64, 128, 100), (10, 5, 64, 128, 100), (80, 5, 48, 128, 100),
                (80, 5, 160, 128, 100), (80, 5, 0, 128, 100), (80, 5, 64, 96, 100),
                (80, 5, 64, 128, 2 ** 31)]:
        assert shared_shape_error(*bad) is not None, bad


def test_byte_model():
    from shallow_encoders.word2vec.sgns import sgns_shared_bytes
    b = sgns_shared_bytes(8192, 80, 5, 64, 128)
    rows = 8192 * (70 + 144)                      # 214 rows per walk
    assert b['reads'] == rows * 512 + 8192 * (320 + 512)
    assert b['atomic_rows'] == rows * 512 and b['atomics'] == 2 * b['atomic_rows']


# ---- the trainer's constructor and the config --------------------------------------------------
def _make(**kw):
    model = kw.pop('model', None) or SkipGram(30, 64)
    return Word2VecTrainer(model, None, None, neg_samples=5, vocab_size=30, context_radius=2, **kw)


def test_trainer_constructor_errors():
    with pytest.raises(ValueError, match='noise="torch"'):
        _make(noise='torch', shared_negatives=32)
    with pytest.raises(ValueError, match='noise="torch"'):
        _make(shared_negatives=32)                # 'torch' is the default noise
    with pytest.raises(ValueError, match='max_norm'):
        _make(noise='device', shared_negatives=32, model=SkipGram(30, 64, max_norm=1.0))
    with pytest.raises(ValueError, match='>= 0'):
        _make(noise='device', shared_negatives=-32)
    assert _make(noise='device', shared_negatives=32)._shared == 32
    assert _make(noise='unigram', shared_negatives=64,
                 noise_weights=torch.ones(30))._shared == 64
    assert _make()._shared == 0                   # off by default: the reference's step


def test_config_field():
    from shallow_encoders.config_parser import load_config
    assert load_config('sge_sg_karate_club').train.shared_negatives == 0
    c = load_config('sge_sg_karate_club', overrides=['train.shared_negatives=32'])
    assert c.train.shared_negatives == 32
    import glob
    import os
    from shallow_encoders.common.path import CONFIG_PATH
    for path in glob.glob(os.path.join(CONFIG_PATH, '*.yaml')):   # no shipped config turns it on
        assert 'shared_negatives' not in open(path).read(), path
