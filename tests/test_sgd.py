"""The SGD optimizer (csrc/dw_sgd.hip, word2vec/optim.SGD), the parts that need no GPU: the numpy
restatement (tests/sgd_ref.py) against torch.optim.SGD on CPU fp32 bit for bit, the constructor,
the config substitution, the entry points' argument checks through ctypes and the rows-or-dense
rule."""
import numpy as np
import pytest
import torch

import sgd_ref
from shallow_encoders import _native
from sgd_ref import mixed_grads
from shallow_encoders.word2vec import optim


@pytest.mark.parametrize('name', sorted(sgd_ref.OPTION_SETS))
def test_restatement_equals_torch_sgd_bit_for_bit(name):
    """3 steps on a 257 x 100 table, lr changed before the third: every entry of the parameter
    (and of the momentum buffer) equals torch.optim.SGD's on CPU fp32 tensors, bit for bit."""
    opts = sgd_ref.OPTION_SETS[name]
    rng = np.random.default_rng(7)
    p0 = (rng.standard_normal((257, 100)) * 0.1).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    topt = torch.optim.SGD([tp], lr=0.05, foreach=False, **opts)
    p, buf = p0.copy(), None
    for step in range(3):
        lr = 0.05 if step < 2 else 0.0125
        topt.param_groups[0]['lr'] = lr
        g = mixed_grads(rng, p.shape)
        tp.grad = torch.from_numpy(g.copy())
        topt.step()
        p, buf = sgd_ref.sgd_step(p, g, buf, lr, **opts)
        np.testing.assert_array_equal(p.view(np.uint32), tp.detach().numpy().view(np.uint32))
        if opts.get('momentum'):
            tb = topt.state[tp]['momentum_buffer'].numpy()
            np.testing.assert_array_equal(buf.view(np.uint32), tb.view(np.uint32))
        else:
            assert buf is None and 'momentum_buffer' not in topt.state[tp]


def test_rows_restatement_is_the_dense_one_on_the_listed_rows():
    rng = np.random.default_rng(3)
    p = rng.standard_normal((37, 6)).astype(np.float32)
    g = mixed_grads(rng, p.shape)
    ids = np.array([5, 5, 36, 0, 5, 40, -1])          # duplicates and two ids out of range
    p1, g1 = sgd_ref.sgd_rows(p, g, ids, 0.3)
    dense, _ = sgd_ref.sgd_step(p, g, None, 0.3)
    listed = np.array([0, 5, 36])
    rest = np.setdiff1d(np.arange(37), listed)
    np.testing.assert_array_equal(p1[listed].view(np.uint32), dense[listed].view(np.uint32))
    np.testing.assert_array_equal(p1[rest].view(np.uint32), p[rest].view(np.uint32))
    np.testing.assert_array_equal(g1[rest].view(np.uint32), g[rest].view(np.uint32))
    assert not g1[listed].any()


# ---- the constructor ----------------------------------------------------------------------------
def _params():
    return [torch.nn.Parameter(torch.zeros(3, 2))]


@pytest.mark.parametrize('kw', [dict(lr=-0.1), dict(lr=0.1, momentum=-0.5),
                                dict(lr=0.1, weight_decay=-1e-3),
                                dict(lr=0.1, nesterov=True),
                                dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1)])
def test_constructor_refuses_what_torch_refuses(kw):
    with pytest.raises(ValueError) as theirs:
        torch.optim.SGD(_params(), **kw)
    with pytest.raises(ValueError) as ours:
        optim.SGD(_params(), **kw)
    assert str(ours.value) == str(theirs.value)


@pytest.mark.parametrize('kw', [dict(), dict(lr=0.0), dict(lr=0.5, momentum=0.9),
                                dict(lr=0.5, momentum=0.9, nesterov=True, weight_decay=1e-4),
                                dict(lr=0.5, momentum=0.9, dampening=0.5),
                                dict(lr=0.5, maximize=False, foreach=None, fused=None,
                                     differentiable=False)])
def test_constructor_accepts_what_torch_accepts(kw):
    theirs = torch.optim.SGD(_params(), **kw)
    ours = optim.SGD(_params(), **kw)
    assert ours.param_groups[0].keys() == theirs.param_groups[0].keys()
    for k in ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov'):
        assert ours.param_groups[0][k] == theirs.param_groups[0][k], k
    assert ours.zero_grad_in_step and ours.last_apply == {}


@pytest.mark.parametrize('flag', ['maximize', 'foreach', 'fused', 'differentiable'])
def test_unsupported_flags_raise(flag):
    with pytest.raises(NotImplementedError, match=flag):
        optim.SGD(_params(), lr=0.1, **{flag: True})


def test_state_dict_has_torch_format():
    """The param group keys are torch's, so the state loads into torch.optim.SGD and back."""
    ours = optim.SGD(_params(), lr=0.25, momentum=0.9)
    theirs = torch.optim.SGD(_params(), lr=0.1)
    theirs.load_state_dict(ours.state_dict())
    assert theirs.param_groups[0]['lr'] == 0.25 and theirs.param_groups[0]['momentum'] == 0.9
    ours.load_state_dict(theirs.state_dict())


def test_host_tensors_are_refused_not_stepped_on_the_cpu():
    p = _params()
    p[0].grad = torch.ones(3, 2)
    with pytest.raises(TypeError, match='HIP device'):
        optim.SGD(p, lr=0.1).step()


# ---- the config substitution --------------------------------------------------------------------
def test_config_substitutes_sgd_like_adam():
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.config_parser.core import TARGET_SUBSTITUTES
    assert TARGET_SUBSTITUTES['torch.optim.SGD'] == 'shallow_encoders.word2vec.optim.SGD'
    c = load_config('sge_sg_karate_club', overrides=['train.optimizer._target_=torch.optim.SGD',
                                                     'train.optimizer.lr=0.5'])
    opt = c.train.instantiate_optimizer(_params())
    assert type(opt) is optim.SGD and opt.param_groups[0]['lr'] == 0.5
    sched = c.train.instantiate_scheduler(opt)       # torch's schedulers take it unchanged
    assert sched.optimizer is opt
    adam = load_config('sge_sg_karate_club').train.instantiate_optimizer(_params())
    assert type(adam) is optim.Adam


def test_shipped_sgd_config_is_the_rmat20_config_under_sgd():
    from shallow_encoders.config_parser import load_config_dict
    sgd, adam = load_config_dict('sge_sg_rmat20_sgd'), load_config_dict('sge_sg_rmat20')
    assert sgd['train']['optimizer'] == {'_target_': 'torch.optim.SGD', 'lr': 10000.0}
    assert sgd['train'].pop('experiment') != adam['train'].pop('experiment')
    del sgd['train']['optimizer'], adam['train']['optimizer']
    assert sgd == adam


# ---- the entry points' argument checks (no device call is made) ---------------------------------
def _dense(param=1 << 12, grad=1 << 13, buf=None, n=8, mu=0.0):
    lib = _native.load()
    rc = lib.dw_sgd_dense(param, grad, buf, n, -0.1, 0.0, mu, 1.0, 0, 0, 1, None)
    return rc, lib.dw_last_error_string()


def _rows(param=1 << 12, grad=1 << 13, V=100, d=8, ids=1 << 14, id_bytes=4, n=5,
          claim=1 << 15, nlr=-0.1):
    lib = _native.load()
    rc = lib.dw_sgd_rows(param, grad, V, d, ids, id_bytes, n, claim, nlr, None, None)
    return rc, lib.dw_last_error_string()


@pytest.mark.parametrize('kw,msg', [
    (dict(param=None), b'dw_sgd_dense: null pointer'),
    (dict(grad=None), b'dw_sgd_dense: null pointer'),
    (dict(n=-1), b'dw_sgd_dense: negative size'),
    (dict(mu=0.9), b'momentum != 0 needs a momentum buffer'),
])
def test_dense_abi_rejects_bad_arguments_without_a_device(kw, msg):
    rc, err = _dense(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert msg in err, err


@pytest.mark.parametrize('kw,msg', [
    (dict(param=None), b'dw_sgd_rows: null pointer'),
    (dict(grad=None), b'dw_sgd_rows: null pointer'),
    (dict(claim=None), b'dw_sgd_rows: null pointer'),
    (dict(ids=None), b'dw_sgd_rows: null pointer'),
    (dict(id_bytes=2), b'id_bytes must be 4 (int32) or 8 (int64) (got 2)'),
    (dict(id_bytes=16), b'id_bytes must be 4 (int32) or 8 (int64) (got 16)'),
    (dict(d=0), b'dim must be >= 1 (got 0)'),
    (dict(d=-4), b'dim must be >= 1 (got -4)'),
    (dict(n=-1), b'negative id count'),
    (dict(V=0), b'n_table_rows must be in [1, 2^31)'),
    (dict(V=2 ** 31), b'n_table_rows must be in [1, 2^31)'),
    (dict(nlr=0.1), b'neg_lr must be <= 0'),
])
def test_rows_abi_rejects_bad_arguments_without_a_device(kw, msg):
    rc, err = _rows(**kw)
    assert rc == _native.DW_E_INVALID_ARG
    assert msg in err, err


def test_abi_empty_calls_are_no_ops_without_a_device():
    """n = 0 returns DW_OK before any launch (the pointers here are not device memory)."""
    assert _dense(n=0)[0] == _native.DW_OK
    assert _rows(n=0, ids=None)[0] == _native.DW_OK


# ---- rows or dense ------------------------------------------------------------------------------
def test_rows_or_dense_rule_at_its_boundary():
    V = 4097
    assert optim.ROWS_MAX_IDS_PER_ROW == 1
    assert optim.rows_apply(0, V) and optim.rows_apply(V - 1, V)
    assert not optim.rows_apply(V, V) and not optim.rows_apply(V + 1, V)
    # the shapes of the issue: 64 walks of C3 go by rows in both tables, the headline batch's
    # out table (2.9e7 negatives over 1,048,577 rows) goes dense
    V, L, R, K = 1_048_577, 80, 5, 5
    for n, want_in, want_out in ((64, True, True), (8192, True, False)):
        centres = n * (L - 2 * R)
        assert optim.rows_apply(centres, V) is want_in
        assert optim.rows_apply(n * L + centres * 2 * R * K, V) is want_out
