"""numpy restatement of the SGD chain of csrc/dw_sgd.hip (include/dw_hip.h dw_sgd_dense /
dw_sgd_rows), every fma a single rounding through oracle.adam_ref.fma32:

    g1  = wd != 0 ? fma(wd, p, g) : g
    buf = first ? g1 : fma(omd, g1, RN(mu * buf))          (mu != 0)
    g2  = mu == 0 ? g1 : nesterov ? fma(mu, buf, g1) : buf
    p   = fma(nlr, g2, p)

with the scalars prepared in float64 and cast to float32 as optim.SGD hands them to the kernels.
tests/test_sgd.py pins it to torch.optim.SGD on CPU fp32 bit for bit; the GPU tests pin the
kernels to it."""
import numpy as np

from oracle.adam_ref import fma32

F32 = np.float32

# the five option sets of the tests: plain, momentum, nesterov + weight_decay,
# dampening + weight_decay, weight_decay alone
OPTION_SETS = {
    'plain': dict(),
    'momentum': dict(momentum=0.9),
    'nesterov_wd': dict(momentum=0.9, nesterov=True, weight_decay=1e-2),
    'dampening_wd': dict(momentum=0.8, dampening=0.3, weight_decay=1e-3),
    'wd': dict(weight_decay=5e-2),
}


def mixed_grads(rng, shape):
    """Test gradients that mix the magnitudes 0, 1e-6, 1e-3 and 1 (random signs and mantissas;
    the zeros of both signs)."""
    mag = rng.choice(np.array([0.0, 1e-6, 1e-3, 1.0]), size=shape)
    return (mag * rng.standard_normal(shape)).astype(F32)


def scalars(lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """(nlr, wd, mu, omd) as float32, nesterov as bool."""
    return (F32(-float(lr)), F32(float(weight_decay)), F32(float(momentum)),
            F32(1.0 - float(dampening)), bool(nesterov))


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """One step over whole float32 arrays: returns (p', buf'); buf None = the first step (or no
    momentum), buf' None when momentum == 0."""
    nlr, wd, mu, omd, nest = scalars(lr, momentum, dampening, weight_decay, nesterov)
    p = np.asarray(p, dtype=F32)
    g1 = np.asarray(g, dtype=F32)
    with np.errstate(all='ignore'):
        if wd != 0:
            g1 = fma32(wd, p, g1)
        g2 = g1
        if mu != 0:
            buf = g1.copy() if buf is None else fma32(omd, g1, mu * np.asarray(buf, dtype=F32))
            g2 = fma32(mu, buf, g1) if nest else buf
        else:
            buf = None
        return fma32(nlr, g2, p), buf


def sgd_rows(p, g, ids, lr):
    """Plain SGD over the listed rows of [V, d] float32 tables: returns (p', g') with every
    distinct in-range row of ``ids`` stepped once and its gradient zeroed, every other row
    untouched."""
    p = np.array(p, dtype=F32)
    g = np.array(g, dtype=F32)
    ids = np.asarray(ids).reshape(-1)
    rows = np.unique(ids[(ids >= 0) & (ids < p.shape[0])])
    if rows.size:
        p[rows], _ = sgd_step(p[rows], g[rows], None, lr)
        g[rows] = 0
    return p, g
