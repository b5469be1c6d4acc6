"""Unigram^0.75 negative sampling without a GPU: the native alias-table build
(dw_noise_alias_build, host code) against its Python restatement (tests/noise_ref.py), the law
the table and the restated sampler represent, and the trainer's argument checks."""
import math

import numpy as np
import pytest
import torch

import noise_ref
from shallow_encoders import _native
from shallow_encoders.word2vec.sgns import unigram_table_host

W7 = np.array([0.0, 3.0, 1.0, 0.0, 10.0, 2.5, 0.5])   # V = 7, two zero weights


def _zipf(V=4097, zeros=64):
    w = np.arange(1, V + 1, dtype=np.float64) ** -1.2
    w[:zeros] = 0.0
    return w


def _native_table(w) -> np.ndarray:
    w = np.ascontiguousarray(w, dtype=np.float64)
    table = np.empty(len(w), dtype=np.uint64)
    _native.call('dw_noise_alias_build', w.ctypes.data, len(w), table.ctypes.data)
    return table


CASES = {'v7_two_zeros': W7, 'v1': np.array([2.5]), 'zipf_4097_first_64_zero': _zipf()}


@pytest.mark.parametrize('name', list(CASES))
def test_native_build_equals_restatement(name):
    w = CASES[name]
    got, want = _native_table(w), noise_ref.alias_table(w)
    assert got.dtype == want.dtype == np.uint64
    np.testing.assert_array_equal(got, want)
    assert int((got >> np.uint64(32)).max()) < len(w)   # every alias is an id


@pytest.mark.parametrize('name', list(CASES))
def test_table_mass_is_the_weights(name):
    """|mass_i - w_i / sum| <= (m_i + 1) 2^-32 / V + 1e-15, m_i = slots aliased to i: each slot's
    threshold is floor(p 2^32) (error < 2^-32 of the slot's 1/V, falling on the slot's id and on
    its alias), and the float64 build's own rounding stays below 1e-15. Zero weight: mass 0."""
    w = CASES[name]
    V = len(w)
    table = _native_table(w)
    mass = noise_ref.table_mass(table)
    thr = table & np.uint64(0xFFFFFFFF)
    alias = (table >> np.uint64(32)).astype(np.int64)
    m = np.bincount(alias[thr != np.uint64(0xFFFFFFFF)], minlength=V)
    err = np.abs(mass - w / w.sum())
    assert np.all(err <= (m + 1) * 2.0 ** -32 / V + 1e-15), float(err.max())
    assert np.all(mass[w == 0.0] == 0.0)
    assert abs(mass.sum() - 1.0) < 1e-12


def test_unigram_table_host_takes_the_power_in_float64():
    counts = torch.tensor([0, 5, 1, 0, 81, 16, 2], dtype=torch.int32)
    got = unigram_table_host(counts, power=0.75).numpy()
    want = noise_ref.alias_table(counts.double().pow(0.75).numpy())
    np.testing.assert_array_equal(got, want)
    mass = noise_ref.table_mass(got)
    law = counts.double().numpy() ** 0.75
    np.testing.assert_allclose(mass, law / law.sum(), atol=1e-9)


@pytest.mark.parametrize('w, what', [([1.0, -0.5, 2.0], b'negative or not finite'),
                                     ([1.0, float('nan')], b'negative or not finite'),
                                     ([1.0, float('inf')], b'negative or not finite'),
                                     ([0.0, 0.0, 0.0], b'positive, finite sum')])
def test_build_refuses_bad_weights(w, what):
    lib = _native.load()
    w = np.array(w, dtype=np.float64)
    table = np.zeros(len(w), dtype=np.uint64)
    rc = lib.dw_noise_alias_build(w.ctypes.data, len(w), table.ctypes.data)
    assert rc == _native.DW_E_INVALID_ARG
    assert what in lib.dw_last_error_string()


def test_build_refuses_bad_sizes():
    lib = _native.load()
    w = np.ones(4)
    table = np.zeros(4, dtype=np.uint64)
    for V in (0, -3, 2 ** 31):   # (sizes are tested before anything is read)
        assert lib.dw_noise_alias_build(w.ctypes.data, V, table.ctypes.data) == \
            _native.DW_E_INVALID_ARG
        assert b'[1, 2^31)' in lib.dw_last_error_string()
    assert lib.dw_noise_alias_build(None, 4, table.ctypes.data) == _native.DW_E_INVALID_ARG
    with pytest.raises(_native.DWError):
        unigram_table_host(torch.zeros(5))


def test_restated_sampler_law_is_unigram_075():
    """400 x 4 x 5 draws of the restated sampler at V = 7, seed fixed: chi-square against
    w^0.75 / sum over the 5 positive ids (4 degrees of freedom, survival function
    exp(-x/2) (1 + x/2)) gives p > 1e-3, and the zero-weight ids are never drawn."""
    law = W7 ** 0.75
    table = noise_ref.alias_table(law)
    ids = noise_ref.alias_noise(table, seed=20241019, noise_offset=12345, n_centres=400, n_ctx=4,
                                k=5)
    assert ids.shape == (400, 4, 5)
    counts = np.bincount(ids.ravel(), minlength=7)
    assert counts[0] == 0 and counts[3] == 0
    pos = law > 0
    expect = ids.size * law[pos] / law.sum()
    x = float(((counts[pos] - expect) ** 2 / expect).sum())
    p = math.exp(-x / 2) * (1 + x / 2)
    print(f'chi2 = {x:.3f}, p = {p:.4f}')
    assert p > 1e-3, (x, p)


def test_restated_sampler_equals_device_noise_oracle_on_equal_weights():
    """Equal weights: every entry is 'always keep', the draw is its slot — oracle/philox.py
    device_noise (what dw_sgns_noise writes), also across the counter's high word."""
    from oracle import philox as ph
    V = 1001
    table = noise_ref.alias_table(np.full(V, 3.0))
    assert np.all(table & np.uint64(0xFFFFFFFF) == np.uint64(0xFFFFFFFF))
    for off in (0, 2 ** 32 - 3):
        np.testing.assert_array_equal(noise_ref.alias_noise(table, 7, off, 6, 3, 3),
                                      ph.device_noise(7, off, 6, 3, 3, V))


def _trainer(**kw):
    from shallow_encoders.word2vec.model import SkipGram
    from shallow_encoders.word2vec.optim import Adam
    from shallow_encoders.word2vec.trainer import Word2VecTrainer
    model = SkipGram(7, 8)
    return Word2VecTrainer(model, Adam(model.parameters(), lr=0.1), None, neg_samples=3,
                           vocab_size=7, **kw)


def test_trainer_unigram_arguments():
    with pytest.raises(ValueError, match='noise_weights'):
        _trainer(noise='unigram')
    with pytest.raises(ValueError, match='vocab_size = 7'):
        _trainer(noise='unigram', noise_weights=torch.ones(6))
    with pytest.raises(ValueError, match='"torch", "device" or "unigram"'):
        _trainer(noise='bigram')
    with pytest.raises(ValueError, match='only used by'):
        _trainer(noise='device', noise_weights=torch.ones(7))
    with pytest.raises(_native.DWError):
        _trainer(noise='unigram', noise_weights=-torch.ones(7))
    tr = _trainer(noise='unigram', noise_weights=torch.as_tensor(W7))   # no device needed
    np.testing.assert_array_equal(tr._noise_table_host.numpy(),
                                  noise_ref.alias_table(W7 ** 0.75))


def test_config_unigram_weights_are_degrees_and_text_is_refused():
    from shallow_encoders.config_parser import load_config
    from shallow_encoders.config_parser.core import unigram_weights
    c = load_config('sge_sg_karate_club', overrides=['train.noise=unigram'])
    assert c.train.noise == 'unigram' and c.train.noise_power == 0.75
    assert load_config('sge_sg_karate_club').train.noise_power == 0.75
    ds = c.datamodule.instantiate_dataset()
    w = unigram_weights(ds).numpy()
    assert w.dtype == np.float64 and len(w) == len(ds.vocab)
    csr = ds.dataset.csr
    assert csr.weighted   # networkx's karate club carries edge weights: the weighted degrees
    want = [csr.weights[csr.row_ptr[i]:csr.row_ptr[i + 1]].sum() for i in range(len(w))]
    np.testing.assert_array_equal(w, want)
    assert w[0] == 0 and w[1:].min() >= 1

    from shallow_encoders.graph.csr import CSRGraph
    plain = CSRGraph.from_arrays(csr.row_ptr, csr.host_col())   # unweighted: the degrees

    class Wrap:
        class dataset:
            csr = plain
    np.testing.assert_array_equal(unigram_weights(Wrap()).numpy(), np.diff(csr.row_ptr))

    class Text:   # a text dataset has no CSR behind it
        pass
    with pytest.raises(ValueError, match='noise_weights'):
        unigram_weights(Text())
