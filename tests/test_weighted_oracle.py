"""The alias oracle (oracle/philox.alias_tables, the restatement dw_alias_build is pinned to bit
for bit) REPRESENTS its weights on a graph with hub rows, zero weights and heavy-tailed rows:
every entry's mass is within the truncation the table's 32-bit thresholds allow — not an
absolute tolerance — and a zero-weight entry carries no mass at all."""
import numpy as np
import pytest

from oracle import philox as ph

import weighted_ref as wr


@pytest.mark.parametrize('family', wr.FAMILIES)
def test_alias_oracle_represents_hub_graph_weights(family):
    csr = wr.hub_graph()
    w = wr.sym_weights(csr, family)
    prob, alias = ph.alias_tables(csr.row_ptr, w)
    worst, zero_mass = wr.alias_mass_error(csr.row_ptr, prob, alias, w)
    print(f'{family}: worst |mass - w / sum w| n / bound = {worst:.4f}, '
          f'zero-weight entries with mass: {zero_mass}')
    assert worst <= 1.0
    assert zero_mass == 0


def test_weight_families_are_symmetric_and_as_described():
    csr = wr.hub_graph()
    rp, col = np.asarray(csr.row_ptr), np.asarray(csr.host_col())
    deg = np.diff(rp)
    row = np.repeat(np.arange(len(deg)), deg)
    back = {(int(r), int(c)): e for e, (r, c) in enumerate(zip(row, col))}
    rev = np.array([back[(int(c), int(r))] for r, c in zip(row, col)])
    for family in wr.FAMILIES:
        w = wr.sym_weights(csr, family)
        np.testing.assert_array_equal(w, w[rev])
        assert (np.add.reduceat(w, rp[1:-1]) > 0).all()
    # the replay families keep every partial sum exact (rng='python' takes them on any CPython)
    from shallow_encoders.graph.csr import CSRGraph
    from shallow_encoders.graph.random_walk_generator import sum_is_exact
    for family in ('int', 'dyadic', 'zeros'):
        g = CSRGraph.from_arrays(csr.row_ptr, csr.col, wr.sym_weights(csr, family), itos=csr.itos)
        assert sum_is_exact(g, 1.0, 1.0, node2vec=False)
        for p, q in ((0.25, 4.0), (2.0, 0.5)):
            assert sum_is_exact(g, 1.0 / p, 1.0 / q, node2vec=True)
    z = wr.sym_weights(csr, 'zeros')
    assert 0.08 < (z == 0).mean() < 0.12
    first, last = rp[1:-1], rp[2:] - 1            # every row but <unk>'s has a neighbour
    assert (z[first] == 0).any() and (z[last] == 0).any()
    s = wr.sym_weights(csr, 'skew')
    assert 0.01 < (s == 1000.0).mean() < 0.03


def test_alias_mass_error_sees_a_wrong_table():
    """The check itself: one threshold moved by 2^-20 of its column, or one alias moved to the
    neighbouring entry, is far outside the bound; a zero-weight entry made ALWAYS is counted."""
    csr = wr.hub_graph()
    w = wr.sym_weights(csr, 'zeros')
    prob, alias = ph.alias_tables(csr.row_ptr, w)
    rp = np.asarray(csr.row_ptr)
    a, b = int(rp[wr.HUB_ID]), int(rp[wr.HUB_ID + 1])
    j = a + int(np.flatnonzero((prob[a:b] != ph.ALWAYS) & (prob[a:b] > 1 << 20))[0])
    bad = prob.copy()
    bad[j] -= 1 << 12
    assert wr.alias_mass_error(rp, bad, alias, w)[0] > 100
    bad_alias = alias.copy()
    bad_alias[j] = (alias[j] + 1) % (b - a)
    assert wr.alias_mass_error(rp, prob, bad_alias, w)[0] > 100
    z = int(np.flatnonzero(w == 0)[0])
    bad = prob.copy()
    bad[z] = ph.ALWAYS
    assert wr.alias_mass_error(rp, bad, alias, w)[1] == 1
