"""The records gather of SGNS pass 2 (k_rec_gather): records staged 64 at a time, a row's Adam
state loaded when the row begins, one flush site. The tests choose how many records each out row
gets (explicit targets and noise), so that rows start and end at every offset of a staged block,
inside a chunk and across chunks, in the plain, fused-Adam, pieces, deterministic and lazy forms.
Gradients are compared with the float64 closed form at test_phase2_pieces_equal_phase2's bar."""
import numpy as np
import pytest
import torch

from oracle import sgns_ref

from shallow_encoders.word2vec import exact
from shallow_encoders.word2vec.sgns import (set_walk_agg, sgns_accumulate, sgns_phase2_pieces,
                                            walk_agg_active)
from test_gpu_sgns import assert_no_row_drift, assert_params_close

pytestmark = pytest.mark.gpu

# records per out row: around the group of 8, the 32-record chunk and the staged block of 64,
# and one row spanning dozens of chunks
LATTICE = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 1500]
GCH = 512


def _chunk(n_rec, device):
    """launch_pass2's chunk size: GCH, halved down to 32 while the chunks would not give every
    SIMD of the chip four waves."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    gch = GCH
    while gch > 32 and -(-n_rec // gch) < 16 * cus:
        gch >>= 1
    return gch


def _inside_one_chunk(keys, gch, V):
    """bool [V]: the rows with records, all of them inside one chunk of the sorted records (such a
    row is summed in registers by one wave; the others go through atomics), and the touched rows."""
    ks = np.sort(np.asarray(keys).reshape(-1))
    pos = np.arange(ks.size)
    first = np.full(V, ks.size, np.int64)
    last = np.full(V, -1, np.int64)
    np.minimum.at(first, ks, pos)
    np.maximum.at(last, ks, pos)
    touched = last >= 0
    return touched & (first // gch == last // gch), touched


def _ids_with_counts(counts, rng):
    """A shuffled id list in which row r occurs counts[r] times."""
    ids = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(ids)
    return ids


def _lattice_counts(n_ids, lo, V, rng, filler=3):
    """counts [V] summing to n_ids: the LATTICE rows and filler rows of `filler` records (the
    last one takes the rest), at shuffled rows of [lo, V)."""
    rest = n_ids - sum(LATTICE)
    assert rest > 0
    fill = [filler] * (rest // filler) + ([rest % filler] if rest % filler else [])
    per_row = LATTICE + fill
    assert lo + len(per_row) <= V, (lo, len(per_row), V)
    rows = lo + rng.permutation(V - lo)[:len(per_row)]
    counts = np.zeros(V, np.int64)
    counts[rows] = per_row
    return counts


def _pairs_case(V, d, K, counts, seed):
    rng = np.random.default_rng(seed)
    ids = _ids_with_counts(counts, rng)
    assert ids.size % (1 + K) == 0
    B = ids.size // (1 + K)
    targets, noise = ids[:B].reshape(B, 1), ids[B:].reshape(B, 1, K)
    inputs = rng.integers(0, V, B)
    w_in = (rng.random((V, d), dtype=np.float32) - 0.5)
    w_out = (rng.random((V, d), dtype=np.float32) - 0.5)
    return w_in, w_out, inputs, targets, noise


def _pairs_g_out(w_in, w_out, inputs, targets, noise, K, device):
    dv = [torch.as_tensor(x).to(device) for x in (w_in, w_out, inputs, targets, noise)]
    g_in, g_out = torch.zeros_like(dv[0]), torch.zeros_like(dv[1])
    sgns_accumulate(dv[0], dv[1], g_in, g_out, K, inputs=dv[2], targets=dv[3], noise=dv[4],
                    scatter='sorted')
    torch.cuda.synchronize()
    return g_out, dv


def _assert_g_close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))


@pytest.mark.parametrize('d', [64, 100, 128, 256, 512])
def test_row_length_lattice(hip_device, d):
    """Out rows of exactly 1 ... 129 and 1,500 records among 3-record rows, 3,505 records in all
    (1 mod 8, 49 mod 64) in 32-record chunks: g_out equals the float64 sum of coef * w_in over
    each row's records. d = 100 takes the masked instantiation."""
    V, K, B = 600, 4, 701
    n_rec = B * (1 + K)
    assert n_rec % 8 and n_rec % 64 and _chunk(n_rec, hip_device) == 32
    rng = np.random.default_rng(d)
    counts = _lattice_counts(n_rec, 0, V, rng)
    inside, touched = _inside_one_chunk(np.repeat(np.arange(V), counts), 32, V)
    assert inside.sum() > 300 and (touched & ~inside).sum() > 20   # both kinds of row
    case = _pairs_case(V, d, K, counts, d + 1)
    g_out, _ = _pairs_g_out(*case, K, hip_device)
    _, _, ref = sgns_ref.sgns_grads_closed_form(*case)
    got = g_out.cpu().numpy()
    assert not got[counts == 0].any()
    _assert_g_close(got, ref)


def test_full_chunk_path(hip_device):
    """Enough records that the chunk stays at 512 (16 x CUs x 512, as launch_pass2 counts): rows
    of 300 records, about four in ten of them inside one chunk, and one hub row of 5,000."""
    V, d, K = 7400, 128, 4
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    B = -(-16 * cus * GCH // (1 + K)) + 3
    n_rec = B * (1 + K)
    assert _chunk(n_rec, hip_device) == GCH and n_rec // 300 + 2 <= V
    per_row = [5000] + [300] * ((n_rec - 5000) // 300)
    per_row.append(n_rec - sum(per_row))
    rng = np.random.default_rng(5)
    counts = np.zeros(V, np.int64)
    counts[rng.permutation(V)[:len(per_row)]] = per_row
    inside, touched = _inside_one_chunk(np.repeat(np.arange(V), counts), GCH, V)
    assert inside.sum() > 1000 and (touched & ~inside).sum() > 1000
    case = _pairs_case(V, d, K, counts, 6)
    g_out, dv = _pairs_g_out(*case, K, hip_device)
    _, _, ref = sgns_ref.sgns_grads_closed_form_torch(*dv)
    _assert_g_close(g_out.cpu().numpy(), ref.cpu().numpy())


def _walks_case(V, n, L, R, K, n_nodes, counts_of, seed):
    """Walks over nodes [0, n_nodes) and replayed negatives whose ids occur counts_of(n_neg)[r]
    times; the sorted keys of the call's records without walk aggregation (every context, every
    negative)."""
    rng = np.random.default_rng(seed)
    walks = rng.integers(0, n_nodes, (n, L)).astype(np.int32)
    ins, tgt = sgns_ref.sg_windows(walks, R)
    n_neg = tgt.size * K
    noise = _ids_with_counts(counts_of(n_neg, rng), rng).reshape(len(ins), 2 * R, K)
    keys = np.concatenate([tgt.reshape(-1), noise.reshape(-1)])
    return walks, noise, keys


def _one_step(device, V, d, R, K, walks, noise, fuse):
    """One step from the seeded tables: phase 1, then phase 2 with the out table's Adam fused in,
    or plain phase 2 and the dense Adam. Returns the out table's p, m, v, the in table and the
    tables object."""
    from shallow_encoders.word2vec.sharding import ShardedTables
    t = ShardedTables(V, d, device, lr=0.02, init_seed=5)
    kw = dict(walks=walks, context_radius=R, noise=noise)
    sgns_accumulate(t.w_in, t.w_out, t.g_in, t.g_out, K, phase=1, **kw)
    t.exchange_in()
    spec = t.out_adam_spec() if fuse else None
    assert (spec is not None) == fuse
    sgns_accumulate(t.w_in, t.w_out, t.g_in, t.g_out, K, phase=2, out_adam=spec, **kw)
    t.exchange_out(fused_out=fuse)
    t.sync()
    torch.cuda.synchronize()
    return (t.w_out.clone(), t.m[1][:V].clone(), t.v[1][:V].clone(), t.w_in.clone(), t)


@pytest.mark.parametrize('d', [128, 256])
def test_fused_adam_equals_unfused_per_row(hip_device, d):
    """The lattice through the walks form (7,500 records, 4 mod 8, in 32-record chunks): a row
    wholly inside one chunk gets the same gradient and the same adam_elem fused and unfused, so
    its p, m, v are bit-equal; those rows are at least 90% of the touched ones. The rest
    (atomics at the chunk boundaries) meet assert_params_close's Adam-aware bar."""
    V, n, L, R, K, nodes = 2400, 25, 19, 2, 4, 300
    set_walk_agg(0)
    try:
        walks, noise, keys = _walks_case(
            V, n, L, R, K, nodes, lambda n_neg, rng: _lattice_counts(n_neg, nodes, V, rng, 2), d)
        assert keys.size % 8 and keys.size % 64 and _chunk(keys.size, hip_device) == 32
        inside, touched = _inside_one_chunk(keys, 32, V)
        assert inside.sum() >= 0.9 * touched.sum(), (inside.sum(), touched.sum())
        wk, nz = torch.as_tensor(walks).to(hip_device), torch.as_tensor(noise).to(hip_device)
        fused = _one_step(hip_device, V, d, R, K, wk, nz, True)
        plain = _one_step(hip_device, V, d, R, K, wk, nz, False)
    finally:
        set_walk_agg(-1)
    assert float(fused[4].grads.abs().max()) == 0.0 and int(fused[4]._row_flags.max()) == 0
    rows = torch.as_tensor(np.nonzero(inside)[0]).to(hip_device)
    for a, b, what in zip(fused[:3], plain[:3], 'pmv'):
        diff = (a[rows] != b[rows]).any(dim=1)
        assert not bool(diff.any()), (what, rows[diff][:10].tolist())
    for a, b in ((fused[0], plain[0]), (fused[3], plain[3])):
        assert_params_close(a.cpu().numpy(), b.cpu().numpy(), 0.02, max_frac=5e-3,
                            max_abs=2.05 * 0.02)
        assert_no_row_drift(a.cpu().numpy(), b.cpu().numpy())
    np.testing.assert_allclose(fused[1].cpu().numpy(), plain[1].cpu().numpy(), rtol=1e-3,
                               atol=1e-6)


def test_run_to_run_bit_identical(hip_device):
    """No row has more than 33 records and the chunks hold 32, so every row lies in at most two
    chunks and a boundary sum is two commuting adds: g_out, and the fused form's p, m, v, are
    bit-identical between two runs."""
    V, d, n, L, R, K, nodes = 3000, 128, 25, 19, 2, 4, 1500

    def counts_of(n_neg, rng):
        per_row = []
        while sum(per_row) + 33 <= n_neg:
            per_row.append(1 + len(per_row) % 33)
        per_row += [1] * (n_neg - sum(per_row))
        counts = np.zeros(V, np.int64)
        counts[nodes + rng.permutation(V - nodes)[:len(per_row)]] = per_row
        return counts

    set_walk_agg(0)
    try:
        walks, noise, keys = _walks_case(V, n, L, R, K, nodes, counts_of, 2)
        assert _chunk(keys.size, hip_device) == 32
        assert np.bincount(keys, minlength=V).max() <= 33
        ks = np.sort(keys)
        first = np.searchsorted(ks, np.arange(V), 'left')
        last = np.searchsorted(ks, np.arange(V), 'right') - 1
        assert (last // 32 - first // 32)[last >= first].max() == 1   # two chunks, and no more
        wk, nz = torch.as_tensor(walks).to(hip_device), torch.as_tensor(noise).to(hip_device)
        w_in0, w_out0 = sgns_ref.xavier_tables(V, d, seed=3)
        w_in, w_out = torch.as_tensor(w_in0).to(hip_device), torch.as_tensor(w_out0).to(hip_device)
        outs = []
        for _ in range(2):
            g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
            sgns_accumulate(w_in, w_out, g_in, g_out, K, walks=wk, context_radius=R, noise=nz)
            torch.cuda.synchronize()
            outs.append(g_out)
        assert float(outs[0].abs().max()) > 0 and torch.equal(outs[0], outs[1])
        a = _one_step(hip_device, V, d, R, K, wk, nz, True)
        b = _one_step(hip_device, V, d, R, K, wk, nz, True)
    finally:
        set_walk_agg(-1)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('agg', [0, 1])
def test_pieces_and_aggregate_records(hip_device, agg):
    """A walks call in 32-record chunks, walk aggregation off and on, through
    sgns_phase2_pieces in 1, 3 and 8 pieces: phase 2's g_out at its bar; in the deterministic
    mode bit-equal across the piece counts."""
    V, d, R, K, n, L = 900, 128, 3, 4, 40, 30
    g = torch.Generator().manual_seed(agg)
    walks = torch.randint(0, V, (n, L), generator=g, dtype=torch.int32)
    walks[:, ::4] = 5                                   # a hub row spanning many chunks
    walks = walks.to(hip_device)
    w_in = (torch.rand((V, d), generator=g) - 0.5).to(hip_device)
    w_out = (torch.rand((V, d), generator=g) - 0.5).to(hip_device)
    kw = dict(walks=walks, context_radius=R, seed=3)
    scale = 1.0 / (n * (L - 2 * R) * 2 * R)
    rows = {p: -(-V // p) for p in (1, 3, 8)}
    set_walk_agg(agg)
    try:
        assert walk_agg_active(n, L, R, K, d) == bool(agg)
        assert _chunk(n * (L - 2 * R) * 2 * R * (1 + K), hip_device) == 32
        ref_in, ref_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
        sgns_accumulate(w_in, w_out, ref_in, ref_out, K, **kw)
        for p in (1, 3, 8):
            g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
            sgns_accumulate(w_in, w_out, g_in, g_out, K, phase=1, **kw)
            sgns_phase2_pieces(w_in, g_out, K, walks=walks, context_radius=R, n_pieces=p,
                               piece_rows=rows[p])
            torch.cuda.synchronize()
            _assert_g_close(g_out.cpu().numpy(), ref_out.cpu().numpy())
        outs = []
        for p in (1, 3, 8):
            g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
            reg = exact.Registry()
            reg.ensure(0, g_in, scale)
            reg.ensure(1, g_out, scale)
            sgns_accumulate(w_in, w_out, g_in, g_out, K, phase=1, **kw)
            sgns_phase2_pieces(w_in, g_out, K, walks=walks, context_radius=R, n_pieces=p,
                               piece_rows=rows[p])
            torch.cuda.synchronize()
            reg.release()
            outs.append(g_out)
        _assert_g_close(outs[0].cpu().numpy(), ref_out.cpu().numpy())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    finally:
        set_walk_agg(-1)


def test_lazy_form_lags(hip_device):
    """OwnerLazyTables on one rank with the lazy out table through the gather path
    (dw_sgns_owner_pass2_lazy: this kernel with last != NULL): out rows stepped with lags 0, 1
    and 5 equal dense training at test_owner_lazy_single_rank_equals_dense's bar."""
    from shallow_encoders.word2vec.sharding import ShardedTables
    from test_gpu_owner import _lazy_vs_dense
    V, d, R, K, L, n, steps, lr = 5000, 128, 2, 3, 12, 16, 7, 0.01
    walks = torch.randint(10, V, (steps, n, L), generator=torch.Generator().manual_seed(3),
                          dtype=torch.int32)
    walks[:, :, 5] = 1            # every step, every walk: lag 0, a row across chunks
    walks[0::2, 0, 3] = 2         # every other step: lag 1
    walks[0, 1, 3] = 3            # steps 1 and 7: lag 5
    walks[6, 1, 3] = 3
    seen = [sorted(set((walks[s] == r).any().item() * (s + 1) for s in range(steps)) - {0})
            for r in (1, 2, 3)]
    assert seen == [[1, 2, 3, 4, 5, 6, 7], [1, 3, 5, 7], [1, 7]]
    ref = ShardedTables(V, d, hip_device, lr=lr, init_seed=4)
    per = L - 2 * R
    for s in range(steps):
        sgns_accumulate(ref.w_in, ref.w_out, ref.g_in, ref.g_out, K, walks=walks[s].cuda(),
                        context_radius=R, seed=11, noise_offset=s * n * per)
        ref.step()

    def cfg(t):
        t.rows_major = False
    t, _ = _lazy_vs_dense(hip_device, walks, V, d, R, K, lr, lazy_out=True, configure=cfg)
    assert not t._rows_step
    assert t.last_out[:4].tolist()[1:] == [steps, steps, steps]
    for got, exp in ((t.w_in.cpu().numpy(), ref.w_in.cpu().numpy()),
                     (t.full_w_out().cpu().numpy(), ref.w_out.cpu().numpy())):
        assert_params_close(got, exp, lr, rtol=1e-5, atol=1e-6, max_frac=1e-3,
                            max_abs=2.05 * lr * steps)
        assert_no_row_drift(got, exp)
