"""Python restatement of the unigram noise sampler (TEST INFRASTRUCTURE).

``alias_table`` restates dw_noise_alias_build (dw_host.cpp) with Python floats — IEEE doubles,
the same operations in the same order — so the native build can be checked bit for bit;
``alias_noise`` restates dw_sgns_noise_alias (dw_noise.hip) on top of oracle/philox.py;
``table_mass`` rebuilds the law a table samples.
"""
import math

import numpy as np

from oracle import philox as ph

ALWAYS = 0xFFFFFFFF


def alias_table(weights) -> np.ndarray:
    """uint64 [V]: entry = alias id << 32 | prob_thr (Vose, float64; the small list a stack
    growing from the front, the large list one growing from the back, both popped from the top)."""
    w = [float(x) for x in np.asarray(weights, dtype=np.float64)]
    V = len(w)
    if V < 1:
        raise ValueError('empty weight vector')
    total = 0.0
    heaviest = 0
    for i, x in enumerate(w):
        if not (0.0 <= x <= 1.7976931348623157e308):
            raise ValueError(f'weight {i} is negative or not finite')
        total += x
        if x > w[heaviest]:
            heaviest = i
    if not (0.0 < total <= 1.7976931348623157e308):
        raise ValueError('the weights must have a positive, finite sum')
    scaled = [x * float(V) / total for x in w]
    small, large = [], []
    for i in range(V):
        (small if scaled[i] < 1.0 else large).append(i)
    table = [0] * V
    while small and large:
        l_ = small.pop()
        g = large.pop()
        pl = scaled[l_]
        table[l_] = (g << 32) | int(min(math.floor(pl * 4294967296.0), 4294967295.0))
        pg = (scaled[g] + pl) - 1.0
        scaled[g] = pg
        (small if pg < 1.0 else large).append(g)
    for g in large:
        table[g] = (g << 32) | ALWAYS
    for l_ in small:
        table[l_] = (heaviest << 32) if w[l_] == 0.0 else ((l_ << 32) | ALWAYS)
    return np.array(table, dtype=np.uint64)


def table_mass(table) -> np.ndarray:
    """float64 [V]: the probability of each id under the sampler's rule (slot uniform over V,
    kept with probability prob_thr / 2^32, or 1 for 0xFFFFFFFF; else the alias)."""
    t = np.asarray(table, dtype=np.uint64)
    V = len(t)
    thr = (t & np.uint64(ALWAYS)).astype(np.int64)
    alias = (t >> np.uint64(32)).astype(np.int64)
    keep = np.where(thr == ALWAYS, 1.0, thr.astype(np.float64) / 4294967296.0)
    mass = keep / V
    np.add.at(mass, alias, (1.0 - keep) / V)
    return mass


def alias_noise(table, seed: int, noise_offset: int, n_centres: int, n_ctx: int,
                k: int) -> np.ndarray:
    """int64 [B', C, K]: what dw_sgns_noise_alias writes. Centre b's slot n = j*K + k takes
    Philox call n // 2, counter (g lo, g hi, n // 2, TAG_SGNS) with g = noise_offset + b, words
    (x, y) for even n and (z, w) for odd n; T = hi*V + ((lo*V) >> 32), slot i = T >> 32, fraction
    f = T & 0xFFFFFFFF, id = i if prob_thr(i) is 0xFFFFFFFF or f < prob_thr(i) else alias(i)."""
    t = np.asarray(table, dtype=np.uint64)
    V = len(t)
    if not 0 < V < 2 ** 31:
        raise ValueError('vocab_size must be in [1, 2^31)')
    m32, s32 = np.uint64(ph.MASK), np.uint64(32)
    k0, k1 = seed & ph.MASK, (seed >> 32) & ph.MASK
    g = (np.arange(n_centres, dtype=np.uint64) + np.uint64(noise_offset % 2 ** 64))
    gg = np.repeat(g, n_ctx * k)
    nn = np.tile(np.arange(n_ctx * k, dtype=np.uint64), n_centres)
    r = ph.philox(gg & m32, gg >> s32, nn >> np.uint64(1),
                  np.full(gg.shape, ph.TAG_SGNS, np.uint64), k0, k1)
    odd = (nn & np.uint64(1)).astype(bool)
    lo = np.where(odd, r[2], r[0])
    hi = np.where(odd, r[3], r[1])
    T = hi * np.uint64(V) + ((lo * np.uint64(V)) >> s32)   # < 2^64 for V < 2^32: never wraps
    i = (T >> s32).astype(np.int64)
    f = T & m32
    e = t[i]
    thr = e & m32
    keep = (thr == np.uint64(ALWAYS)) | (f < thr)
    ids = np.where(keep, i, (e >> s32).astype(np.int64))
    return ids.reshape(n_centres, n_ctx, k)
