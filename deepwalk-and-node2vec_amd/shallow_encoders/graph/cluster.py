"""Community detection from the embeddings: k-means and the partition scores (node2vec §4.1
clusters the Les Misérables embeddings with k-means; a departure: the reference has no clustering
task).

  * ``kmeans``: Lloyd's algorithm over the rows ``table[ids]``. ``device=None`` is numpy on the
    host; a HIP device keeps the fp32 table in HBM, every pass one dw_kmeans_step (both products on
    the float64 MFMA, no float64 copy of the features), the seeding dw_kmeans_seed;
  * ``contingency``, ``nmi`` (arithmetic normalisation, sklearn's default), ``ari``: two
    partitions compared; ``modularity``: a partition of a CSR graph's rows scored structurally
    (weights ignored), counted as networkx does. The integer tables come from
    dw_partition_counts / dw_modularity_counts for device tensors, from numpy otherwise; the few
    float64 operations on the small tables run on the host.

Departures from sklearn.cluster.KMeans: the stop rule is exact (no label changed; no tolerance),
an empty cluster keeps its centroid (no relocation), and k-means++ is the plain D² law (one draw
per centre), not sklearn's greedy variant. Labels are -1 for a sample that takes no part.
"""
import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from shallow_encoders import _native

MAX_CLUSTERS = 1024
MAX_DIM = 512
TAG_KMEANS = 0x4B4D0000
_M32 = 0xFFFFFFFF


# ---- the seeding law's uniforms ----------------------------------------------------------------
def _philox(c0: int, c1: int, c2: int, c3: int, k0: int, k1: int):
    """Philox4x32-10 on Python integers (csrc/dw_common.h::philox)."""
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, \
            ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def seed_uniform(seed: int, j: int) -> float:
    """U_j in [0, 1) of dw_kmeans_seed: counter (j, 0, 0, 'KM'), key (seed lo, seed hi)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = _philox(int(j) & _M32, 0, 0, TAG_KMEANS, seed & _M32, seed >> 32)
    return float(((r[0] >> 5) << 26) | (r[1] >> 6)) * 2.0 ** -53


def _is_device(device) -> bool:
    return device is not None and torch.device(device).type == 'cuda'


def _host_rows(table, ids) -> np.ndarray:
    """table[ids] widened to float64 (the host path's copy); IndexError for an id out of range."""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim != 2 or t.dtype != np.float32:
        raise ValueError('table must be a float32 [V, d] array')
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64)
    if ids.ndim != 1:
        raise ValueError('ids must be an int64 [n] array')
    if ids.size and (ids.min() < 0 or ids.max() >= t.shape[0]):
        raise IndexError('kmeans: index out of range [0, vocab_size)')
    return t[ids].astype(np.float64)


# ---- one Lloyd pass ----------------------------------------------------------------------------
def kmeans_step_host(X: np.ndarray, centroids: np.ndarray,
                     prev: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """dw_kmeans_step in numpy over the float64 rows X: (labels int64 [n], out float64
    [K (d + 1) + 2]: per cluster the members' sum and count, then the inertia, then the number of
    labels that differ from ``prev`` (n without one))."""
    C = np.asarray(centroids, dtype=np.float64)
    n, d = X.shape
    K = C.shape[0]
    scores = np.einsum('kj,kj->k', C, C)[None, :] - 2.0 * (X @ C.T)
    labels = np.argmin(scores, axis=1).astype(np.int64)   # the first minimum: the lowest k
    out = np.zeros(K * (d + 1) + 2)
    acc = out[:K * (d + 1)].reshape(K, d + 1)
    order = np.argsort(labels, kind='stable')
    counts = np.bincount(labels, minlength=K)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    filled = counts > 0
    if n:
        acc[filled, :d] = np.add.reduceat(X[order], starts[filled], axis=0)
    acc[:, d] = counts
    out[-2] = float(np.sum(np.einsum('ij,ij->i', X, X) + scores[np.arange(n), labels]))
    out[-1] = float(n if prev is None else np.count_nonzero(np.asarray(prev) != labels))
    return labels, out


def step_workspace(n: int, d: int, n_clusters: int, device) -> torch.Tensor:
    """A dw_kmeans_step workspace for n samples of dimension d and n_clusters clusters."""
    nb = ctypes.c_size_t(0)
    _native.call('dw_kmeans_step_workspace_bytes', int(n), int(d), int(n_clusters),
                 ctypes.byref(nb))
    return torch.empty(max(int(nb.value), 256), dtype=torch.uint8, device=device)


def _check_device_shapes(table: torch.Tensor, ids: torch.Tensor, n_clusters: int) -> None:
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('table must be a float32 [V, d] device tensor')
    if not 1 <= table.shape[1] <= MAX_DIM:
        raise ValueError(f'embedding size {table.shape[1]} outside [1, {MAX_DIM}]')
    if not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f'n_clusters {n_clusters} outside [1, {MAX_CLUSTERS}]')
    if ids.dtype != torch.int64 or ids.dim() != 1:
        raise ValueError('ids must be an int64 [n] device tensor')
    if ids.device != table.device:
        raise ValueError('ids and table live on different devices')


def kmeans_step(table: torch.Tensor, ids: torch.Tensor, centroids: torch.Tensor,
                prev: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None,
                check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """One dw_kmeans_step pass at ``centroids`` (float64 [K, d] on the device): (labels int32 [n],
    out float64 [K (d + 1) + 2]), both device tensors. ``prev``: the previous labels (int32 [n])
    or None; ``labels``: an optional destination."""
    K = centroids.shape[0] if centroids.dim() == 2 else 0
    _check_device_shapes(table, ids, K)
    dev = table.device
    n, d = ids.shape[0], table.shape[1]
    if centroids.dtype != torch.float64 or centroids.shape != (K, d) or centroids.device != dev:
        raise ValueError('centroids must be a float64 [n_clusters, d] tensor on the table\'s '
                         'device')
    for name, t in (('prev', prev), ('labels', labels)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (n,) or t.device != dev):
            raise ValueError(f'{name} must be an int32 [n] tensor on the table\'s device')
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.zeros(K * (d + 1) + 2, dtype=torch.float64, device=dev)
    if n == 0:
        return labels, out
    if workspace is None:
        workspace = step_workspace(n, d, K, dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_kmeans_step', _native.ptr(table.contiguous()), table.shape[0], d,
                     _native.ptr(ids.contiguous()), n, _native.ptr(centroids.contiguous()), K,
                     _native.ptr(prev), _native.ptr(labels), _native.ptr(out),
                     _native.ptr(workspace), workspace.numel() * workspace.element_size(),
                     _native.ptr(st), _native.stream(dev))
    if check:
        _native.check_status(st, 'kmeans_step')
    return labels, out


# ---- seeding -----------------------------------------------------------------------------------
def kmeans_seed_host(X: np.ndarray, n_clusters: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """dw_kmeans_seed's law in numpy over the float64 rows X: (chosen int64 [K], centroids)."""
    n, K = X.shape[0], int(n_clusters)
    if n < K:
        raise ValueError(f'kmeans: {K} centres from {n} samples')
    chosen = np.empty(K, dtype=np.int64)
    chosen[0] = min(int(seed_uniform(seed, 0) * n), n - 1)
    d2 = None
    for j in range(1, K):
        diff = X - X[chosen[j - 1]]
        dist = np.einsum('ij,ij->i', diff, diff)
        d2 = dist if d2 is None else np.minimum(d2, dist)
        total = float(d2.sum())
        if total > 0.0:
            run = np.cumsum(d2)
            hit = np.flatnonzero((run > seed_uniform(seed, j) * total) & (d2 > 0.0))
            chosen[j] = hit[0] if hit.size else np.flatnonzero(d2 > 0.0)[-1]
        else:   # fewer distinct rows than centres: the lowest index not chosen yet
            taken = set(chosen[:j].tolist())
            chosen[j] = next(i for i in range(j + 1) if i not in taken)
    return chosen, X[chosen].copy()


def kmeans_seed(table: torch.Tensor, ids: torch.Tensor, n_clusters: int, seed: int,
                check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """dw_kmeans_seed: (chosen int64 [K] sample indices, centroids float64 [K, d]), device
    tensors."""
    _check_device_shapes(table, ids, n_clusters)
    dev = table.device
    n, d, K = ids.shape[0], table.shape[1], int(n_clusters)
    if n < K:
        raise ValueError(f'kmeans: {K} centres from {n} samples')
    chosen = torch.zeros(K, dtype=torch.int64, device=dev)
    cent = torch.zeros((K, d), dtype=torch.float64, device=dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_kmeans_seed_workspace_bytes', n, ctypes.byref(nb))
    ws = torch.empty(max(int(nb.value), 256), dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_kmeans_seed', _native.ptr(table.contiguous()), table.shape[0], d,
                     _native.ptr(ids.contiguous()), n, K, int(seed) & 0xFFFFFFFFFFFFFFFF,
                     _native.ptr(chosen), _native.ptr(cent), _native.ptr(ws), ws.numel(),
                     _native.ptr(st), _native.stream(dev))
    if check:
        _native.check_status(st, 'kmeans_seed')
    return chosen, cent


# ---- Lloyd's algorithm -------------------------------------------------------------------------
class _HostBackend:
    def __init__(self, table, ids):
        self.X = _host_rows(table, ids)
        self.n, self.d = self.X.shape

    def seed(self, K, seed):
        return kmeans_seed_host(self.X, K, seed)[1]

    def rows(self, idx):
        return self.X[idx].copy()

    def step(self, C, prev):
        return kmeans_step_host(self.X, C, prev)

    def labels_out(self, labels):
        return labels


class _DeviceBackend:
    def __init__(self, table, ids, K, device):
        self.dev = _native.require_device(device)
        self.table = table.to(self.dev) if isinstance(table, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(table)).to(self.dev)
        self.ids = torch.as_tensor(ids, dtype=torch.int64).to(self.dev)
        _check_device_shapes(self.table, self.ids, K)
        self.n, self.d = self.ids.shape[0], self.table.shape[1]
        self.ws = step_workspace(self.n, self.d, K, self.dev)
        self.bufs = [torch.empty(self.n, dtype=torch.int32, device=self.dev) for _ in range(2)]

    def seed(self, K, seed):
        return kmeans_seed(self.table, self.ids, K, seed)[1].cpu().numpy()

    def rows(self, idx):
        sel = self.ids[torch.as_tensor(idx, dtype=torch.int64, device=self.dev)]
        if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= self.table.shape[0]):
            raise IndexError('kmeans: index out of range [0, vocab_size)')
        return self.table[sel].double().cpu().numpy()

    def step(self, C, prev):
        dst = self.bufs[1] if prev is self.bufs[0] else self.bufs[0]
        labels, out = kmeans_step(self.table, self.ids, torch.from_numpy(C).to(self.dev), prev,
                                  dst, self.ws)
        return labels, out.cpu().numpy()   # (synchronises: the loop reads the changed count)

    def labels_out(self, labels):
        return labels.to(torch.int64)


def _lloyd(be, C: np.ndarray, max_iter: int):
    """From the centroids C: (labels, centroids, inertia, n_iter). A pass assigns and sums; no
    label changed: the centroids are the labels' means already, stop. Else the new centroid is
    sum / count (an empty cluster keeps its own). After max_iter updates a last pass makes labels
    and inertia those of the returned centroids."""
    K, d = C.shape
    prev, n_iter = None, 0
    for n_iter in range(1, max_iter + 1):
        labels, out = be.step(C, prev)
        if out[-1] == 0.0:
            return labels, C, float(out[-2]), n_iter
        acc = out[:K * (d + 1)].reshape(K, d + 1)
        filled = acc[:, d] > 0
        C = C.copy()
        C[filled] = acc[filled, :d] / acc[filled, d:d + 1]
        prev = labels
    labels, out = be.step(C, prev)
    return labels, C, float(out[-2]), n_iter


def kmeans(table, ids, n_clusters: int, init='k-means++', n_init: int = 1, max_iter: int = 100,
           seed: int = 0, device=None):
    """k-means of the rows ``table[ids]`` (float32 [V, d]; ids int64 [n]) into ``n_clusters``
    clusters: (labels int64 [n], centroids float64 [K, d], inertia, n_iter) of the best of
    ``n_init`` restarts (lowest inertia, ties to the earliest; restart r seeds with seed + r).

    init: 'k-means++' (dw_kmeans_seed's law), 'random' (K distinct samples, numpy's generator) or
    a float64 [K, d] array (one run). ``device=None`` runs in numpy and returns numpy labels; a
    HIP device runs the passes there and returns the labels as a device tensor. The loop stops
    when no label changed (exactly) or after ``max_iter`` centroid updates."""
    K = int(n_clusters)
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f'n_clusters {n_clusters} outside [1, {MAX_CLUSTERS}]')
    if int(max_iter) < 1 or int(n_init) < 1:
        raise ValueError('max_iter and n_init must be >= 1')
    explicit = not isinstance(init, str)
    if not explicit and init not in ('k-means++', 'random'):
        raise ValueError(f"init must be 'k-means++', 'random' or an array, got {init!r}")
    be = _DeviceBackend(table, ids, K, device) if _is_device(device) else _HostBackend(table, ids)
    if be.n < K:
        raise ValueError(f'kmeans: {K} clusters from {be.n} samples')
    best = None
    for r in range(1 if explicit else int(n_init)):
        if explicit:
            C = np.array(init, dtype=np.float64)
            if C.shape != (K, be.d):
                raise ValueError(f'init must have shape ({K}, {be.d}), got {C.shape}')
        elif init == 'k-means++':
            C = be.seed(K, int(seed) + r)
        else:
            rng = np.random.default_rng(int(seed) + r)
            C = be.rows(np.sort(rng.choice(be.n, size=K, replace=False)))
        run = _lloyd(be, np.ascontiguousarray(C), int(max_iter))
        if best is None or run[2] < best[2]:
            best = (be.labels_out(run[0]),) + run[1:]   # (a copy: the passes reuse their buffers)
    return best


# ---- partition scores --------------------------------------------------------------------------
def _n_classes(x) -> int:
    if isinstance(x, torch.Tensor):
        return int(x.max()) + 1 if x.numel() else 0
    return int(np.max(x)) + 1 if np.size(x) else 0


def contingency(a, b, n_a: Optional[int] = None, n_b: Optional[int] = None) -> np.ndarray:
    """int64 [Ka, Kb]: cell [i, j] counts the samples with a = i and b = j; a label of -1 in
    either skips the sample. Ka, Kb default to the largest label + 1. Device tensors go through
    dw_partition_counts, anything else through numpy."""
    if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
        raise ValueError('contingency: two device tensors or two arrays')
    if len(a) != len(b):
        raise ValueError('contingency: the partitions differ in length')
    Ka = max(int(n_a) if n_a is not None else _n_classes(a), 1)
    Kb = max(int(n_b) if n_b is not None else _n_classes(b), 1)
    if isinstance(a, torch.Tensor) and a.device.type == 'cuda':
        dev = a.device
        a32, b32 = a.to(torch.int32).contiguous(), b.to(dev, torch.int32).contiguous()
        table = torch.zeros((Ka, Kb), dtype=torch.int64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native.call('dw_partition_counts', _native.ptr(a32), Ka, _native.ptr(b32), Kb,
                         a32.numel(), _native.ptr(table), _native.ptr(st), _native.stream(dev))
        _native.check_status(st, 'partition counts')
        return table.cpu().numpy()
    a = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.int64)
    b = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, dtype=np.int64)
    if a.size and (a.min() < -1 or a.max() >= Ka or b.min() < -1 or b.max() >= Kb):
        raise IndexError('contingency: a label is out of range')
    keep = (a >= 0) & (b >= 0)
    return np.bincount(a[keep] * Kb + b[keep], minlength=Ka * Kb).reshape(Ka, Kb)


def _entropy(counts: np.ndarray) -> float:
    c = counts[counts > 0].astype(np.float64)
    if c.size == 0:
        return 1.0
    total = c.sum()
    return float(-np.sum((c / total) * (np.log(c) - np.log(total))))


def nmi_from_table(table: np.ndarray) -> float:
    """Normalised mutual information (arithmetic mean of the entropies, sklearn's default) of a
    contingency table; empty classes take no part."""
    t = np.asarray(table, dtype=np.int64)
    ra, rb = t.sum(axis=1), t.sum(axis=0)
    if np.count_nonzero(ra) <= 1 and np.count_nonzero(rb) <= 1:
        return 1.0   # one cluster against one cluster (or no samples): sklearn's convention
    n = float(t.sum())
    i, j = np.nonzero(t)
    if len(i) == np.count_nonzero(ra) == np.count_nonzero(rb):
        return 1.0   # the same partition under other names, exactly
    nij = t[i, j].astype(np.float64)
    mi = float(np.sum(nij / n * (np.log(nij) + np.log(n) - np.log(ra[i].astype(np.float64))
                                 - np.log(rb[j].astype(np.float64)))))
    mi = max(mi, 0.0)
    norm = 0.5 * (_entropy(ra) + _entropy(rb))
    # I(a; b) <= min(H(a), H(b)) <= the mean: rounding alone can pass 1
    return min(mi / max(norm, np.finfo(np.float64).eps), 1.0)


def ari_from_table(table: np.ndarray) -> float:
    """Adjusted Rand index of a contingency table, its pair counts in exact integers."""
    t = np.asarray(table, dtype=np.int64)
    n = int(t.sum())
    ra, rb = [int(x) for x in t.sum(axis=1)], [int(x) for x in t.sum(axis=0)]
    sq = sum(int(x) * int(x) for x in t.ravel())
    tp = sq - n
    fp = sum(int(t[i, j]) * rb[j] for i, j in zip(*np.nonzero(t))) - sq
    fn = sum(int(t[i, j]) * ra[i] for i, j in zip(*np.nonzero(t))) - sq
    tn = n * n - fp - fn - sq
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def nmi(a, b) -> float:
    return nmi_from_table(contingency(a, b))


def ari(a, b) -> float:
    return ari_from_table(contingency(a, b))


def modularity_counts(csr, labels, n_clusters: Optional[int] = None) -> np.ndarray:
    """int64 [K, 2] per cluster: the CSR entries with both ends in it and its summed degree, a
    self-loop entry (stored once) counting twice in both. ``labels`` covers the CSR's rows
    (-1: in no cluster). A device tensor goes through dw_modularity_counts."""
    V = csr.vocab_size
    if len(labels) != V:
        raise ValueError(f'modularity: {len(labels)} labels for {V} CSR rows')
    K = max(int(n_clusters) if n_clusters is not None else _n_classes(labels), 1)
    if isinstance(labels, torch.Tensor) and labels.device.type == 'cuda':
        dev = labels.device
        d = csr.device_tensors(dev)
        lab = labels.to(torch.int32).contiguous()
        out = torch.zeros((K, 2), dtype=torch.int64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native.call('dw_modularity_counts', _native.ptr(d['row_ptr']),
                         _native.ptr(d['col']) if csr.nnz else None, V, csr.nnz,
                         _native.ptr(lab), K, _native.ptr(out), _native.ptr(st),
                         _native.stream(dev))
        _native.check_status(st, 'modularity counts')
        return out.cpu().numpy()
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels, dtype=np.int64)
    if lab.size and (lab.min() < -1 or lab.max() >= K):
        raise IndexError('modularity: a label is out of range')
    u = np.repeat(np.arange(V, dtype=np.int64), np.diff(csr.row_ptr))
    v = csr.host_col().astype(np.int64)
    w = np.where(u == v, 2, 1).astype(np.int64)
    lu = lab[u]
    out = np.zeros((K, 2), dtype=np.int64)
    on = lu >= 0
    out[:, 1] = np.bincount(lu[on], weights=w[on], minlength=K).astype(np.int64)
    same = on & (lab[v] == lu)
    out[:, 0] = np.bincount(lu[same], weights=w[same], minlength=K).astype(np.int64)
    return out


def modularity(csr, labels, n_clusters: Optional[int] = None) -> float:
    """Structural modularity Q = sum_c in_c / 2m - (deg_c / 2m)^2 of ``labels`` over the
    undirected graph the symmetric CSR stores (networkx.community.modularity with weight=None);
    weights are ignored. 0 for a graph without edges."""
    counts = modularity_counts(csr, labels, n_clusters)
    two_m = int(counts[:, 1].sum())
    if two_m == 0:
        return 0.0
    return float(sum(int(i) / two_m - (int(g) / two_m) ** 2 for i, g in counts))
