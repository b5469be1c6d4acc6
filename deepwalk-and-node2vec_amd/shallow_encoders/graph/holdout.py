"""Held-out edge split for link prediction (node2vec §4.4's protocol).

``split_edges(csr, ratio, seed)`` hides ``round(ratio * E)`` edges of a simple undirected
``CSRGraph`` and returns the residual (train) graph and the hidden edges. The rule is a pure
function of (graph, ratio, seed), so the training tool, the downstream tool and every rank of a
multi-GPU job get the same split without passing a file:

  * ``mix64`` is splitmix64's finaliser, a bijection on 64 bits; the priority of edge {u, v},
    u < v, is ``mix64(((u << 32) | v) ^ mix64(seed))`` — distinct edges never tie;
  * self-loops are never held out and protect nothing;
  * every node with a non-loop edge protects its non-loop edge of smallest priority; an edge is
    protected when either endpoint protects it; the other non-loop edges are the candidates;
  * ``n_want = round(ratio * E_nl)``, ``n_hold = min(n_want, n_candidates)``, and the held edges
    are the ``n_hold`` candidates of smallest priority;
  * the train CSR is the full CSR without both directed entries of every held edge, rows
    compacted in order (weights follow their entries; names, ``vocab_size`` and row 0 stay);
    ``held`` lists the held edges (u, v), u < v, in the row order of the full CSR.

Every node of degree >= 1 keeps degree >= 1, so the table's rows line up with the full graph and
the walker never meets an isolated node. That rule (``protect='degree'``, the default) gives
minimum degree 1, not connectivity. ``protect='connected'`` is the paper's: it removes edges
"while ensuring that the residual network is connected".

  * the protected edges are the minimum spanning forest of the non-loop edges under the same
    priorities (distinct, so the forest is unique); the candidates are the other non-loop edges,
    ``n_candidates = E_nl - n_forest``, and the rest of the rule is unchanged;
  * the residual graph then has exactly the full graph's connected components and no bridge is
    ever held; by the cut property every edge the degree rule protects is in the forest, so the
    connected rule's candidates are a subset of the degree rule's;
  * ``info`` gains ``n_forest`` and ``n_components`` (the components that hold a non-loop edge:
    ``n_forest`` = nodes with a non-loop edge - ``n_components``).

``connected_components(csr)`` labels every row by the smallest row of its component.

``device=None`` is vectorised numpy (the forest by Boruvka rounds); a HIP device runs
dw_edge_holdout_count + dw_edge_holdout, or dw_edge_forest + dw_edge_holdout_count_protected +
dw_edge_holdout_protected (csrc/dw_holdout.hip). Both give identical arrays.
"""
import ctypes
from typing import Dict, Tuple

import numpy as np
import torch

from shallow_encoders.graph.csr import CSRGraph

_M64 = (1 << 64) - 1
_LIMIT_31 = 1 << 31
_NO_PRIO = np.uint64(_M64)


def mix64(x: int) -> int:
    """splitmix64's finaliser on a Python int (mod 2^64)."""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hold_counts(ratio: float, n_edges: int, n_candidates: int) -> Tuple[int, int]:
    """(n_want, n_hold) of a graph with ``n_edges`` non-loop edges."""
    n_want = round(ratio * n_edges)
    return n_want, min(n_want, n_candidates)


def _check_args(csr: CSRGraph, ratio: float) -> None:
    if not 0.0 <= ratio < 1.0:
        raise ValueError(f'holdout ratio must be in [0, 1), got {ratio!r}')
    if csr.nnz >= _LIMIT_31:
        raise ValueError(f'{csr.nnz} directed entries: the edge split takes fewer than 2^31')
    if csr.vocab_size >= 1 and csr.row_ptr[min(1, csr.vocab_size)] != 0:
        raise ValueError('edge split: malformed CSR graph (row 0, <unk>, has neighbours)')


PROTECT = ('degree', 'connected')


def _entries(csr: CSRGraph):
    """(x, y) int64 per directed entry, checked: in range and no neighbour twice in a row."""
    V = csr.vocab_size
    row_ptr = np.asarray(csr.row_ptr, dtype=np.int64)
    x = np.repeat(np.arange(V, dtype=np.int64), np.diff(row_ptr))
    y = csr.host_col().astype(np.int64)
    if y.size and (int(y.min()) < 1 or int(y.max()) >= V):
        raise ValueError('edge split: malformed CSR graph (a neighbour on row 0 or out of range)')
    if np.unique(x * np.int64(V) + y).size != y.size:
        raise ValueError('edge split: a CSR row lists the same neighbour twice (the split needs '
                         'a simple graph)')
    return x, y


def _prio(x: np.ndarray, y: np.ndarray, seed: int) -> np.ndarray:
    u, v = np.minimum(x, y).astype(np.uint64), np.maximum(x, y).astype(np.uint64)
    return _mix64_np(((u << np.uint64(32)) | v) ^ np.uint64(mix64(seed)))


def _forest(V: int, x: np.ndarray, y: np.ndarray, prio: np.ndarray):
    """(forest bool per entry, labels int32[V], rounds): the minimum spanning forest of the
    non-loop entries by Boruvka rounds, the kernels' rule restated on whole arrays; both directed
    entries of an edge are present, so a component's minimum is taken over its own rows only."""
    comp = np.arange(V, dtype=np.int64)
    forest = np.zeros(x.size, dtype=bool)
    nonloop = x != y
    rounds = 0
    while True:
        cx, cy = comp[x], comp[y]
        live = nonloop & (cx != cy)
        if not live.any():
            break
        rounds += 1
        best = np.full(V, _NO_PRIO, dtype=np.uint64)
        np.minimum.at(best, cx[live], prio[live])
        mine, theirs = live & (prio == best[cx]), live & (prio == best[cy])
        forest |= mine | theirs
        parent = np.arange(V, dtype=np.int64)
        hook = mine & ~(theirs & (cx < cy))        # a mutual pick: the smaller label stays a root
        parent[cx[hook]] = cy[hook]
        while True:                                # pointer jumping to the roots
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        comp = parent[comp]
    smallest = np.full(V, V, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(V, dtype=np.int64))
    return forest, smallest[comp].astype(np.int32), rounds


def connected_components(csr: CSRGraph, device=None) -> Tuple[object, int]:
    """(labels int32[V], n_components): ``labels[v]`` is the smallest row of v's connected
    component (a row without a non-loop edge, row 0 included, is its own id); ``n_components``
    counts the components of the nodes, rows 1 .. V - 1, isolated ones included. ``labels`` is a
    numpy array, or a device tensor when ``device`` is a HIP device (dw_edge_forest)."""
    _check_args(csr, 0.0)
    V = csr.vocab_size
    if device is not None and torch.device(device).type == 'cuda':
        from shallow_encoders import _native
        dev = _native.require_device(device)
        csr.require_simple(dev)
        labels = _forest_device(csr, 0, dev)[1]
        own = labels[1:] == torch.arange(1, V, dtype=torch.int32, device=dev)
        return labels, int(own.sum())
    x, y = _entries(csr)
    labels = _forest(V, x, y, _prio(x, y, 0))[1]
    return labels, int((labels[1:] == np.arange(1, V)).sum())


def split_edges(csr: CSRGraph, ratio: float, seed: int, device=None,
                protect: str = 'degree') -> Tuple[CSRGraph, object, Dict[str, int]]:
    """(train_csr, held, info): ``held`` int64 [n_hold, 2] (a numpy array, or a device tensor
    when ``device`` is a HIP device), ``info`` = {'n_edges', 'n_want', 'n_candidates',
    'n_hold'}, and 'n_forest' and 'n_components' with ``protect='connected'``. Raises ValueError
    for a ratio outside [0, 1), an unknown ``protect``, a repeated neighbour in a row or a
    neighbour on row 0."""
    ratio, seed = float(ratio), int(seed) & _M64
    if protect not in PROTECT:
        raise ValueError(f"protect must be 'degree' or 'connected', got {protect!r}")
    _check_args(csr, ratio)
    if device is not None and torch.device(device).type == 'cuda':
        return _split_device(csr, ratio, seed, device, protect)
    V = csr.vocab_size
    row_ptr = np.asarray(csr.row_ptr, dtype=np.int64)
    col = csr.host_col()
    weights = csr.weights
    x, y = _entries(csr)
    nonloop = x != y
    prio = _prio(x, y, seed)
    upper = nonloop & (y > x)                                  # each edge once
    extra = {}
    if protect == 'connected':
        forest, labels, _ = _forest(V, x, y, prio)
        free = nonloop & ~forest
        heads = np.zeros(V, dtype=bool)                        # a component's smallest row ...
        heads[labels[x[nonloop]]] = True                       # ... that has a non-loop edge
        extra = {'n_forest': int((upper & forest).sum()), 'n_components': int(heads.sum())}
    else:
        # the per-node minimum: rows are contiguous runs of entries
        minp = np.full(V, _NO_PRIO, dtype=np.uint64)
        starts = row_ptr[:-1][np.diff(row_ptr) > 0]
        if starts.size:
            minp[x[starts]] = np.minimum.reduceat(np.where(nonloop, prio, _NO_PRIO), starts)
        free = nonloop & (prio != minp[x]) & (prio != minp[y])     # not protected
    n_edges, n_cand = int(upper.sum()), int((upper & free).sum())
    n_want, n_hold = hold_counts(ratio, n_edges, n_cand)
    held_entry = np.zeros(y.size, dtype=bool)
    if n_hold:
        threshold = np.partition(prio[upper & free], n_hold - 1)[n_hold - 1]
        held_entry = free & (prio <= threshold)
    pick = held_entry & upper
    held = np.stack([x[pick], y[pick]], axis=1).astype(np.int64).reshape(-1, 2)
    keep = ~held_entry
    new_ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(x[keep], minlength=V), out=new_ptr[1:])
    train = CSRGraph.from_arrays(new_ptr, col[keep], None if weights is None else weights[keep],
                                 itos=csr.itos, names=csr.names)
    return train, held, {'n_edges': n_edges, 'n_want': n_want, 'n_candidates': n_cand,
                         'n_hold': n_hold, **extra}


def _forest_device(csr: CSRGraph, seed: int, dev):
    """(forest uint8[nnz], labels int32[V], counts int64[4]) of dw_edge_forest, all on ``dev``
    (synchronises on the status word)."""
    from shallow_encoders import _native
    d = csr.device_tensors(dev)
    V, nnz = csr.vocab_size, csr.nnz
    with torch.cuda.device(dev):
        nb = ctypes.c_size_t(0)
        _native.call('dw_edge_forest_workspace_bytes', V, nnz, ctypes.byref(nb))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        forest = torch.empty(max(nnz, 1), dtype=torch.uint8, device=dev)
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.call('dw_edge_forest', _native.ptr(d['row_ptr']),
                     _native.ptr(d['col']) if nnz else None, V, nnz, seed, _native.ptr(forest),
                     _native.ptr(labels), _native.ptr(counts), _native.ptr(status),
                     _native.ptr(ws), ws.numel(), _native.stream(dev))
        _native.check_status(status, 'spanning forest')
        del ws
    return forest, labels, counts


def _split_device(csr: CSRGraph, ratio: float, seed: int, device, protect: str):
    from shallow_encoders import _native
    dev = _native.require_device(device)
    csr.require_simple(dev)                     # DW_S_DUP_NEIGHBOR -> ValueError
    d = csr.device_tensors(dev)
    V, nnz = csr.vocab_size, csr.nnz
    weights = d['weights']
    extra, flags, suffix = {}, (), ''
    if protect == 'connected':
        forest, _, fcounts = _forest_device(csr, seed, dev)
        _, n_forest, n_comp, _ = (int(c) for c in fcounts.tolist())
        extra = {'n_forest': n_forest, 'n_components': n_comp}
        flags, suffix = (_native.ptr(forest),), '_protected'
    with torch.cuda.device(dev):
        s = _native.stream(dev)
        nb = ctypes.c_size_t(0)
        _native.call('dw_edge_holdout_workspace_bytes', V, nnz, ctypes.byref(nb))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        colp = _native.ptr(d['col']) if nnz else None
        _native.call('dw_edge_holdout_count' + suffix, _native.ptr(d['row_ptr']), colp, V, nnz,
                     seed, *flags, _native.ptr(counts), _native.ptr(status), _native.ptr(ws),
                     ws.numel(), s)
        n_edges, n_cand = (int(c) for c in counts.tolist())   # synchronises: the output sizes
        _native.check_status(status, 'edge split')
        n_want, n_hold = hold_counts(ratio, n_edges, n_cand)
        nnz_out = nnz - 2 * n_hold
        new_ptr = torch.empty(V + 1, dtype=torch.int64, device=dev)
        new_col = torch.empty(max(nnz_out, 1), dtype=torch.int32, device=dev)
        new_w = None if weights is None else torch.empty(max(nnz_out, 1), dtype=torch.float64,
                                                         device=dev)
        held = torch.empty((n_hold, 2), dtype=torch.int64, device=dev)
        _native.call('dw_edge_holdout' + suffix, _native.ptr(d['row_ptr']), colp,
                     _native.ptr(weights), V, nnz, seed, *flags, n_cand, n_hold,
                     _native.ptr(new_ptr), _native.ptr(new_col),
                     _native.ptr(new_w), _native.ptr(held) if n_hold else None,
                     _native.ptr(status), _native.ptr(ws), ws.numel(), s)
        _native.check_status(status, 'edge split')
        del ws
    train = CSRGraph.from_device(new_ptr, new_col[:nnz_out], csr.itos,
                                 None if new_w is None else new_w[:nnz_out])
    train.names = csr.names
    return train, held, {'n_edges': n_edges, 'n_want': n_want, 'n_candidates': n_cand,
                         'n_hold': n_hold, **extra}
