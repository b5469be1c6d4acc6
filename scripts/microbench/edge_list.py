"""Cost of edge-list ingestion (shallow_encoders/graph/edge_list.py, csrc/dw_edgelist.hip) on
R-MAT 20's edge list (host rmat_edges: 2^20 nodes, 10M draws) written as text, one "u v" line
per edge, into a temporary directory.

  device   read + copy (file -> pinned staging -> HBM, host clock around a synchronise), then
           with the whole text resident in HBM: dw_edgelist_parse, dw_edges_canonical and
           dw_csr_from_edges_loops each between device events (warm-up, best of REPS), the parse
           against dw_stream_copy over the same bytes; and read_edge_list(device=...) end to end;
  host     the same file through the numpy / Python host path (parse and build, wall clock);
  weighted the same edges with a third column repr(uniform + 0.5), the whole text resident in HBM:
           dw_edgelist_parse_weighted against dw_edgelist_parse (the id-only parser) over the
           same lines without the column, in the same call; the undecided tokens; and
           read_edge_list(device=..., weighted=True) end to end (host patch included);
  parent   at R-MAT 16 only, the route a user had before: pandas.read_csv ->
           nx.from_pandas_edgelist -> CSRGraph.from_networkx, beside both new paths on that file.

    python scripts/microbench/edge_list.py [--part device|host|weighted|parent|all] [--json PATH]

One JSON line per part on stdout (and appended to --json).
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph import edge_list as el  # noqa: E402
from shallow_encoders.graph.rmat import rmat_edges  # noqa: E402

REPS = 5


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def write_text(edges: np.ndarray, path: str) -> int:
    import pandas as pd
    pd.DataFrame(edges).to_csv(path, sep=' ', header=False, index=False)
    return os.path.getsize(path)


def best_event_ms(fn, dev, reps=REPS):
    fn()
    torch.cuda.synchronize(dev)
    best = float('inf')
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        best = min(best, a.elapsed_time(b))
    return best


def best_wall_ms(fn, dev=None, reps=3):
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if dev is not None:
            torch.cuda.synchronize(dev)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def part_device(path, n_bytes, m_raw, dev, out):
    s = _native.stream(dev)
    # read + copy: the chunk loop of read_edge_arrays without the parse
    size = min(el.DEFAULT_CHUNK_BYTES, n_bytes + 1)
    stage_t = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    text = torch.empty(size, dtype=torch.uint8, device=dev)

    def read_copy():
        for n in el._text_chunks(path, stage_t.numpy()):
            text[:n].copy_(stage_t[:n], non_blocking=True)
            torch.cuda.synchronize(dev)
    read_copy_ms = best_wall_ms(read_copy, dev)
    assert n_bytes < size, 'the microbenchmark keeps the whole text in one chunk'
    # parse, text resident
    nb = ctypes.c_size_t(0)
    _native.call('dw_edgelist_workspace_bytes', n_bytes, m_raw, ctypes.byref(nb))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    cap = (n_bytes + 1) // 4 + 1
    src = torch.empty(cap, dtype=torch.int64, device=dev)
    dst = torch.empty(cap, dtype=torch.int64, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    parse_ms = best_event_ms(lambda: _native.call(
        'dw_edgelist_parse', _native.ptr(text), n_bytes, 0, _native.ptr(src), _native.ptr(dst),
        cap, _native.ptr(info), _native.ptr(info[2:]), _native.ptr(status), _native.ptr(ws),
        ws.numel(), s), dev)
    m = int(info[0])
    assert m == m_raw and int(status.item()) == 0
    nb16 = n_bytes - n_bytes % 16
    cdst = torch.empty(nb16, dtype=torch.uint8, device=dev)
    copy_ms = best_event_ms(lambda: _native.call('dw_stream_copy', _native.ptr(text),
                                                 _native.ptr(cdst), nb16, s), dev)
    del cdst
    # canonical form
    src, dst = src[:m].clone(), dst[:m].clone()
    id_bits = max(1, int(torch.maximum(src.max(), dst.max())).bit_length())
    node_ids = torch.empty(2 * m, dtype=torch.int64, device=dev)
    edges = torch.empty(m, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    canon_ms = best_event_ms(lambda: _native.call(
        'dw_edges_canonical', _native.ptr(src), _native.ptr(dst), None, m, id_bits,
        _native.ptr(node_ids), _native.ptr(edges), None, _native.ptr(counts),
        _native.ptr(status), _native.ptr(ws), ws.numel(), s), dev)
    n, E = counts.tolist()
    row_ptr = torch.empty(n + 2, dtype=torch.int64, device=dev)
    col = torch.empty(2 * E, dtype=torch.int32, device=dev)
    csr_ms = best_event_ms(lambda: _native.call(
        'dw_csr_from_edges_loops', _native.ptr(edges), None, E, n, _native.ptr(row_ptr),
        _native.ptr(col), None, _native.ptr(status), _native.ptr(ws), ws.numel(), s), dev)
    assert int(status.item()) == 0
    del ws, src, dst, node_ids, edges, row_ptr, col, text
    total_ms = best_wall_ms(lambda: el.read_edge_list(path, device=dev), dev)
    emit({'part': 'device', 'file_bytes': n_bytes, 'lines': m_raw, 'nodes': n, 'edges': E,
          'read_copy_ms': read_copy_ms, 'parse_ms': parse_ms,
          'parse_gbps': n_bytes / parse_ms / 1e6, 'stream_copy_ms': copy_ms,
          'stream_copy_gbps': 2 * nb16 / copy_ms / 1e6,
          'parse_fraction_of_stream_copy_time': copy_ms / parse_ms,
          'canonical_ms': canon_ms, 'csr_ms': csr_ms,
          'read_edge_list_device_ms': total_ms, 'reps': REPS}, out)


def _resident(path, dev):
    """The whole file in HBM (one chunk, whatever its size)."""
    return torch.from_numpy(np.fromfile(path, dtype=np.uint8)).to(dev)


def part_weighted(edges, plain_path, plain_bytes, tmp, dev, out):
    import pandas as pd
    m_raw = len(edges)
    path = os.path.join(tmp, 'weighted.txt')
    w = np.random.default_rng(0).random(m_raw) + 0.5
    pd.DataFrame({'u': edges[:, 0], 'v': edges[:, 1], 'w': w}).to_csv(
        path, sep=' ', header=False, index=False)
    n_bytes = os.path.getsize(path)
    s = _native.stream(dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_edgelist_workspace_bytes', n_bytes, 0, ctypes.byref(nb))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    cap = m_raw + 1
    src = torch.empty(cap, dtype=torch.int64, device=dev)
    dst = torch.empty(cap, dtype=torch.int64, device=dev)
    wt = torch.empty(cap, dtype=torch.float64, device=dev)
    und = torch.empty(2 * el.UNDECIDED_CAPACITY, dtype=torch.int64, device=dev)
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    pow5 = el._pow5_device(dev)
    text = _resident(path, dev)
    weighted_ms = best_event_ms(lambda: _native.call(
        'dw_edgelist_parse_weighted', _native.ptr(text), n_bytes, 0, _native.ptr(pow5),
        _native.ptr(src), _native.ptr(dst), _native.ptr(wt), cap, _native.ptr(und),
        el.UNDECIDED_CAPACITY, _native.ptr(info), _native.ptr(info[3:]), _native.ptr(status),
        _native.ptr(ws), ws.numel(), s), dev)
    m, _, n_und, _ = info.tolist()
    assert m == m_raw and int(status.item()) == 0
    exact = bool(np.array_equal(wt[:m].cpu().numpy().view(np.uint64), w.view(np.uint64)))
    del text
    text = _resident(plain_path, dev)
    id_only_ms = best_event_ms(lambda: _native.call(
        'dw_edgelist_parse', _native.ptr(text), plain_bytes, 0, _native.ptr(src),
        _native.ptr(dst), cap, _native.ptr(info), _native.ptr(info[2:]), _native.ptr(status),
        _native.ptr(ws), ws.numel(), s), dev)
    assert int(info[0]) == m_raw and int(status.item()) == 0
    del text, ws, src, dst, wt, und
    total_ms = best_wall_ms(lambda: el.read_edge_list(path, device=dev, weighted=True), dev)
    emit({'part': 'weighted', 'lines': m_raw, 'weighted_file_bytes': n_bytes,
          'id_only_file_bytes': plain_bytes, 'weighted_parse_ms': weighted_ms,
          'weighted_parse_gbps': n_bytes / weighted_ms / 1e6, 'id_only_parse_ms': id_only_ms,
          'id_only_parse_gbps': plain_bytes / id_only_ms / 1e6,
          'time_ratio': weighted_ms / id_only_ms, 'bytes_ratio': n_bytes / plain_bytes,
          'undecided_tokens': n_und, 'weights_equal_float_before_patch': exact,
          'read_edge_list_device_weighted_ms': total_ms, 'reps': REPS}, out)


def part_host(path, n_bytes, m_raw, out):
    t0 = time.perf_counter()
    src, dst = el.read_edge_arrays(path)
    t1 = time.perf_counter()
    g = el.edge_list_csr(src, dst)
    t2 = time.perf_counter()
    emit({'part': 'host', 'file_bytes': n_bytes, 'lines': m_raw, 'nodes': g.vocab_size - 1,
          'parse_ms': (t1 - t0) * 1e3, 'build_ms': (t2 - t1) * 1e3,
          'read_edge_list_host_ms': (t2 - t0) * 1e3}, out)


def part_parent(tmp, dev, out):
    import networkx as nx
    import pandas as pd
    from shallow_encoders.graph.csr import CSRGraph
    edges, _ = rmat_edges(16, 655_360, seed=0)
    path = os.path.join(tmp, 'rmat16.txt')
    n_bytes = write_text(edges, path)
    t0 = time.perf_counter()
    df = pd.read_csv(path, sep=' ', header=None, names=['source', 'target'])
    df['source'] = 'n' + df['source'].astype(str).str.zfill(7)
    df['target'] = 'n' + df['target'].astype(str).str.zfill(7)
    g = CSRGraph.from_networkx(nx.from_pandas_edgelist(df))
    parent_ms = (time.perf_counter() - t0) * 1e3
    host_ms = best_wall_ms(lambda: el.read_edge_list(path), reps=1)
    dev_ms = best_wall_ms(lambda: el.read_edge_list(path, device=dev), dev)
    new = el.read_edge_list(path, device=dev)
    same = bool(np.array_equal(new.row_ptr, g.row_ptr) and np.array_equal(new.host_col(), g.col))
    emit({'part': 'parent', 'scale': 16, 'file_bytes': n_bytes, 'lines': len(edges),
          'pandas_networkx_from_networkx_ms': parent_ms, 'read_edge_list_host_ms': host_ms,
          'read_edge_list_device_ms': dev_ms, 'same_csr': same}, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--part', default='all', choices=['device', 'host', 'weighted', 'parent', 'all'])
    ap.add_argument('--json', default=None)
    ap.add_argument('--scale', type=int, default=20)
    ap.add_argument('--draws', type=int, default=10_000_000)
    args = ap.parse_args()
    dev = _native.require_device(None)   # no device: an error, not a CPU timing
    with tempfile.TemporaryDirectory() as tmp:
        if args.part in ('device', 'host', 'weighted', 'all'):
            edges, _ = rmat_edges(args.scale, args.draws, seed=0)
            path = os.path.join(tmp, f'rmat{args.scale}.txt')
            n_bytes = write_text(edges, path)
            if args.part in ('device', 'all'):
                part_device(path, n_bytes, len(edges), dev, args.json)
            if args.part in ('weighted', 'all'):
                part_weighted(edges, path, n_bytes, tmp, dev, args.json)
            if args.part in ('host', 'all'):
                part_host(path, n_bytes, len(edges), args.json)
        if args.part in ('parent', 'all'):
            part_parent(tmp, dev, args.json)


if __name__ == '__main__':
    main()
