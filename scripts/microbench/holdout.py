"""Cost of held-out link prediction (shallow_encoders/graph/holdout.py, dw_edge_scores and
dw_roc_auc in csrc/dw_linkpred.hip) at the headline shape C3: the device-built R-MAT 20
(1,048,577 rows, 10M edge draws), d = 128. Everything is reported, nothing is gated.

  split    split_edges at ratio 0.5 on the device (wall clock around a synchronise, the workspace
           allocation and the one host read of the counts included) against the numpy host path;
           byte model: what the kernels must read and write at least once — row_ptr in and out
           (16 B per row), every entry's col in (4 B) and, kept, out (4 B), 16 B per held edge;
  scores   dw_edge_scores against dw_edge_logreg on the same 2 * 10^7 pairs, d = 128, hadamard,
           alternating five times after a warm-up; the medians (the scores pass does strictly
           less work, so its median should not exceed the logreg pass's); byte model
           8 d + 16 + 8 B per pair (two rows, the ids, z);
  auc      dw_roc_auc on 2 * 10^7 scores against sklearn.metrics.roc_auc_score on the host's
           threads; byte model 8 + 1 B per score in, twice (the key pass and the rank pass);
  forest   split_edges at ratio 0.5 with protect='connected' against protect='degree' in the
           same run (same clock as `split`), dw_edge_forest alone (events around the one
           asynchronous call), the rounds it used and, from a kernel trace of one call, each
           round's kernel times; byte model of a round: rows, col (4 B each) and two component
           labels (4 B each, gathered) per entry, in k_comp_min and again in k_hook;
  quality  one sge_sg_rmat20 epoch with holdout_ratio=0.5, then protocol=heldout (10
           experiments), per noise law and per holdout_protect rule: the held-out AUC and
           accuracy.

Each kernel's model bytes over its time are also given as a share of dw_stream_copy's rate.

    python scripts/microbench/holdout.py [--part split|forest|scores|auc|kernels|quality|all] [--json PATH]

One JSON line per part on stdout (and appended to --json, default profiles/holdout.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph import linkpred  # noqa: E402
from shallow_encoders.graph.csr import CSRGraph  # noqa: E402
from shallow_encoders.graph.holdout import split_edges  # noqa: E402
from shallow_encoders.graph.rmat import rmat_graph  # noqa: E402

SCALE, EDGES, N_PAIRS, D = 20, 10_000_000, 10_000_000, 128


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def event_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def stream_copy_gbps(nbytes, dev, reps=10):
    nbytes -= nbytes % 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def copy():
        _native.call('dw_stream_copy', _native.ptr(src), _native.ptr(dst), nbytes,
                     _native.stream(dev))
    copy()
    torch.cuda.synchronize(dev)
    ms = statistics.median(event_ms(copy, dev) for _ in range(reps))
    return 2 * nbytes / ms / 1e6


def part_split(csr, dev, path, reps=5):
    csr.require_simple(dev)
    split_edges(csr, 0.5, 0, device=dev)          # warm-up (code objects, the sort's choice)
    times = []
    for i in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        train, held, info = split_edges(csr, 0.5, i + 1, device=dev)
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) * 1e3)
    host = CSRGraph.from_arrays(csr.row_ptr, csr.host_col(), None, itos=csr.itos)
    t0 = time.perf_counter()
    h_train, h_held, h_info = split_edges(host, 0.5, reps, device=None)
    host_s = time.perf_counter() - t0
    same = (h_info == info and np.array_equal(h_held, held.cpu().numpy())
            and np.array_equal(h_train.row_ptr, train.row_ptr)
            and np.array_equal(h_train.col, train.host_col()))
    ms = statistics.median(times)
    nbytes = 16 * (csr.vocab_size + 1) + 4 * csr.nnz + 4 * train.nnz + 16 * info['n_hold']
    copy = stream_copy_gbps(nbytes, dev)
    emit({'part': 'split', 'rows': csr.vocab_size, 'nnz': csr.nnz, 'ratio': 0.5, **info,
          'device_ms': ms, 'device_ms_all': times, 'host_numpy_s': host_s,
          'device_equals_host': bool(same), 'model_bytes': nbytes,
          'model_GBps': nbytes / ms / 1e6, 'stream_copy_GBps': copy,
          'fraction_of_stream_copy': nbytes / ms / 1e6 / copy}, path)


def forest_call(csr, seed, dev):
    """One dw_edge_forest call on preallocated buffers: (launch, counts, status)."""
    import ctypes
    d = csr.device_tensors(dev)
    V, nnz = csr.vocab_size, csr.nnz
    nb = ctypes.c_size_t(0)
    _native.call('dw_edge_forest_workspace_bytes', V, nnz, ctypes.byref(nb))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    flags = torch.empty(nnz, dtype=torch.uint8, device=dev)
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch():
        _native.call('dw_edge_forest', _native.ptr(d['row_ptr']), _native.ptr(d['col']), V, nnz,
                     seed, _native.ptr(flags), _native.ptr(labels), _native.ptr(counts),
                     _native.ptr(status), _native.ptr(ws), ws.numel(), _native.stream(dev))
    return launch, counts, status


def forest_kernel_trace(launch, dev):
    """{kernel: [ms per launch, in launch order]} of one call, from torch's profiler; None when
    it records no device kernels here."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        launch()
        torch.cuda.synchronize(dev)
    out = {}
    events = sorted((ev for ev in prof.events() if 'cuda' in str(ev.device_type).lower()),
                    key=lambda ev: ev.time_range.start)
    for ev in events:
        for k in ('k_forest_init', 'k_forest_rows', 'k_comp_minid', 'k_comp_min', 'k_hook',
                  'k_compress', 'k_forest_count', 'k_forest_labels'):
            if k in ev.name:
                us = getattr(ev, 'device_time', None)
                us = ev.cuda_time if us is None else us
                out.setdefault(k, []).append(us / 1e3)
                break
    return out or None


def part_forest(csr, dev, path, reps=5):
    csr.require_simple(dev)
    times = {'degree': [], 'connected': []}
    for rule in times:
        split_edges(csr, 0.5, 0, device=dev, protect=rule)                   # warm-up
    for i in range(reps):
        for rule in times:                                                   # alternating
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            train, held, info = split_edges(csr, 0.5, i + 1, device=dev, protect=rule)
            torch.cuda.synchronize(dev)
            times[rule].append((time.perf_counter() - t0) * 1e3)
    launch, counts, status = forest_call(csr, reps, dev)
    launch()
    torch.cuda.synchronize(dev)
    forest_ms = [event_ms(launch, dev) for _ in range(reps)]
    assert int(status.item()) == 0
    n_edges, n_forest, n_comp, rounds = counts.tolist()
    try:
        trace = forest_kernel_trace(launch, dev)
    except Exception as exc:   # the profiler is an optional extra of the measurement
        trace = None
        print(f'no kernel trace: {exc!r}', file=sys.stderr)
    round_bytes = 2 * 16 * csr.nnz
    copy = stream_copy_gbps(round_bytes, dev)
    emit({'part': 'forest', 'rows': csr.vocab_size, 'nnz': csr.nnz, 'ratio': 0.5, **info,
          'connected_split_ms': statistics.median(times['connected']),
          'connected_split_ms_all': times['connected'],
          'degree_split_ms': statistics.median(times['degree']),
          'degree_split_ms_all': times['degree'],
          'forest_call_ms': statistics.median(forest_ms), 'forest_call_ms_all': forest_ms,
          'rounds': rounds, 'rounds_launched': (csr.vocab_size - 1).bit_length(),
          'n_forest_call': n_forest, 'n_components_call': n_comp,
          'kernel_ms': trace, 'round_model_bytes': round_bytes, 'stream_copy_GBps': copy,
          'round_model_ms_at_stream_copy': round_bytes / copy / 1e6}, path)


def labelled_pairs(csr, dev):
    pos = linkpred.positive_edges(csr, dev)
    pos = pos[torch.randperm(pos.shape[0], device=dev)][:N_PAIRS]
    neg = linkpred.negative_edges(csr, pos.shape[0], 2, device=dev)
    labels = torch.cat([torch.ones(pos.shape[0], dtype=torch.uint8, device=dev),
                        torch.zeros(neg.shape[0], dtype=torch.uint8, device=dev)])
    return torch.cat([pos, neg]), labels


def part_scores(csr, dev, path, rounds=5):
    pairs, labels = labelled_pairs(csr, dev)
    n = pairs.shape[0]
    torch.manual_seed(0)
    table = torch.randn((csr.vocab_size, D), dtype=torch.float32, device=dev)
    coef = (torch.randn(D + 1, dtype=torch.float64, device=dev) / D ** 0.5).contiguous()
    ws = linkpred.logreg_workspace(n, D, dev)
    z = torch.empty(n, dtype=torch.float64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)

    def scores():
        _native.call('dw_edge_scores', _native.ptr(table), table.shape[0], D, 1,
                     _native.ptr(pairs), n, _native.ptr(coef), _native.ptr(z), _native.ptr(st),
                     _native.stream(dev))

    def logreg():
        linkpred.edge_logreg_sums(table, 1, pairs, labels, coef, ws, check=False)
    for fn in (scores, logreg, scores, logreg):
        fn()
    torch.cuda.synchronize(dev)
    t_scores, t_logreg = [], []
    for _ in range(rounds):
        t_scores.append(event_ms(scores, dev))
        t_logreg.append(event_ms(logreg, dev))
    assert int(st.item()) == 0
    ms, ms_lr = statistics.median(t_scores), statistics.median(t_logreg)
    nbytes = n * (8 * D + 16 + 8)
    copy = stream_copy_gbps(table.numel() * 4, dev)
    emit({'part': 'scores', 'd': D, 'operator': 'hadamard', 'pairs': n, 'scores_ms': ms,
          'logreg_ms': ms_lr, 'scores_ms_all': t_scores, 'logreg_ms_all': t_logreg,
          'scores_not_slower': bool(ms <= ms_lr), 'model_bytes': nbytes,
          'model_GBps': nbytes / ms / 1e6, 'stream_copy_GBps': copy,
          'fraction_of_stream_copy': nbytes / ms / 1e6 / copy}, path)
    return z, labels


def part_auc(z, labels, dev, path, reps=5):
    from sklearn.metrics import roc_auc_score
    n = z.shape[0]
    linkpred.roc_auc(z, labels)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        auc = linkpred.roc_auc(z, labels)        # workspace allocation and the host read included
        times.append((time.perf_counter() - t0) * 1e3)
    zh, yh = z.cpu().numpy(), labels.cpu().numpy()
    t0 = time.perf_counter()
    want = roc_auc_score(yh, zh)
    host_s = time.perf_counter() - t0
    ms = statistics.median(times)
    nbytes = 2 * 9 * n
    copy = stream_copy_gbps(nbytes, dev)
    emit({'part': 'auc', 'scores': n, 'device_ms': ms, 'device_ms_all': times,
          'sklearn_s': host_s, 'threads': torch.get_num_threads(), 'auc': auc,
          'abs_diff_to_sklearn': abs(auc - want), 'model_bytes': nbytes,
          'model_GBps': nbytes / ms / 1e6, 'stream_copy_GBps': copy,
          'fraction_of_stream_copy': nbytes / ms / 1e6 / copy}, path)


def part_quality(path, noises=('device', 'unigram'), protects=('degree', 'connected')):
    import random

    from tools import graph_model_downstream_classification as downstream
    from tools import train as train_tool
    for noise, protect in [(n, p) for n in noises for p in protects]:
        with tempfile.TemporaryDirectory() as out:
            base = ['--config-name', 'sge_sg_rmat20', f'path.output_dir={out}',
                    f'output_dir={out}', f'train.noise={noise}', 'train.max_epochs=1',
                    'datamodule.additional_parameters.holdout_ratio=0.5',
                    f'datamodule.additional_parameters.holdout_protect={protect}',
                    'downstream.node_classification.enable=false']
            torch.manual_seed(0)
            random.seed(0)
            t0 = time.perf_counter()
            train_tool.main(base)
            train_s = time.perf_counter() - t0
            for scorer in ('classifier', 'dot'):
                t0 = time.perf_counter()
                res = downstream.main(base + ['downstream.edge_classification.protocol=heldout',
                                              'downstream.edge_classification.backend=device',
                                              f'downstream.edge_classification.scorer={scorer}'])
                emit({'part': 'quality', 'config': 'sge_sg_rmat20', 'epochs': 1, 'noise': noise,
                      'holdout_ratio': 0.5, 'holdout_protect': protect, 'scorer': scorer, **res,
                      'train_tool_s': train_s,
                      'downstream_tool_s': time.perf_counter() - t0}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all',
                    choices=['all', 'kernels', 'split', 'forest', 'scores', 'auc', 'quality'])
    ap.add_argument('--json', default=os.path.join(REPO, 'profiles', 'holdout.jsonl'))
    ap.add_argument('--noise', default=None, choices=['device', 'unigram'],
                    help='quality: one noise law instead of both')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    if args.part != 'quality':
        csr = rmat_graph(SCALE, EDGES, 0, device=dev)
        if args.part in ('all', 'kernels', 'split'):
            part_split(csr, dev, args.json)
        if args.part in ('all', 'kernels', 'forest'):
            part_forest(csr, dev, args.json)
        if args.part in ('all', 'kernels', 'scores', 'auc'):
            z, labels = part_scores(csr, dev, args.json if args.part != 'auc' else None)
            if args.part != 'scores':
                part_auc(z, labels, dev, args.json)
        del csr
    if args.part in ('all', 'quality'):
        part_quality(args.json, noises=(args.noise,) if args.noise else ('device', 'unigram'))


if __name__ == '__main__':
    main()
