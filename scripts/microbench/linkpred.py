"""Cost of device link prediction (shallow_encoders/graph/linkpred.py) at the headline shape C3:
the device-built R-MAT 20 (1,048,577 rows, 10M edge draws), d = 128.

  sampler     dw_negative_edges, 10^7 pairs, device events around REPS launches;
  logreg      dw_edge_logreg, one pass over 2 * 10^7 labelled pairs (10^7 edges in shuffled
              order + 10^7 sampled non-edges) of a random float32 table, against the byte model
              8 d + 17 B per sample and against dw_stream_copy's rate over a buffer of the same
              size as the table; d = 128 and d = 256;
  experiment  one whole edge_classification_device experiment (shuffle, both negative sets, the
              L-BFGS fit on 2 * n_train pairs, the score on 2 E pairs), wall clock.

    python scripts/microbench/linkpred.py [--part sampler|logreg|experiment|all] [--json PATH]

One JSON line per part on stdout (and appended to --json). `--part once` runs each kernel a few
times for a kernel-trace pass (rocprofv3 --kernel-trace --stats -- python ... --part once).
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph import linkpred  # noqa: E402
from shallow_encoders.graph.rmat import rmat_graph  # noqa: E402

SCALE, EDGES, N_PAIRS = 20, 10_000_000, 10_000_000
PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def timed(fn, dev, reps):
    fn(0)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i + 1)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def stream_copy_gbps(nbytes, dev, reps):
    nbytes -= nbytes % 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = timed(lambda i: _native.call('dw_stream_copy', _native.ptr(src), _native.ptr(dst), nbytes,
                                      _native.stream(dev)), dev, reps)
    return 2 * nbytes / ms / 1e6


def part_sampler(csr, dev, path, reps):
    d = csr.device_tensors(dev, need_sorted=True)
    linkpred.negative_edges(csr, 1, 0, device=dev)   # the graph checks, once
    pairs = torch.empty((N_PAIRS, 2), dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ms = timed(lambda i: _native.call(
        'dw_negative_edges', _native.ptr(d['row_ptr']), _native.ptr(d['col_sorted']),
        csr.vocab_size, 1, N_PAIRS, 1, i * N_PAIRS, _native.ptr(pairs), _native.ptr(st),
        _native.stream(dev)), dev, reps)
    assert int(st.item()) == 0
    emit({'part': 'sampler', 'pairs': N_PAIRS, 'ms': ms, 'pairs_per_s': N_PAIRS / ms * 1e3,
          'write_GBps': N_PAIRS * 16 / ms / 1e6}, path)


def labelled_pairs(csr, dev):
    pos = linkpred.positive_edges(csr, dev)
    pos = pos[torch.randperm(pos.shape[0], device=dev)][:N_PAIRS]
    neg = linkpred.negative_edges(csr, pos.shape[0], 2, device=dev)
    pairs = torch.cat([pos, neg])
    labels = torch.cat([torch.ones(pos.shape[0], dtype=torch.uint8, device=dev),
                        torch.zeros(neg.shape[0], dtype=torch.uint8, device=dev)])
    return pairs, labels


def part_logreg(csr, dev, path, reps, dims=(128, 256)):
    pairs, labels = labelled_pairs(csr, dev)
    n = pairs.shape[0]
    for d in dims:
        torch.manual_seed(0)
        table = torch.randn((csr.vocab_size, d), dtype=torch.float32, device=dev)
        coef = (torch.randn(d + 1, dtype=torch.float64, device=dev) / d ** 0.5).contiguous()
        ws = linkpred.logreg_workspace(n, d, dev)
        copy = stream_copy_gbps(table.numel() * 4, dev, reps)
        for op, name in ((1, 'hadamard'),):
            ms = timed(lambda i: linkpred.edge_logreg_sums(table, op, pairs, labels, coef, ws,
                                                           check=False), dev, reps)
            nbytes = n * (8 * d + 17)
            emit({'part': 'logreg', 'd': d, 'operator': name, 'samples': n, 'ms_per_pass': ms,
                  'model_bytes': nbytes, 'model_GBps': nbytes / ms / 1e6,
                  'fraction_of_peak': nbytes / ms / 1e6 / PEAK_GBPS,
                  'stream_copy_GBps': copy, 'fraction_of_stream_copy': nbytes / ms / 1e6 / copy,
                  'table_bytes': table.numel() * 4}, path)
        del table


def part_experiment(csr, dev, path, d=128):
    torch.manual_seed(0)
    table = torch.randn((csr.vocab_size, d), dtype=torch.float32, device=dev)
    linkpred.negative_edges(csr, 1, 0, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    mean, best, accs = linkpred.edge_classification_device(
        table, csr, 0.5, 1, 'hadamard', seed=0, device=dev, return_accuracies=True)
    torch.cuda.synchronize(dev)
    emit({'part': 'experiment', 'd': d, 'table': 'random normal', 'seconds': time.perf_counter()
          - t0, 'accuracy': accs}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all',
                    choices=['all', 'sampler', 'logreg', 'experiment', 'once'])
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    csr = rmat_graph(SCALE, EDGES, 0, device=dev)
    if args.part in ('all', 'sampler'):
        part_sampler(csr, dev, args.json, args.reps)
    if args.part in ('all', 'logreg'):
        part_logreg(csr, dev, args.json, args.reps)
    if args.part in ('all', 'experiment'):
        part_experiment(csr, dev, args.json)
    if args.part == 'once':
        part_sampler(csr, dev, None, 3)
        part_logreg(csr, dev, None, 3, dims=(128,))


if __name__ == '__main__':
    main()
