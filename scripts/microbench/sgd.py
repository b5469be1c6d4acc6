"""The SGD optimizer (csrc/dw_sgd.hip, word2vec/optim.SGD) at the C3 shapes: R-MAT 20
(V = 1,048,577), d = 128, walks of L = 80, R = 5, K = 5.

  dense   dw_sgd_dense over one table (plain, and with momentum), gradient refilled before every
          timed call so the pass moves its full 16 (24) bytes per element, beside dw_stream_copy
          of the same table in the same process (the measured HBM roofline);
  rows    dw_sgd_rows at the 64-walk id counts: the centres (4,480 int32 ids, the input table)
          and the walks + negatives (5,120 int32 + 224,000 int64 ids, the output table), the
          listed rows' gradient refilled before every timed call; bytes by the model
          16 d per distinct row + the id reads;
  step    Word2VecTrainer's eager step (walker + training_step + optimizer.step) at 64 walks in
          three forms on the same build and box, alternating windows: HIP SGD by rows, HIP SGD
          forced dense (SGD.force_dense), and the HIP Adam's fused step.

    python scripts/microbench/sgd.py [--part dense|rows|step|all] [--json PATH]

One JSON line per case on stdout, appended to --json (default profiles/sgd.jsonl).
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.graph.random_walk_generator import DeepWalk  # noqa: E402
from shallow_encoders.graph.rmat import rmat_graph  # noqa: E402
from shallow_encoders.word2vec.model import SkipGram  # noqa: E402
from shallow_encoders.word2vec.optim import SGD, Adam, rows_apply  # noqa: E402
from shallow_encoders.word2vec.sgns import device_noise  # noqa: E402
from shallow_encoders.word2vec.trainer import Word2VecTrainer  # noqa: E402

SCALE, EDGES, D, R, K, L, WALKS = 20, 10_000_000, 128, 5, 5, 80, 64
V = (1 << SCALE) + 1
CENTRES = WALKS * (L - 2 * R)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'a') as f:
            f.write(line + '\n')


def timed(prepare, run, reps, dev):
    """Per-call ms (device events around each call; ``prepare`` runs untimed before it)."""
    ms = []
    for _ in range(reps):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {'mean_ms': sum(ms) / len(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def part_dense(dev, path, reps=20):
    n = V * D
    p = torch.randn(n, device=dev) * 0.01
    g = torch.empty(n, device=dev)
    buf = torch.zeros(n, device=dev)
    dst = torch.empty(n, device=dev)
    s = _native.stream(dev)

    def copy():
        _native.call('dw_stream_copy', _native.ptr(p), _native.ptr(dst), n * 4, s)

    def dense(mu):
        _native.call('dw_sgd_dense', _native.ptr(p), _native.ptr(g), _native.ptr(buf) if mu else None,
                     n, -0.025, 0.0, mu, 1.0, 0, 0, 1, s)
    for f in (copy, lambda: dense(0.0), lambda: dense(0.9)):   # warm up every shape timed
        g.fill_(1e-3)
        f()
    torch.cuda.synchronize(dev)
    c = stats(timed(lambda: None, copy, reps, dev))
    copy_gbps = 2 * n * 4 / c['mean_ms'] / 1e6
    emit({'part': 'dense', 'case': 'dw_stream_copy', 'elements': n, 'bytes': 2 * n * 4, **c,
          'GBps': copy_gbps}, path)
    for name, mu, per in (('plain', 0.0, 16), ('momentum', 0.9, 24)):
        t = stats(timed(lambda: g.fill_(1e-3), lambda: dense(mu), reps, dev))
        gbps = n * per / t['mean_ms'] / 1e6
        emit({'part': 'dense', 'case': f'dw_sgd_dense/{name}', 'V': V, 'd': D, 'elements': n,
              'bytes_per_element': per, 'bytes': n * per, **t, 'GBps': gbps,
              'of_stream_copy': gbps / copy_gbps}, path)


def batch_ids(csr, dev):
    """One 64-walk batch's id lists: centres, walks, negatives (the trainer's, noise='device')."""
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    starts = torch.arange(1, WALKS + 1, dtype=torch.int32, device=dev)
    walks = walker.walk_batch(starts, walk_id0=0)
    centres = walks[:, R:L - R].contiguous()
    noise = device_noise(CENTRES, 2 * R, K, V, 1, 0, dev)
    return centres, walks, noise


def part_rows(csr, dev, path, reps=20):
    centres, walks, noise = batch_ids(csr, dev)
    p = torch.randn(V, D, device=dev) * 0.01
    g = torch.zeros(V, D, device=dev)
    claim = torch.zeros((V + 31) // 32, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = _native.stream(dev)

    def rows(lists):
        for t in lists:
            _native.call('dw_sgd_rows', _native.ptr(p), _native.ptr(g), V, D, _native.ptr(t),
                         t.element_size(), t.numel(), _native.ptr(claim), -0.025,
                         _native.ptr(status), s)
    for name, lists in (('in: centres', [centres]), ('out: walks + negatives', [walks, noise])):
        distinct = torch.unique(torch.cat([t.reshape(-1).long() for t in lists]))
        n_ids = sum(t.numel() for t in lists)
        id_bytes = sum(t.numel() * t.element_size() for t in lists)

        def refill():
            g[distinct] = 1e-3
        refill()
        rows(lists)                                     # warm-up
        t = stats(timed(refill, lambda: rows(lists), reps, dev))
        model = int(distinct.numel()) * 16 * D + id_bytes
        emit({'part': 'rows', 'case': f'dw_sgd_rows/{name}', 'V': V, 'd': D, 'n_ids': n_ids,
              'distinct_rows': int(distinct.numel()), 'model_bytes': model,
              'dense_bytes': 16 * D * V, 'goes_by_rows': rows_apply(n_ids, V), **t,
              'model_GBps': model / t['mean_ms'] / 1e6}, path)
    assert int(status.item()) == 0 and not bool(claim.any())


def make_trainer(kind, dev):
    torch.manual_seed(0)
    model = SkipGram(V, D).to(dev)
    if kind == 'adam_fused':
        opt = Adam(model.parameters(), lr=0.01)
    else:
        opt = SGD(model.parameters(), lr=0.025)
        opt.force_dense = kind == 'sgd_dense'
    tr = Word2VecTrainer(model, opt, None, neg_samples=K, vocab_size=V, noise='device', seed=1,
                         context_radius=R)
    tr.manual_grads = True
    return tr, opt


def part_step(csr, dev, path, warmup, steps, rounds):
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    starts = torch.arange(1, WALKS + 1, dtype=torch.int32, device=dev)
    walks = torch.empty((WALKS, L), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = {k: make_trainer(k, dev) for k in ('sgd_rows', 'sgd_dense', 'adam_fused')}
    count = {k: 0 for k in runs}

    def step(k):
        tr, opt = runs[k]
        walker.walk_batch(starts, walk_id0=count[k] * WALKS, out=walks, check=False,
                          status=status)
        tr.training_step(walks)
        opt.step()
        opt.zero_grad()
        count[k] += 1
    for k in runs:
        for _ in range(warmup):
            step(k)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k in runs:   # alternating windows
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(k)
            b.record()
            torch.cuda.synchronize(dev)
            ms[k].append(a.elapsed_time(b) / steps)
    assert int(status.item()) == 0
    for k in ('sgd_rows', 'sgd_dense'):
        runs[k][1].check_status()
    applied = {k: sorted(runs[k][1].last_apply.values()) for k in ('sgd_rows', 'sgd_dense')}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    emit({'part': 'step', 'walks': WALKS, 'centres': CENTRES, 'V': V, 'd': D,
          'steps_per_window': steps, 'ms_per_step': ms, 'mean_ms': mean,
          'spread_ms': {k: max(v) - min(v) for k, v in ms.items()}, 'last_apply': applied,
          'rows_faster_than_dense_by_more_than_the_spreads':
              min(ms['sgd_dense']) - max(ms['sgd_rows']) > 0,
          'rows_over_dense': mean['sgd_rows'] / mean['sgd_dense'],
          'rows_over_adam_fused': mean['sgd_rows'] / mean['adam_fused'],
          'last_loss': {k: float(runs[k][0].logged['train/loss']) for k in runs}}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'dense', 'rows', 'step'])
    ap.add_argument('--json', default=os.path.join(REPO, 'profiles', 'sgd.jsonl'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    _native.require_device(dev)
    if args.part in ('all', 'dense'):
        part_dense(dev, args.json)
    if args.part in ('all', 'rows', 'step'):
        csr = rmat_graph(SCALE, EDGES, 0, device=dev)
        assert csr.vocab_size == V
        if args.part in ('all', 'rows'):
            part_rows(csr, dev, args.json)
        if args.part in ('all', 'step'):
            part_step(csr, dev, args.json, args.warmup, args.steps, args.rounds)


if __name__ == '__main__':
    main()
