"""Cost of the unigram^0.75 negatives (noise='unigram') at the headline shape C3: R-MAT 20,
8,192 walks of L = 80 per step, R = 5, K = 5, d = 128 — 573,440 centres, 28.7M negatives.

  build   dw_noise_alias_build on the host, V = 1,048,577 (the graph's degree^0.75) and
          V = 16,777,217 (a shuffled rank^-1.2 law), seconds;
  fill    dw_sgns_noise_alias alone (the materialised int64 [B', 2R, K] tensor, 229 MB) against
          dw_sgns_noise (the uniform fill), device events around REPS launches;
  step    Word2VecTrainer's fused step (walker + training_step + optimizer.step) with
          noise='unigram' against noise='device' on the same build, alternating, ROUNDS windows
          of STEPS steps each after WARMUP.

    python scripts/microbench/noise_alias.py [--part build|fill|step|all] [--json PATH]

One JSON line per part on stdout (and appended to --json). `--part once` runs a few steps of
each mode for a kernel-trace pass (rocprofv3 --kernel-trace --stats -- python ... --part once).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders.graph.random_walk_generator import DeepWalk  # noqa: E402
from shallow_encoders.graph.rmat import rmat_graph  # noqa: E402
from shallow_encoders.word2vec.model import SkipGram  # noqa: E402
from shallow_encoders.word2vec.optim import Adam  # noqa: E402
from shallow_encoders.word2vec.sgns import (device_noise, unigram_noise,  # noqa: E402
                                            unigram_table, unigram_table_host)
from shallow_encoders.word2vec.trainer import Word2VecTrainer  # noqa: E402

SCALE, EDGES, D, R, K, L, WALKS = 20, 10_000_000, 128, 5, 5, 80, 8192
CENTRES = WALKS * (L - 2 * R)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def part_build(degrees, path):
    big = np.arange(1, 16_777_217 + 1, dtype=np.float64) ** -1.2
    np.random.default_rng(0).shuffle(big)
    for name, w in (('rmat20_degrees', torch.as_tensor(degrees)), ('rank^-1.2 shuffled',
                                                                   torch.as_tensor(big))):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            unigram_table_host(w, 0.75)
            ts.append(time.perf_counter() - t0)
        emit({'part': 'build', 'weights': name, 'V': int(w.numel()), 'seconds': ts,
              'best_s': min(ts)}, path)


def part_fill(table, dev, path, reps=20):
    V = int(table.numel())
    out = torch.empty((CENTRES, 2 * R, K), dtype=torch.int64, device=dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps
    uni = timed(lambda i=0: unigram_noise(CENTRES, 2 * R, K, table, 1, i * CENTRES, dev, out=out))
    flat = timed(lambda i=0: device_noise(CENTRES, 2 * R, K, V, 1, i * CENTRES, dev))
    nbytes = out.numel() * 8
    emit({'part': 'fill', 'negatives': out.numel(), 'bytes_written': nbytes,
          'alias_ms': uni, 'alias_write_GBps': nbytes / uni / 1e6,
          'uniform_ms': flat, 'uniform_note': 'dw_sgns_noise allocates its output per call',
          'table_bytes': V * 8}, path)


def make_trainer(mode, V, degrees, dev):
    torch.manual_seed(0)
    model = SkipGram(V, D).to(dev)
    opt = Adam(model.parameters(), lr=0.01)
    kw = dict(noise_weights=torch.as_tensor(degrees)) if mode == 'unigram' else {}
    tr = Word2VecTrainer(model, opt, None, neg_samples=K, vocab_size=V, noise=mode, seed=1,
                         context_radius=R, **kw)
    tr.manual_grads = True
    return tr, opt


def part_step(csr, degrees, dev, path, warmup, steps, rounds):
    V = csr.vocab_size
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    starts = torch.arange(1, WALKS + 1, dtype=torch.int32, device=dev)
    walks = torch.empty((WALKS, L), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = {m: make_trainer(m, V, degrees, dev) for m in ('device', 'unigram')}
    count = {m: 0 for m in runs}

    def step(m):
        tr, opt = runs[m]
        walker.walk_batch(starts, walk_id0=count[m] * WALKS, out=walks, check=False,
                          status=status)
        tr.training_step(walks)
        opt.step()
        opt.zero_grad()
        count[m] += 1
    for m in runs:
        for _ in range(warmup):
            step(m)
    torch.cuda.synchronize(dev)
    ms = {m: [] for m in runs}
    for _ in range(rounds):
        for m in runs:   # alternating windows
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(m)
            b.record()
            torch.cuda.synchronize(dev)
            ms[m].append(a.elapsed_time(b) / steps)
    assert int(status.item()) == 0
    best = {m: min(v) for m, v in ms.items()}
    losses = {m: float(runs[m][0].logged['train/loss']) for m in runs}
    emit({'part': 'step', 'walks': WALKS, 'centres': CENTRES, 'steps_per_window': steps,
          'ms_per_step': ms, 'best_ms': best,
          'unigram_over_device': best['unigram'] / best['device'], 'last_loss': losses}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'build', 'fill', 'step', 'once'])
    ap.add_argument('--json', default=None)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    csr = rmat_graph(SCALE, EDGES, 0, device=dev)
    degrees = np.diff(csr.row_ptr).astype(np.float64)
    if args.part in ('all', 'build'):
        part_build(degrees, args.json)
    if args.part in ('all', 'fill'):
        part_fill(unigram_table(torch.as_tensor(degrees), 0.75, device=dev), dev, args.json)
    if args.part in ('all', 'step'):
        part_step(csr, degrees, dev, args.json, args.warmup, args.steps, args.rounds)
    if args.part == 'once':
        part_step(csr, degrees, dev, None, 2, 5, 1)


if __name__ == '__main__':
    main()
