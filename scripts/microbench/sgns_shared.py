"""Shared negatives per walk (Word2VecTrainer(shared_negatives=64)) at the headline shape C3:
R-MAT 20, 8,192 walks of L = 80 per step, R = 5, K = 5, d = 128 — 573,440 centres.

  step    Word2VecTrainer's step (walker + training_step + optimizer.step), noise='device', with
          shared_negatives=64 (dw_sgns_noise ids + dw_sgns_walks_shared + the dense HIP Adam)
          against shared_negatives=0 (the fused records step) on the same build and box,
          alternating, ROUNDS windows of STEPS steps each after WARMUP;
  kernel  dw_sgns_walks_shared alone on one batch of walks (device events around REPS launches)
          against its byte model (sgns.sgns_shared_bytes) and the 1.3 TB/s float-atomic rate.

    python scripts/microbench/sgns_shared.py [--part step|kernel|all] [--json PATH]

One JSON line per part on stdout (and appended to --json). `--part once` runs a few steps of
each mode for a kernel-trace pass (rocprofv3 --kernel-trace --stats -- python ... --part once).
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders.graph.random_walk_generator import DeepWalk  # noqa: E402
from shallow_encoders.graph.rmat import rmat_graph  # noqa: E402
from shallow_encoders.word2vec.model import SkipGram  # noqa: E402
from shallow_encoders.word2vec.optim import Adam  # noqa: E402
from shallow_encoders.word2vec.sgns import (device_noise, sgns_shared_accumulate,  # noqa: E402
                                            sgns_shared_bytes)
from shallow_encoders.word2vec.trainer import Word2VecTrainer  # noqa: E402

SCALE, EDGES, D, R, K, L, WALKS, S = 20, 10_000_000, 128, 5, 5, 80, 8192, 64
CENTRES = WALKS * (L - 2 * R)
ATOMIC_GBPS = 1300.0   # the chip-wide float-atomic ceiling


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def make_trainer(shared, V, dev):
    torch.manual_seed(0)
    model = SkipGram(V, D).to(dev)
    opt = Adam(model.parameters(), lr=0.01)
    tr = Word2VecTrainer(model, opt, None, neg_samples=K, vocab_size=V, noise='device', seed=1,
                         context_radius=R, shared_negatives=shared)
    tr.manual_grads = True
    return tr, opt


def part_step(csr, dev, path, warmup, steps, rounds):
    V = csr.vocab_size
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    starts = torch.arange(1, WALKS + 1, dtype=torch.int32, device=dev)
    walks = torch.empty((WALKS, L), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = {m: make_trainer(s, V, dev) for m, s in (('per_pair', 0), ('shared', S))}
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
    spread = {m: max(v) - min(v) for m, v in ms.items()}
    mean = {m: sum(v) / len(v) for m, v in ms.items()}
    losses = {m: float(runs[m][0].logged['train/loss']) for m in runs}
    emit({'part': 'step', 'walks': WALKS, 'centres': CENTRES, 'shared_negatives': S,
          'steps_per_window': steps, 'ms_per_step': ms, 'mean_ms': mean, 'spread_ms': spread,
          'gain_ms': mean['per_pair'] - mean['shared'],
          'faster_by_more_than_the_spreads':
              min(ms['per_pair']) - max(ms['shared']) > 0,
          'shared_over_per_pair': mean['shared'] / mean['per_pair'], 'last_loss': losses}, path)


def part_kernel(csr, dev, path, reps=20):
    V = csr.vocab_size
    walker = DeepWalk(csr, L, rng='philox', seed=3, device=dev)
    starts = torch.arange(1, WALKS + 1, dtype=torch.int32, device=dev)
    walks = torch.empty((WALKS, L), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    walker.walk_batch(starts, walk_id0=0, out=walks, check=False, status=status)
    torch.manual_seed(0)
    model = SkipGram(V, D).to(dev)
    w_in, w_out = model.input_weight.detach(), model.output_weight.detach()
    g_in, g_out = torch.zeros_like(w_in), torch.zeros_like(w_out)
    ids = device_noise(WALKS, 1, S, V, 1, 0, dev)
    acc = torch.zeros(4, dtype=torch.float64, device=dev)

    def run():
        sgns_shared_accumulate(w_in, w_out, g_in, g_out, K, walks=walks, context_radius=R,
                               shared_ids=ids, loss_acc=acc, status=status)
    run()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize(dev)
    ms = a.elapsed_time(b) / reps
    assert int(status.item()) == 0
    model_b = sgns_shared_bytes(WALKS, L, R, S, D)
    nct, nbt = -(-(L - 2 * R) // 32), -(-(L + S) // 32)
    flop = WALKS * 3 * 2 * (32 * nct) * (32 * nbt) * D     # three padded products per walk
    emit({'part': 'kernel', 'walks': WALKS, 'shared_negatives': S, 'ms': ms, 'bytes': model_b,
          'read_GBps': model_b['reads'] / ms / 1e6,
          'atomic_row_GBps': model_b['atomic_rows'] / ms / 1e6,
          'atomic_floor_ms': model_b['atomic_rows'] / ATOMIC_GBPS / 1e6,
          'mfma_flop': flop, 'mfma_TFLOPs': flop / ms / 1e9}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'step', 'kernel', 'once'])
    ap.add_argument('--json', default=None)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    csr = rmat_graph(SCALE, EDGES, 0, device=dev)
    if args.part in ('all', 'kernel'):
        part_kernel(csr, dev, args.json)
    if args.part in ('all', 'step'):
        part_step(csr, dev, args.json, args.warmup, args.steps, args.rounds)
    if args.part == 'once':
        part_step(csr, dev, None, 2, 5, 1)


if __name__ == '__main__':
    main()
