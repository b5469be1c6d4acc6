"""Cost of device k-means (shallow_encoders/graph/cluster.py) at V = 2^20 + 1 rows (row 0 is
<unk>, n = 2^20 samples), a random float32 table and random centroids — a pass's cost does not
depend on the data.

  yardstick   scripts/microbench/mfma_f64_peak: the float64 MFMA rate of a bare
              v_mfma_f64_16x16x4_f64 loop, on the same box in the same call;
  step        dw_kmeans_step, ms per pass for (dim, K) in SHAPES, and for K <= 64 dw_node_softmax
              at the same (n, dim, K) in alternating windows of one process (medians of WINDOWS
              windows of --reps launches between device events, after a warm-up window); the MFMA
              FLOP/s of each (what the instruction stream executes: the scores 2 n Kp dim with
              Kp = K rounded up to 16, the sums 2 n Ks dim with Ks = Kp below 64 clusters and K
              rounded up to 64 above; 4 n Kp dim for the softmax pass) and their fraction of the
              yardstick;
  kmeans      the wall time of one whole kmeans() run (ITERATIONS Lloyd updates from an explicit
              init) at (128, 47);
  sklearn     sklearn.cluster.KMeans from the same init, as many iterations, on the float64 copy
              of the same rows, 16 threads.

    python scripts/microbench/cluster.py [--json PATH] [--part all|yardstick|step|kmeans|sklearn]

Without --part every part runs in a process of its own under `timeout`, one after the other, and
the run stops at the first that fails. One JSON line per record on stdout (and appended to
--json, default profiles/cluster.jsonl).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

HERE = os.path.dirname(os.path.abspath(__file__))
PEAK_BIN = os.path.join(HERE, 'mfma_f64_peak')
N = 1 << 20
SHAPES = ((128, 2), (128, 7), (128, 47), (128, 64), (128, 256), (128, 1024), (256, 47))
WINDOWS = 5
ITERATIONS = 20


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def part_yardstick(path):
    if not os.path.exists(PEAK_BIN):
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-o', PEAK_BIN,
                        PEAK_BIN + '.hip'], check=True)
    out = subprocess.run([PEAK_BIN], check=True, capture_output=True, text=True).stdout
    rec = json.loads(out.strip().splitlines()[-1])
    emit(rec, path)
    return rec['flops']


def problem(d, dev):
    import torch
    torch.manual_seed(0)
    table = torch.randn((N + 1, d), dtype=torch.float32, device=dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev)
    return table, ids


def part_step(path, reps, peak):
    import torch
    from shallow_encoders.graph import cluster, nodeclf
    dev = torch.device('cuda', 0)
    for d, K in SHAPES:
        table, ids = problem(d, dev)
        cent = torch.randn((K, d), dtype=torch.float64, device=dev)
        ws = cluster.step_workspace(N, d, K, dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        prev = torch.zeros(N, dtype=torch.int32, device=dev)
        runs = {'kmeans_step': lambda: cluster.kmeans_step(table, ids, cent, prev, labels, ws,
                                                           check=False)}
        if 2 <= K <= 64:
            y = torch.randint(0, K, (N,), dtype=torch.int32, device=dev)
            coef = (torch.randn((K, d + 1), dtype=torch.float64, device=dev) / d ** 0.5)
            nws = nodeclf.softmax_workspace(N, d, K, dev)
            pred = torch.empty(N, dtype=torch.int32, device=dev)
            runs['node_softmax'] = lambda: nodeclf.softmax_sums(table, ids, y, coef, K, nws,
                                                                pred=pred, check=False)

        def window(run, r):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(r):
                run()
            b.record()
            torch.cuda.synchronize(dev)
            return a.elapsed_time(b) / r
        r = max(2, reps // 4) if K >= 256 else reps
        for run in runs.values():   # warm-up
            window(run, 2)
        ms = {name: [] for name in runs}
        for _ in range(WINDOWS):   # alternating: drift on a shared box hits both alike
            for name, run in runs.items():
                ms[name].append(window(run, r))
        med = {name: statistics.median(v) for name, v in ms.items()}
        kp = (K + 15) // 16 * 16
        ks = kp if K < 64 else (K + 63) // 64 * 64
        flop = {'kmeans_step': 2.0 * N * d * (kp + ks), 'node_softmax': 4.0 * N * kp * d}
        rec = {'part': 'step', 'd': d, 'K': K, 'samples': N, 'ms_per_pass': med, 'ms_windows': ms,
               'mfma_flop': {k: flop[k] for k in runs},
               'mfma_flops': {k: flop[k] / med[k] * 1e3 for k in runs},
               'useful_flops': 4.0 * N * K * d / med['kmeans_step'] * 1e3,
               'spread': (max(ms['kmeans_step']) - min(ms['kmeans_step'])) / med['kmeans_step']}
        if 'node_softmax' in runs:
            rec['ratio_to_node_softmax'] = med['kmeans_step'] / med['node_softmax']
        if peak:
            rec['mfma_f64_peak_flops'] = peak
            rec['fraction_of_mfma_f64_peak'] = {k: rec['mfma_flops'][k] / peak for k in runs}
        emit(rec, path)
        del table, ids, ws, labels, prev, runs


def _init(table, K):
    return table[1:K + 1].double().cpu().numpy()


def part_kmeans(path, d=128, K=47):
    import torch
    from shallow_encoders.graph import cluster
    dev = torch.device('cuda', 0)
    table, ids = problem(d, dev)
    init = _init(table, K)
    cluster.kmeans(table, ids, K, init=init, max_iter=2, device=dev)   # warm-up
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    _, _, inertia, n_iter = cluster.kmeans(table, ids, K, init=init, max_iter=ITERATIONS,
                                           device=dev)
    torch.cuda.synchronize(dev)
    emit({'part': 'kmeans', 'd': d, 'K': K, 'samples': N, 'seconds': time.perf_counter() - t0,
          'iterations': n_iter, 'passes': n_iter + 1, 'inertia': inertia}, path)


def part_sklearn(path, d=128, K=47):
    import numpy as np
    import torch
    from sklearn.cluster import KMeans
    dev = torch.device('cuda', 0)
    table, _ = problem(d, dev)   # the same rows and init as part_kmeans
    init = _init(table, K)
    X = table[1:].cpu().numpy().astype(np.float64)
    del table
    t0 = time.perf_counter()
    km = KMeans(n_clusters=K, init=init, n_init=1, max_iter=ITERATIONS, tol=0.0,
                algorithm='lloyd').fit(X)
    emit({'part': 'sklearn', 'd': d, 'K': K, 'samples': N, 'seconds': time.perf_counter() - t0,
          'iterations': int(km.n_iter_), 'inertia': float(km.inertia_),
          'threads': int(os.environ.get('OMP_NUM_THREADS', 0))}, path)


def run_all(args):
    """Every part in a process of its own under `timeout`; stops at the first failure."""
    peak = None
    for part, limit in (('yardstick', 120), ('step', 300), ('kmeans', 200), ('sklearn', 400)):
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__),
               '--part', part, '--reps', str(args.reps), '--json', args.json]
        if peak:
            cmd += ['--peak', repr(peak)]
        if part == 'yardstick':   # its rate goes to the parts behind it
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
        else:
            r = subprocess.run(cmd)
        if r.returncode != 0:
            sys.exit(f'part {part} ended with status {r.returncode}: stopping')
        if part == 'yardstick':
            peak = json.loads(r.stdout.strip().splitlines()[-1])['flops']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all',
                    choices=['all', 'yardstick', 'step', 'kmeans', 'sklearn'])
    ap.add_argument('--json', default=os.path.join(REPO, 'profiles', 'cluster.jsonl'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--peak', type=float, default=None, help='the yardstick\'s FLOP/s')
    args = ap.parse_args()
    if args.part == 'all':
        run_all(args)
    elif args.part == 'yardstick':
        part_yardstick(args.json)
    elif args.part == 'step':
        part_step(args.json, args.reps, args.peak)
    elif args.part == 'kmeans':
        part_kmeans(args.json)
    else:
        part_sklearn(args.json)


if __name__ == '__main__':
    main()
