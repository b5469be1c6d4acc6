"""Cost of device node classification (shallow_encoders/graph/nodeclf.py) at V = 2^20 + 1 rows
(row 0 is <unk>, n = 2^20 samples), a random float32 table and uniform random labels — the
pass's cost does not depend on the data.

  yardstick   scripts/microbench/mfma_f64_peak: the float64 MFMA rate of a bare
              v_mfma_f64_16x16x4_f64 loop, on the same box in the same call;
  pass        dw_node_softmax, ms per pass (median of WINDOWS windows of --reps launches between
              device events, after a warm-up window) for (dim, K) in SHAPES; its MFMA FLOP/s
              (4 n Kp dim with Kp = K rounded up to 16: what the instruction stream executes)
              as a fraction of the yardstick, and the useful share 4 n K dim;
  ovr         dw_node_ovr under both decision rules beside dw_node_softmax at the same shape,
              SHAPES plus (128, 39) (BlogCatalog's label count): windows of the three alternate
              in one process; ms per pass (medians), each rule's ratio to softmax and the
              softmax windows' spread, (max - min) / median — the yardstick of the ratios;
  fit         the wall time of one whole NodeLogisticRegression.fit at (128, 7);
  sklearn     LogisticRegression().fit on the float64 copy of the same features, 16 threads.

    python scripts/microbench/nodeclf.py [--json PATH] [--part all|yardstick|pass|ovr|fit|sklearn]

Without --part every part runs in a process of its own under `timeout`, one after the other, and
the run stops at the first that fails. One JSON line per record on stdout (and appended to
--json).
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
SHAPES = ((128, 2), (128, 7), (128, 47), (256, 47))
WINDOWS = 5


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


def problem(d, K, dev):
    import torch
    torch.manual_seed(0)
    table = torch.randn((N + 1, d), dtype=torch.float32, device=dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev)
    labels = torch.randint(0, K, (N,), dtype=torch.int32, device=dev)
    return table, ids, labels


def part_pass(path, reps, peak):
    import torch
    from shallow_encoders.graph import nodeclf
    dev = torch.device('cuda', 0)
    for d, K in SHAPES:
        table, ids, labels = problem(d, K, dev)
        coef = (torch.randn((K, d + 1), dtype=torch.float64, device=dev) / d ** 0.5).contiguous()
        ws = nodeclf.softmax_workspace(N, d, K, dev)
        pred = torch.empty(N, dtype=torch.int32, device=dev)

        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                nodeclf.softmax_sums(table, ids, labels, coef, K, ws, pred=pred, check=False)
            b.record()
            torch.cuda.synchronize(dev)
            return a.elapsed_time(b) / reps
        window()   # warm-up
        ms = [window() for _ in range(WINDOWS)]
        med = statistics.median(ms)
        kp = (K + 15) // 16 * 16
        mfma = 4.0 * N * kp * d
        rec = {'part': 'pass', 'd': d, 'K': K, 'samples': N, 'ms_per_pass': med,
               'ms_windows': ms, 'mfma_flop': mfma, 'mfma_flops': mfma / med * 1e3,
               'useful_flops': 4.0 * N * K * d / med * 1e3,
               'read_bytes': N * (4 * d + 12), 'read_GBps': N * (4 * d + 12) / med / 1e6}
        if peak:
            rec['mfma_f64_peak_flops'] = peak
            rec['fraction_of_mfma_f64_peak'] = rec['mfma_flops'] / peak
        emit(rec, path)
        del table, ids, labels, ws, pred


def part_ovr(path, reps):
    import torch
    from shallow_encoders.graph import nodeclf
    dev = torch.device('cuda', 0)
    for d, K in SHAPES + ((128, 39),):
        table, ids, labels = problem(d, K, dev)
        # about two labels a sample, as bit masks; bit 63 is never set at these K
        bits = torch.rand((N, K), device=dev) < min(2.0 / K, 0.5)
        masks = (bits.to(torch.int64) << torch.arange(K, device=dev)).sum(dim=1)
        del bits
        coef = (torch.randn((K, d + 1), dtype=torch.float64, device=dev) / d ** 0.5).contiguous()
        ws = nodeclf.ovr_workspace(N, d, K, dev)   # the longer row: serves softmax too
        pred32 = torch.empty(N, dtype=torch.int32, device=dev)
        pred64 = torch.empty(N, dtype=torch.int64, device=dev)
        runs = {
            'softmax': lambda: nodeclf.softmax_sums(table, ids, labels, coef, K, ws, pred=pred32,
                                                    check=False),
            'threshold': lambda: nodeclf.ovr_sums(table, ids, masks, coef, K, 'threshold', ws,
                                                  pred=pred64, check=False),
            'top_k': lambda: nodeclf.ovr_sums(table, ids, masks, coef, K, 'top_k', ws,
                                              pred=pred64, check=False)}

        def window(run):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                run()
            b.record()
            torch.cuda.synchronize(dev)
            return a.elapsed_time(b) / reps
        for run in runs.values():   # warm-up
            window(run)
        ms = {name: [] for name in runs}
        for _ in range(WINDOWS):   # alternating: drift on a shared box hits all three alike
            for name, run in runs.items():
                ms[name].append(window(run))
        med = {name: statistics.median(v) for name, v in ms.items()}
        emit({'part': 'ovr', 'd': d, 'K': K, 'samples': N, 'ms_per_pass': med, 'ms_windows': ms,
              'ratio_to_softmax': {name: med[name] / med['softmax']
                                   for name in ('threshold', 'top_k')},
              'softmax_spread': (max(ms['softmax']) - min(ms['softmax'])) / med['softmax']},
             path)
        del table, ids, labels, masks, ws, pred32, pred64


def part_fit(path, d=128, K=7):
    import torch
    from shallow_encoders.graph import nodeclf
    dev = torch.device('cuda', 0)
    table, ids, labels = problem(d, K, dev)
    y = labels.cpu().numpy()
    nodeclf.NodeLogisticRegression(max_iter=2).fit(table, ids, y)   # warm-up
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    clf = nodeclf.NodeLogisticRegression().fit(table, ids, y)
    torch.cuda.synchronize(dev)
    emit({'part': 'fit', 'd': d, 'K': K, 'samples': N, 'seconds': time.perf_counter() - t0,
          'iterations': clf.n_iter_, 'objective': clf.objective_}, path)


def part_sklearn(path, d=128, K=7):
    import numpy as np
    import torch
    from sklearn.linear_model import LogisticRegression
    torch.manual_seed(0)
    dev = torch.device('cuda', 0)
    table, _, labels = problem(d, K, dev)   # the same features and labels as part_fit
    X = table[1:].cpu().numpy().astype(np.float64)
    y = labels.cpu().numpy()
    del table
    t0 = time.perf_counter()
    clf = LogisticRegression().fit(X, y)
    emit({'part': 'sklearn', 'd': d, 'K': K, 'samples': N, 'seconds': time.perf_counter() - t0,
          'iterations': int(clf.n_iter_[0]),
          'threads': int(os.environ.get('OMP_NUM_THREADS', 0))}, path)


def run_all(args):
    """Every part in a process of its own under `timeout`; stops at the first failure."""
    peak = None
    for part, limit in (('yardstick', 120), ('pass', 300), ('ovr', 300), ('fit', 300),
                        ('sklearn', 400)):
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__),
               '--part', part, '--reps', str(args.reps)]
        if args.json:
            cmd += ['--json', args.json]
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
                    choices=['all', 'yardstick', 'pass', 'ovr', 'fit', 'sklearn'])
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--peak', type=float, default=None, help='the yardstick\'s FLOP/s')
    args = ap.parse_args()
    if args.part == 'all':
        run_all(args)
    elif args.part == 'yardstick':
        part_yardstick(args.json)
    elif args.part == 'pass':
        part_pass(args.json, args.reps, args.peak)
    elif args.part == 'ovr':
        part_ovr(args.json, args.reps)
    elif args.part == 'fit':
        part_fit(args.json)
    else:
        part_sklearn(args.json)


if __name__ == '__main__':
    main()
