"""lr sweep of sge_sg_rmat20 under torch.optim.SGD (the HIP SGD): two epochs per lr (StepLR halves
the lr after the first), epoch-mean losses recorded; then the device link prediction of the
first epoch's checkpoint of the largest lr whose loss falls (both epoch means finite, the first
below the initial 6 ln 2, the second below the first). One JSON line per run, appended to
DW_SWEEP_JSON (default profiles/sgd_lr_sweep.jsonl, the recorded sweep behind
configs/sge_sg_rmat20_sgd.yaml's lr).

    python scripts/experiments/sgd_lr_sweep.py [lr ...]
"""
import csv
import json
import math
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(REPO, 'deepwalk-and-node2vec_amd')
sys.path.insert(0, PKG)

from tools import conventions  # noqa: E402
from tools import graph_model_downstream_classification as down  # noqa: E402
from tools import train as train_tool  # noqa: E402

OUT_JSON = os.environ.get('DW_SWEEP_JSON', os.path.join(REPO, 'profiles', 'sgd_lr_sweep.jsonl'))
INITIAL = 6 * math.log(2.0)     # the loss of the initial tables (logits ~ 0), K = 5


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT_JSON, 'a') as f:
        f.write(line + '\n')


def main():
    lrs = [float(x) for x in sys.argv[1:]] or [1e2, 1e3, 1e4, 1e5, 1e6]
    out = tempfile.mkdtemp(prefix='sgd_sweep_')
    os.makedirs(os.path.dirname(OUT_JSON), exist_ok=True)
    good = []
    for lr in lrs:
        exp = f'SG_rmat20_sgd_lr{lr:g}'
        ov = [f'path.output_dir={out}', f'output_dir={out}', f'train.experiment={exp}',
              'train.optimizer._target_=torch.optim.SGD', f'train.optimizer.lr={lr}',
              'train.max_epochs=2']
        t0 = time.perf_counter()
        try:
            train_tool.main(['--config-name', 'sge_sg_rmat20'] + ov)
            err = None
        except AssertionError as e:          # the epoch's NaN check
            err = str(e)
        losses = []
        path = os.path.join(conventions.get_tb_logs_experiment_path(out, 'graph_rmat', exp),
                            'metrics.csv')
        if os.path.exists(path):
            with open(path) as f:
                losses = [float(r['value']) for r in csv.DictReader(f)
                          if r['name'] == 'train-epoch/loss']
        falls = (err is None and len(losses) == 2 and all(math.isfinite(x) for x in losses)
                 and losses[0] < INITIAL and losses[1] < losses[0])
        emit({'part': 'lr_sweep', 'config': 'sge_sg_rmat20', 'optimizer': 'torch.optim.SGD',
              'lr': lr, 'epoch_loss': losses, 'initial_loss': INITIAL, 'falls': falls,
              'error': err, 'seconds': time.perf_counter() - t0})
        ckdir = conventions.get_checkpoints_experiment_path(out, 'graph_rmat', exp)
        if os.path.isdir(ckdir):             # keep the first epoch's checkpoint of a good lr only
            for n in os.listdir(ckdir):
                if not (falls and n.startswith('checkpoint_epoch=000000')):
                    os.remove(os.path.join(ckdir, n))
        if falls:
            good.append((lr, exp))
    if not good:
        emit({'part': 'lr_choice', 'lr': None})
        shutil.rmtree(out, ignore_errors=True)
        return
    lr, exp = max(good)
    ckdir = conventions.get_checkpoints_experiment_path(out, 'graph_rmat', exp)
    first = sorted(n for n in os.listdir(ckdir) if n.startswith('checkpoint_epoch=000000'))[0]
    res = down.main(['--config-name', 'sge_sg_rmat20', f'path.output_dir={out}',
                     f'output_dir={out}', f'train.experiment={exp}',
                     f'analysis.checkpoint={first}', 'downstream.node_classification.enable=false',
                     'downstream.edge_classification.backend=device'])
    emit({'part': 'lr_choice', 'lr': lr, 'checkpoint': first, 'epochs': 1,
          'edge_accuracy': res['edge_accuracy'], 'edge_best': res['edge_best'],
          'n_experiments': 10, 'operator': 'hadamard'})
    shutil.rmtree(out, ignore_errors=True)


if __name__ == '__main__':
    main()
