"""bench.py's own flows, end to end at small sizes (one process per case, each under a time
limit): the JSON line is printed and well formed, and its self-checks pass.

  * the one-GPU lazy owner path at the reference configs' 64-walk batch (the rows-major out
    step, eager warmup then graph replay) on an R-MAT 14 graph;
  * the headline composition (dense Adam, records path) with the batch64 line and its checked
    step, on an R-MAT 14 graph;
  * the C2 shape (HIP-graph replay, atomic scatter);
  * a plain run (no --full) of the C2 shape with --dump-outputs.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=240):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *args],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_lazy_owner_64_walks_small_graph():
    d = _bench('--scale', '14', '--edges', '100000', '--batch-walks', '64', '--n1-in-adam', 'lazy',
               '--steps', '32', '--warmup', '4', '--no-cpu-baseline', '--no-walk-bench',
               '--batch64-steps', '0')
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert 'owner path on one rank' in d['config']['parallelism']
    assert d['mean_loss'] is not None and 0 < d['mean_loss'] < 10


def test_bench_headline_with_batch64_small_graph():
    d = _bench('--full', '--scale', '14', '--edges', '100000', '--batch-walks', '512',
               '--steps', '8', '--warmup', '2', '--no-cpu-baseline', '--no-walk-bench',
               '--exact-steps', '0', '--batch64-steps', '32', '--batch64-long', '160')
    b = d['batch64']
    assert b['value'] > 0 and b['step_check']['ok'], b['step_check']
    # the steady-state leg: replays on to 160 steps, the last ones timed, then the check
    assert b['steady_state']['steps'] == 128 and b['steady_state']['ms_per_step'] > 0
    assert b['roofline']['touched_out_rows'] > 0 and b['roofline']['touched_in_rows'] > 0


def test_bench_c2_graph_replay():
    d = _bench('--config', 'c2', '--steps', '32', '--warmup', '2', '--no-cpu-baseline',
               '--no-walk-bench')
    assert d['value'] > 0 and d['roofline']['graph']


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, leaves out every part that takes a
    run of its own, and --dump-outputs writes the last step's arrays: float32 / float64 .npy
    files of at most 64 MB in all, the sampled rows trained away from their initial values and
    the walks node ids of the C2 graph."""
    import numpy as np
    out = tmp_path / 'dump'
    d = _bench('--config', 'c2', '--steps', '24', '--warmup', '2', '--dump-outputs', str(out))
    assert d['steps'] == 24 and d['warmup'] == 2 and d['ms_per_step'] > 0 and d['value'] > 0
    for k in ('metric', 'unit', 'higher_is_better', 'dtype'):
        assert k in d
    assert 'batch64' not in d and 'c5' not in d
    for k in ('cpu_baseline', 'walks_per_s', 'roofline_walk', 'walks_per_s_replay', 'exact_walks',
              'step_check'):
        assert d[k] is None, k
    assert d['roofline']['measured_copy_GBps'] is None
    files = sorted(os.listdir(out))
    assert files == ['loss_terms.npy', 'rows_in.npy', 'rows_out.npy', 'w_in.npy', 'w_out.npy',
                     'walks.npy']
    a = {f[:-4]: np.load(out / f, allow_pickle=False) for f in files}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    V = 4097                                        # R-MAT 12: 4,096 nodes + the padding row 0
    assert a['w_in'].shape == a['w_out'].shape == (V, 128) and a['w_in'].dtype == np.float32
    assert np.array_equal(a['rows_in'], np.arange(V)) and np.array_equal(a['rows_out'], a['rows_in'])
    lim = np.sqrt(6.0 / (V + 128))                  # the Xavier law of the initial tables
    assert (np.abs(a['w_in']) > lim).any() and (np.abs(a['w_out']) > lim).any()
    assert a['walks'].shape == (64, 10)
    assert np.array_equal(a['walks'], np.round(a['walks']))
    assert a['walks'].min() >= 0 and a['walks'].max() < V
    assert a['loss_terms'].shape == (4,) and (a['loss_terms'] != 0).any()
