import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'deepwalk-and-node2vec_amd')
GOLDEN = os.path.join(REPO, 'tests', 'golden')
for p in (PKG, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs an MI355X (HIP device) and libdw_hip.so')
    config.addinivalue_line('markers', 'slow: long-running parity case')


class _GoldenParts(dict):
    """A fixture stored as several .npz files (make_golden.save(parts=...): every committed file
    stays under 1 MiB), read as one."""

    @property
    def files(self):
        return list(self)


def golden(name):
    path = os.path.join(GOLDEN, name)
    f = np.load(path, allow_pickle=False)
    parts = sorted(glob.glob(glob.escape(os.path.splitext(path)[0]) + '.part*.npz'))
    if not parts:
        return f
    merged = _GoldenParts((k, f[k]) for k in f.files)
    for p in parts:
        with np.load(p, allow_pickle=False) as g:
            merged.update((k, g[k]) for k in g.files)
    return merged


@pytest.fixture(scope='session')
def hip_device():
    import torch
    from shallow_encoders import _native
    if not torch.cuda.is_available():
        pytest.fail('GPU test selected but no HIP device is visible')
    _native.load()
    return torch.device('cuda', 0)
