"""bench.py on one GPU at a small ad-hoc shape: the plain run (headline figure and the output dump only) and --full (every
figure beside it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ['--cells', '20000', '--genes', '2000', '--batch-size', '1024']


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + SHAPE + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    d = str(tmp_path / 'out')
    out = _bench('--steps', '5', '--warmup', '2', '--dump-outputs', d)
    assert out['steps'] == 5 and out['warmup'] == 2 and out['n_gpus'] == 1
    assert out['unit'] == 'cells/s' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    # five full batches of 1 024 cells (18 000 train rows: the partial batch comes after 17 full ones)
    assert abs(out['value'] - 5 * 1024 / (out['ms_per_step'] * 5e-3)) < 1e-6 * out['value']
    for k in ('roofline', 'kernels', 'batch32', 'epoch', 'cpu_baseline'):
        assert out[k] is None, k
    files = sorted(os.listdir(d))
    assert 'loss.npy' in files and 'W0.npy' in files and 'grad_W0.npy' in files
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64e6
    for f in files:
        a = np.load(os.path.join(d, f))
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
    assert np.load(os.path.join(d, 'loss.npy'))[0] == np.float32(out['loss_last'])


def test_full_run_keeps_every_figure():
    out = _bench('--steps', '5', '--warmup', '2', '--full', '--cpu-seconds', '2')
    assert out['steps'] == 5
    assert out['roofline'] is not None and out['kernels']
    assert out['batch32'] is not None and 'ms_per_step' in out['batch32']
    assert out['epoch'] is not None and out['epoch']['timed_epochs'] == 3
    assert out['cpu_baseline'] is not None and out['cpu_baseline']['value'] > 0
