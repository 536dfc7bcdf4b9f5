"""bench.py's command line and its output dump (bench.dump_outputs) on a stand-in engine: no GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


class _StandIn:
    """What dump_outputs reads of an Engine: named parameters, named gradients, the flat gradient with the loss at P."""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.params = {'W0': rng.standard_normal((300, 16)).astype(np.float32),
                       'b0': rng.standard_normal(16).astype(np.float32),
                       'mm0': rng.standard_normal(16).astype(np.float32)}
        self.grads = {'W0': rng.standard_normal((300, 16)).astype(np.float32),
                      'b0': rng.standard_normal(16).astype(np.float32)}
        self.lay = SimpleNamespace(P=300 * 16 + 16)
        self.g = torch.zeros(self.lay.P + 4)
        self.g[self.lay.P] = 2.5

    def get_params(self):
        return {k: v.copy() for k, v in self.params.items()}

    def get_grads(self):
        return {k: v.copy() for k, v in self.grads.items()}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_parse_defaults_are_the_plain_run(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '3'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.gpus == 1
    assert a.full is False and a.dump_outputs == ''
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'out'


def test_dump_outputs_writes_every_array_in_float32(tmp_path):
    eng = _StandIn()
    bench.dump_outputs(eng, str(tmp_path / 'o'))
    got = _load(str(tmp_path / 'o'))
    assert sorted(got) == ['W0', 'b0', 'grad_W0', 'grad_b0', 'loss', 'mm0']
    for k, v in got.items():
        assert v.dtype == np.float32, k
    for k, v in eng.params.items():
        np.testing.assert_array_equal(got[k], v)
    for k, v in eng.grads.items():
        np.testing.assert_array_equal(got['grad_' + k], v)
    np.testing.assert_array_equal(got['loss'], np.float32([2.5]))


def test_dump_outputs_samples_above_the_limit_the_same_way_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 8000)
    for d in ('a', 'b'):
        bench.dump_outputs(_StandIn(), str(tmp_path / d))
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sorted(a) == sorted(b)
    assert sum(v.nbytes for v in a.values()) <= 8000
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # a sample holds elements of the array, in index order
    full = _StandIn().params['W0'].reshape(-1)
    assert 0 < a['W0'].size < full.size
    pos = np.array([np.flatnonzero(full == x)[0] for x in a['W0']])
    assert (np.diff(pos) > 0).all()
