"""The judge the kernel-level GPU tests share (test_stack_kernels_gpu.py, test_layer_kernels_gpu.py): the flat elementwise
classes EL and the worst error / bound table that is printed before anything is asserted."""
import numpy as np

import _stack_ref as SR

EL = {'H': (2e-5, 2e-5), 'Z': (2e-5, 2e-5), 'xhat': (2e-5, 2e-5), 'inv_std': (1e-5, 0.0), 'mm': (1e-5, 1e-6), 'mv': (1e-5, 1e-6)}


class Judge:
    """Worst error / bound per output class; failures are collected so that the table is printed before the assertion."""

    def __init__(self, title):
        self.title, self.worst, self.fail = title, {}, []

    def _note(self, cls, what, ratio):
        ratio = float(ratio)
        if not ratio <= self.worst.get(cls, (-1.0, ''))[0]:
            self.worst[cls] = (ratio, what)
        if not ratio <= 1.0:
            self.fail.append((cls, what, ratio))

    def elem(self, cls, what, got, ref):
        rtol, atol = EL[cls]
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if got.size:
            self._note(cls, what, (np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())

    def bound(self, cls, what, err, bnd):
        err, bnd = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bnd, np.float64))
        if err.size:
            self._note(cls, what, (err / (bnd + 1e-30)).max())

    def red(self, cls, what, o, name, got):
        got = np.asarray(got, np.float64)
        assert got.shape == o[name].shape, (what, got.shape, o[name].shape)
        err, bnd = SR.error_and_bound(o, name, got)
        self.bound(cls, what, err, bnd)

    def true(self, what, ok):
        if not ok:
            self.fail.append(('exact', what, float('inf')))

    def report(self):
        print('\n%s: worst error / bound  ' % self.title +
              '  '.join('%s %.3g' % (k, v[0]) for k, v in sorted(self.worst.items())))
        assert not self.fail, (self.title, len(self.fail), self.fail[:6])
