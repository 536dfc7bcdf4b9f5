"""Every kernel form behind dcahip_zinb_nll against the fp64 oracle (oracle/zinb_np.py), through HipOps / the C ABI, on the
cases of tests/_zinb_nll_cases.py (whose host half, tests/test_zinb_nll_cases_cpu.py, shows that each case reaches the form
named here and walks the rows / fills the queue it was written for).

Which test reaches which instantiation (P = HAS_PI, C = CONST_DISP; flags 1, 0, 3, 2 give every (P, C)):
    zinb_nll_rows_kernel<P, C, 0>            test_vector_form: the gradient call of every case (deep_vec: 2 or 3 rows per
                                             workgroup; its gradients serve as the comparison value of the loss only)
    zinb_nll_compact_kernel<P, C>            test_vector_form: the loss-only call -- deep_vec walks 2 or 3 rows per workgroup
                                             through the look-ahead, clamped at the batch end for some workgroups only, with a
                                             queue remainder of 0, 1 and 63 carried into rows that push 256 more (319 of the 320
                                             entries) and a last flush over entries of several rows; also the loss-only calls of
                                             the ldd / d_* triggers in test_scalar_form, which leave the vector form on
    zinb_nll_kernel<P, C, true, 1>           test_scalar_form, gradient call: deep_scalar (2 or 3 rows per workgroup, gathered),
    zinb_nll_kernel<P, C, false, 1>          edge, tiny with lda % 4 != 0 for every flag; each other trigger alone (ldy, ldd, every
                                             misaligned pointer, theta_w included) on tiny_5x6 and edge; and the loss-only call
    zinb_nll_kernel<0, 0, GRAD, V, LOSS>     test_poisson_mse: LOSS = 1, 2 x GRAD x V = 4, 1 on tiny, deep_scalar and deep_vec's
                                             (1400, 2050); test_scalar_form: the triggers a_mean, y, d_mean, ldy, ldd
    zinb_nll_kernel<P, C, true, 4>           NOT reached: launched only when B * ldd >= 2^32, more than 16 GB of gradient planes

Gradients are held per element to 2e-4 |ref64| + min(2e-6 max |ref64|, 4 R_class) (_zinb_nll_cases.grad_bound); every check
prints, per head and class, the worst err / bound and R_class before it asserts.

Measured on an MI355X (gradients: the worst err / bound over all cases, flags, triggers and classes of the form, with where
it occurred and that class's R_class; nothing needed more than the factor 4, so CLASS_FACTORS is empty):
    zinb_nll_rows_kernel<P, C, 0>           mean 0.0085 (tiny_3x257, flags 3, y != 0, R 8.8e-9), disp 0.044 (tiny_1x1, flags 1,
                                            y != 0, R 1.6e-7), pi 0.44 (edge, flags 1, ridge 0, y = 0.5, R 1.1e-7: the fp32
                                            oracle loses 1 - pi at a_pi = 30, the bound falls back to 2e-6 max |ref|)
    zinb_nll_kernel<P, C, true, 1>          mean 0.0080 (deep_scalar, flags 1, y = 0, R 5.0e-13), disp 0.041 (edge, flags 1,
                                            y = 0.5, R 1.6e-10), pi 0.44 (edge, flags 1, ridge 0, y = 0.5, R 1.1e-7)
    zinb_nll_kernel<0, 0, true, 4 / 1, 1>   mean 0.014 / 0.014 (tiny_3x257, y != 0, R 2.0e-8)
    zinb_nll_kernel<0, 0, true, 4 / 1, 2>   mean 0.00085 / 0.00085 (deep_scalar, y = 0, R 7.3e-12)
    d_theta_w (colsum_chain of d_disp)      0.057 of the project's bound (edge, flags 3), both forms
    loss, relative to the fp64 oracle       rows / compact 2.2e-6 (tiny_1x1: ONE element, a non-zero count through the uncompensated
                                            exp / log of the compacted branch; every other case <= 9.2e-7, edge 1.9e-7 of 3e-5),
                                            V = 1 1.3e-6 (tiny_1x1; edge 4.6e-8), Poisson 2.3e-7, MSE 1.1e-7
    scalar against vector 9.2e-7, loss-only against the gradient call 2.2e-7
The element-wise figures are small because 2e-4 |ref| carries every element whose gradient is not small; the classes' room
4 R_class decides the elements near zero, which the 2e-6 max |ref| term alone used to hide.
"""
import ctypes

import numpy as np
import pytest
import torch

import _zinb_nll_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def call(ops, v):
    """The call of layout v, twice: (loss, partials).  n_partials is gx * gy of the restated grid, the partial slots at and
    beyond it keep their prefill, and the second call gives the same bits."""
    out = []
    for _ in range(2):
        part = torch.full((ops.max_partials,), C.PART_FILL, dtype=torch.float64, device=C.DEVICE)
        n = ops.zinb_nll(*v.args, part)
        loss = torch.zeros(1, device=C.DEVICE)
        ops.loss_finalize(part, n, v.inv_n, loss)
        torch.cuda.synchronize()
        p = part.cpu().numpy()
        assert n == v.grid.n_partials == v.grid.gx * v.grid.gy, (v.kernel, n, v.grid)
        assert (p[n:] == C.PART_FILL).all(), (v.kernel, 'a partial beyond n_partials was written')
        assert np.isfinite(p[:n]).all(), v.kernel
        out.append((loss.item(), p[:n].copy()))
    assert np.array_equal(out[0][1].view(np.int64), out[1][1].view(np.int64)), (v.kernel, 'two calls, different partials')
    assert out[0][0] == out[1][0]
    return out[0]


def check_loss(name, got, want, what):
    rel = abs(got - want) / abs(want)
    print('LOSS|%s|%s|rel %.3g of %.3g' % (what, name, rel, C.loss_rtol(name)))
    assert abs(got - want) <= C.loss_rtol(name) * abs(want), (what, name, got, want, rel)


def check_planes(ops, v):
    """After a gradient call: the layout of the three planes, every head with a per-element reference against the bound,
    and under a constant dispersion the column sums of the d_disp plane (dcahip_colsum_chain) against d_theta_w."""
    c, L = v.case, v.layout
    B, G = c.B, c.G
    o = C.oracle(c.name, v.flags, v.ridge)
    failures = []
    for head, k in zip(C.HEADS, C.GRADS):
        flat = v.dflat[k].cpu().numpy()
        off = 1 if k in L.shifted else 0
        n = (B + C.GUARD_ROWS) * L.ldd
        img = flat[off:off + n].reshape(B + C.GUARD_ROWS, L.ldd)
        written, zero = C.expected_writes(v, k)
        outside = np.ones(flat.shape, bool)
        outside[off:off + n] = ~written.reshape(-1)
        # vector form: columns [G, r4(G)) of a written plane are 0; everything beyond them, the spare rows, the words around
        # the view and the planes the flags do not write keep the sentinel.  Scalar form: every column outside [0, G) does
        assert (flat[outside] == C.SENTINEL).all(), (v.kernel, k, 'wrote outside its window', int((flat[outside] != C.SENTINEL).sum()))
        assert (img[zero] == 0).all(), (v.kernel, k, 'padding of the last quad is not 0')
        if k not in v.written:
            continue
        got = img[:B, :G].astype(np.float64)
        assert np.isfinite(got).all(), (v.kernel, k)
        if head not in o.g:
            continue
        rep, bad = C.grad_report(c.name, v.flags, v.ridge, head, got)
        for cls, (cnt, ratio, R) in sorted(rep.items()):
            print('GRAD|%s|%s|flags %d|ridge %g|%s|%s|class %g|n %d|ratio %.3g|R %.3g'
                  % (v.kernel, c.name, v.flags, v.ridge, L.trigger, head, cls, cnt, ratio, R))
        if bad.any():
            ref = o.g[head]
            failures.append((v.kernel, head, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], ref[bad][:5]))
    if v.flags & C.CONST_DISP:
        out = torch.zeros(G, device=C.DEVICE)
        ops.colsum_chain(v.dview['d_disp'], L.ldd, B, G, v.theta_w, out)
        torch.cuda.synchronize()
        ref = o.d_theta_w
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        tol = C.GRAD_RTOL * np.abs(ref) + C.GRAD_CAP * np.abs(ref).max()            # the project's existing bound
        print('DTHETA|%s|%s|flags %d|ridge %g|%s|ratio %.3g' % (v.kernel, c.name, v.flags, v.ridge, L.trigger, float((err / tol).max())))
        if not (err <= tol).all():
            failures.append((v.kernel, 'd_theta_w', int((~(err <= tol)).sum()), np.argwhere(~(err <= tol))[:5].tolist()))
    assert not failures, failures


def run_forms(ops, name, flags, ridge, trigger, planes=True):
    """The gradient call and the loss-only call of one layout: each against the oracle, and against each other.  Returns
    {grad: loss}."""
    o = C.oracle(name, flags, ridge)
    got = {}
    for grad in (True, False):
        v = C.lay_out(name, flags, trigger, grad, ridge)
        scalar = trigger is not None and C.applies(trigger, flags, grad)
        assert v.vec == (not scalar) and v.kernel == C.instantiation(flags, grad, not scalar, v.case.B, v.layout.ldd), v.kernel
        assert grad or (not v.dflat and v.args[15] is None and v.args[16] is None and v.args[17] is None)
        got[grad], _ = call(ops, v)
        check_loss(name, got[grad], o.loss, v.kernel)
        if grad and planes:
            check_planes(ops, v)
    check_loss(name, got[False], got[True], 'loss-only against the gradient call')
    return got


@pytest.mark.parametrize('name,flags,ridge', C.VECTOR_RUNS)
def test_vector_form(ops, name, flags, ridge):
    """zinb_nll_compact_kernel<..> (loss only) and zinb_nll_rows_kernel<.., 0> (gradients) on 16-byte aligned
    operands.  deep_vec's gradients are covered element-wise at the same shape by test_zinb_nll_row_pairs_and_planes and
    test_zinb_planes_h2_gpu.py: here its gradient call gives the loss the loss-only call is compared with."""
    k, g = C.reaches(C.BY_NAME[name].B, C.BY_NAME[name].G, flags, False)
    assert k.startswith('zinb_nll_compact_kernel') and g.V == 4
    run_forms(ops, name, flags, ridge, None, planes=name != 'deep_vec')


@pytest.mark.parametrize('name,flags,ridge,trigger', C.SCALAR_RUNS)
def test_scalar_form(ops, name, flags, ridge, trigger):
    """zinb_nll_kernel<.., V = 1>: one trigger of the `vec` expression at a time.  A trigger in the gradient operands (ldd, d_*)
    turns the vector form off for the gradient call alone: its loss-only call is the compact kernel again.  The same inputs in
    the vector layout: the losses agree to the loss bound, the gradients of both meet the element-wise bound (the sums
    associate differently: no bit equality)."""
    assert C.reaches(C.BY_NAME[name].B, C.BY_NAME[name].G, flags, True, trigger)[1].V == 1
    scalar = run_forms(ops, name, flags, ridge, trigger)
    vector = run_forms(ops, name, flags, ridge, None)
    check_loss(name, scalar[True], vector[True], 'scalar against vector, gradient calls')
    check_loss(name, scalar[False], vector[False], 'scalar against vector, loss-only calls')


@pytest.mark.parametrize('flag,name', C.SIMPLE_RUNS)
def test_poisson_mse(ops, flag, name):
    """zinb_nll_kernel<false, false, GRAD, V, LOSS>: all four (GRAD, V) of each loss; deep_vec is the (1400, 2050) of the
    vector form.  Counts stay below 1e5 (deep_vec's below 1000), where lgamma(y + 1) and with it the fp64 oracle is finite."""
    assert C.inputs(name)['y'].max() < 1e5 and np.isfinite(C.oracle(name, flag).loss)
    vector = run_forms(ops, name, flag, 0.0, C.SIMPLE_TRIGGERS[0])
    scalar = run_forms(ops, name, flag, 0.0, C.SIMPLE_TRIGGERS[1])
    check_loss(name, scalar[True], vector[True], 'scalar against vector, gradient calls')
    check_loss(name, scalar[False], vector[False], 'scalar against vector, loss-only calls')


def test_argument_checks(ops):
    """Return codes only: every refused call returns DCAHIP_EINVAL before any launch (the partials keep their prefill); the
    calls they differ from are accepted."""
    from dca_amd import hip
    L, p = ops.L, hip.ptr
    B, G, ld = 6, 10, 16
    A = [torch.zeros(B, ld, device=C.DEVICE) for _ in range(3)]
    D = [torch.zeros(B, ld, device=C.DEVICE) for _ in range(3)]
    Y, sf, tw = torch.zeros(B, ld, device=C.DEVICE), torch.ones(B, device=C.DEVICE), torch.zeros(ld, device=C.DEVICE)
    part = torch.full((ops.max_partials,), C.PART_FILL, dtype=torch.float64, device=C.DEVICE)
    n = ctypes.c_int(0)

    def rc(flags, a_disp=A[1], a_pi=A[2], theta_w=tw, d=(D[0], D[1], D[2])):
        return L.dcahip_zinb_nll(p(A[0]), p(a_disp), p(a_pi), ld, p(theta_w), p(Y), ld, p(sf), None, None, B, G, 0.0, 1.0 / (B * G),
                                 flags, p(d[0]), p(d[1]), p(d[2]), ld, p(part), ctypes.byref(n), hip.stream())
    for flags in (C.POISSON | C.HAS_PI, C.POISSON | C.CONST_DISP, C.MSE | C.HAS_PI, C.MSE | C.CONST_DISP, C.MSE | 3):
        assert rc(flags) == C.EINVAL, flags
    assert rc(1, a_pi=None) == C.EINVAL and rc(3, a_pi=None) == C.EINVAL                   # a missing a_pi
    assert rc(2, theta_w=None) == C.EINVAL and rc(3, theta_w=None) == C.EINVAL             # ... theta_w
    assert rc(0, a_disp=None) == C.EINVAL and rc(1, a_disp=None) == C.EINVAL               # ... a_disp
    assert rc(0, d=(D[0], None, None)) == C.EINVAL and rc(2, d=(D[0], None, D[2])) == C.EINVAL      # gradients without d_disp
    assert rc(1, d=(D[0], D[1], None)) == C.EINVAL and rc(3, d=(D[0], D[1], None)) == C.EINVAL      # ... without d_pi
    torch.cuda.synchronize()
    assert (part == C.PART_FILL).all(), 'a refused call launched'
    # what they differ from: accepted (an operand the flags do not read may be missing)
    assert rc(1) == 0 and rc(0, a_pi=None, d=(D[0], D[1], None)) == 0 and rc(2, a_disp=None, a_pi=None) == 0
    assert rc(C.POISSON, a_disp=None, a_pi=None, theta_w=None, d=(D[0], None, None)) == 0
    assert rc(C.MSE, a_disp=None, a_pi=None, theta_w=None, d=(None, None, None)) == 0
    assert rc(3, a_disp=None, d=(None, None, None)) == 0
    torch.cuda.synchronize()
