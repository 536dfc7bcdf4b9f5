"""K-OPT and the fused step end, one kernel call at a time against the fp64 oracle: cases shared by the GPU suite (HipOps)
and the CPU suite (the oracle-backed ops object, which validates the case logic itself without a GPU).

Reference: oracle.net_np.optimizer_update / nadam_mu in fp64, fed the fp32 values the kernel reads.  Every step is checked
on its own: the state before the call is read back, the oracle advances that state by one step, the kernel's result is
compared with it.  The sizes are the smallest that leave the first grid pass (grid caps: 4096 x 256 elements for
dcahip_optimizer_step / dcahip_nadam_step, 2048 x 256 float4 for dcahip_rmsprop_clip*), are no multiple of 256 or 4, and
end in a partial second pass.

The bound on a parameter is relative to its UPDATE, not to the parameter:
    |w - w_ref| <= 2^-23 |w_ref| + TOL |w_ref - w_prev|            (the first term: the rounding of the stored result)
and on a slot s (accumulators, moments) relative to what entered it:
    |s - s_ref| <= TOL (|s_ref| + |s_ref - s_prev|)
TOL is not chosen: `f32_update` below restates the kernels' arithmetic in numpy float32 (same operation order, every
intermediate rounded, no fused multiply-add), runs on the same inputs and is measured against the fp64 oracle with
`measure_f32`; TOL = 4 x its worst relative error, the margin covering sqrtf / pow / the division differing by an ulp
between the host's libm and the device, and fused multiply-adds.  Measured on these inputs (seed 7, three steps each;
relative error of the update | of the slots):
    sgd 5.9e-08 | -            adagrad 2.0e-07 | 6.0e-08    adadelta 1.3e-07 | 2.4e-07    adam 2.5e-07 | 1.3e-07
    adamax 2.2e-07 | 1.3e-07   nadam 2.6e-07 | 1.3e-07      rmsprop (B2's inputs) 2.4e-07 | 1.9e-07
    worst 2.56e-07  ->  TOL = 1.03e-06, the tolerance class of test_kernels_gpu.py::test_rmsprop_clip (1e-6), here on the update
(tests/test_opt_kernels_cpu.py::test_tol_is_four_times_the_measured_fp32_error repeats the measurement and holds TOL to it.)

The gradients of one element keep their sign over the three steps.  With momentum (Adam, Adamax, Nadam) a gradient against
the accumulated moment cancels in m = b1 m + (1 - b1) g, and the update's relative error is then the cancellation's
amplification -- unbounded over a million random elements -- which would leave the measured TOL saying nothing.  The
formulas are the same for either sign; the slots' bound above holds with mixed signs too.
"""
import numpy as np
import torch

from oracle import net_np as N

TOL = 1.03e-6
EPS32 = 2.0 ** -23
CLIP = 5.0
PAD = 64                                  # elements allocated past n: must keep the sentinel
SENTINEL = -777.25
N_OPT = 4096 * 256 + 3 * 256 + 3          # K-OPT: a partial second pass of the grid-stride loop, n % 4 = 3
N_RMS = 2048 * 256 * 4 + 4 * 256 + 3      # RMSprop: a partial second float4 pass and the 3-element scalar tail
KINDS = ('sgd', 'adagrad', 'adadelta', 'adam', 'adamax', 'nadam')
LRS = (1e-3, 1e-3, 2.5e-4)                # the device word changes between steps 2 and 3 (ReduceLROnPlateau)


# ------------------------------------------------------------------ plumbing
def _dev(ops):
    return torch.device(ops.device_type)


def _t(ops, a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(_dev(ops))


def _sync(ops):
    if ops.device_type == 'cuda':
        torch.cuda.synchronize()


def _padded(ops, a):
    """a [n] fp32 -> a device buffer of n + PAD elements, the tail holding the sentinel."""
    buf = np.full(a.size + PAD, SENTINEL, np.float32)
    buf[:a.size] = a
    return _t(ops, buf)


def _host(t, n):
    return t[:n].cpu().numpy().copy()


def _tail_kept(t, n):
    return bool((t[n:].cpu().numpy() == np.float32(SENTINEL)).all())


# ------------------------------------------------------------------ inputs
def opt_inputs(n, seed=7):
    """w: a third exactly 0 (step 1 then shows -lr u without the weight's own rounding), the rest N(0, 1e-2).
    g[k], k = 0..2: N(0, 4) with a fixed sign per element (module docstring), so clip = 5 bites; exact zeros, +-5, 7.5, -9
    and a block of 1e-9-scale values (where epsilon's placement decides the result) in the first pass, in the second
    pass and at the very end."""
    rng = np.random.RandomState(seed)
    w = rng.normal(0, 1e-2, n).astype(np.float32)
    w[::3] = 0.0
    sign = np.where(rng.random_sample(n) < 0.5, -1.0, 1.0)
    gs = []
    for k in range(3):
        g = (sign * np.abs(rng.normal(0, 4, n))).astype(np.float32)
        for at in (0, 4096 * 256 + 200):
            g[at:at + 6] = [0.0, 5.0, -5.0, 7.5, -9.0, 0.0]
            g[at + 16:at + 272] = (sign[at + 16:at + 272] * np.abs(rng.normal(0, 1e-9, 256))).astype(np.float32)
            g[at + 300:at + 340] = 0.0
        g[n - 3:] = [7.5, -9.0, 1e-9]
        gs.append(g)
    return w, gs


def rms_inputs(n, seed=1):
    """The inputs of test_kernels_gpu.py::test_rmsprop_clip at stride scale: accumulators far below epsilon (where its
    placement matters) in the first pass, in the second and in the scalar tail."""
    rng = np.random.RandomState(seed)
    w = rng.normal(0, 1, n).astype(np.float32)
    g = rng.normal(0, 4, n).astype(np.float32)
    ms = rng.uniform(0, 1, n).astype(np.float32)
    for at in (5, 2048 * 256 * 4 + 100):
        if at + 395 <= n:
            ms[at:at + 395] *= 1e-12
            g[at:at + 395] *= 1e-6
    g[:5] = [0, 1e-9, 7.5, -9, 5.0]
    g[n - 3:] = [-7.5, 1e-9, 0.25]
    ms[n - 2] = 1e-13
    return w, g, ms


# ------------------------------------------------------------------ fp32 restatement of the kernels (the basis of TOL)
def f32_update(kind, w, g, a, b, lr, t, clip, p_prev=1.0, rho=0.9, eps=1e-7):
    """dcahip_opt.hip (opt_one, nadam_kernel) and rmsprop_clip_kernel in numpy float32: same operation order, every
    intermediate rounded to fp32.  Returns (w, a, b, m_schedule)."""
    f = np.float32
    g = g.astype(f)
    if clip > 0:
        g = np.minimum(np.maximum(g, f(-clip)), f(clip))
    lr = f(lr)
    e = f(eps)
    c2 = f(1.0 / (1.0 - 0.9 ** t))
    c1 = f(np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    if kind == 'sgd':
        return w - lr * g, a, b, None
    if kind == 'rmsprop':
        a = f(rho) * a + (f(1) - f(rho)) * g * g
        return w - lr * g / (np.sqrt(a) + e), a, b, None
    if kind == 'adagrad':
        a = a + g * g
        return w - lr * g / (np.sqrt(a) + e), a, b, None
    if kind == 'adadelta':
        a = f(0.95) * a + f(0.05) * g * g
        u = g * np.sqrt(b + e) / np.sqrt(a + e)
        b = f(0.95) * b + f(0.05) * u * u
        return w - lr * u, a, b, None
    if kind == 'adam':
        a = f(0.9) * a + f(0.1) * g
        b = f(0.999) * b + f(0.001) * g * g
        return w - lr * c1 * a / (np.sqrt(b) + e), a, b, None
    if kind == 'adamax':
        a = f(0.9) * a + f(0.1) * g
        b = np.maximum(f(0.999) * b, np.abs(g))
        return w - lr * c2 * a / (b + e), a, b, None
    assert kind == 'nadam'
    mu_t, mu_t1 = f(N.nadam_mu(t)), f(N.nadam_mu(t + 1))
    p_new = f(p_prev) * mu_t
    p_next = p_new * mu_t1
    vden = f(1.0 - 0.999 ** t)
    gp = g / (f(1) - p_new)
    a = f(0.9) * a + f(0.1) * g
    b = f(0.999) * b + f(0.001) * g * g
    mbar = (f(1) - mu_t) * gp + mu_t1 * (a / (f(1) - p_next))
    return w - lr * mbar / (np.sqrt(b / vden) + e), a, b, p_new


def rel_errors(w, w_ref, w_prev, slots):
    """(worst error of w in units of its update after the stored result's own rounding, worst error of a slot in units of
    |s_ref| + |s_ref - s_prev|).  slots: (got, ref, prev) triples."""
    w, w_ref, w_prev = (np.asarray(x, np.float64) for x in (w, w_ref, w_prev))
    excess = np.maximum(np.abs(w - w_ref) - EPS32 * np.abs(w_ref), 0.0)
    upd = np.abs(w_ref - w_prev)
    moved = upd > 0
    assert not excess[~moved].any(), 'an element without an update moved'
    ew = float((excess[moved] / upd[moved]).max()) if moved.any() else 0.0
    es = 0.0
    for s, s_ref, s_prev in slots:
        s, s_ref, s_prev = (np.asarray(x, np.float64) for x in (s, s_ref, s_prev))
        den = np.abs(s_ref) + np.abs(s_ref - s_prev)
        err = np.abs(s - s_ref)
        assert not err[den == 0].any(), 'a slot without input moved'
        if (den > 0).any():
            es = max(es, float((err[den > 0] / den[den > 0]).max()))
    return ew, es


def assert_step_close(what, w, w_ref, w_prev, slots, tol=TOL):
    ew, es = rel_errors(w, w_ref, w_prev, slots)
    assert ew <= tol, (what, 'w', ew, tol)
    assert es <= tol, (what, 'slot', es, tol)
    return ew, es


def _ref_step(kind, w, g, a, b, lr, t):
    f = lambda x: None if x is None else x.astype(np.float64)
    return N.optimizer_update(kind, f(w), f(g), f(a), f(b), float(lr), t, CLIP)


def measure_f32():
    """{kind: (update error, slot error)} of the fp32 restatement against the fp64 oracle on the cases' own inputs."""
    out = {}
    w0, gs = opt_inputs(N_OPT)
    for kind in KINDS:
        w = w0.copy()
        a = None if kind == 'sgd' else np.full(N_OPT, 0.1 if kind == 'adagrad' else 0.0, np.float32)
        b = None if kind in ('sgd', 'adagrad') else np.zeros(N_OPT, np.float32)
        p = 1.0
        ew = es = 0.0
        for k in range(3):
            lr = np.float32(LRS[k])
            if kind == 'nadam':                     # the oracle's running product is exact; the kernel's is this fp32 word
                rw, ra, rb = _nadam_ref(w, gs[k], a, b, lr, k + 1, p)
            else:
                rw, ra, rb = _ref_step(kind, w, gs[k], a, b, lr, k + 1)
            nw, na, nb, np_ = f32_update(kind, w, gs[k], a, b, lr, k + 1, CLIP, p)
            e1, e2 = rel_errors(nw, rw, w, [(x, y, z) for x, y, z in ((na, ra, a), (nb, rb, b)) if x is not None])
            ew, es = max(ew, e1), max(es, e2)
            w, a, b = nw, na, nb
            p = np_ if np_ is not None else p
        out[kind] = (ew, es)
    w, g, ms = rms_inputs(N_RMS)
    rw, ra, _ = _ref_step('rmsprop', w, g, ms, None, np.float32(1e-3), 1)
    nw, na, _, _ = f32_update('rmsprop', w, g, ms, None, np.float32(1e-3), 1, CLIP)
    out['rmsprop'] = rel_errors(nw, rw, w, [(na, ra, ms)])
    return out


def _nadam_ref(w, g, a, b, lr, t, p_prev):
    """optimizer_update('nadam') continued from the running product the kernel reads (an fp32 device word) instead of the
    exact product: the same formula, so a step is judged on the state it was given."""
    f = lambda x: x.astype(np.float64)
    w, g, a, b = f(w), np.clip(f(g), -CLIP, CLIP), f(a), f(b)
    mu_t, mu_t1 = N.nadam_mu(t), N.nadam_mu(t + 1)
    p_new = float(p_prev) * mu_t
    p_next = p_new * mu_t1
    gp = g / (1.0 - p_new)
    a = 0.9 * a + 0.1 * g
    b = 0.999 * b + 0.001 * g * g
    mbar = (1.0 - mu_t) * gp + mu_t1 * a / (1.0 - p_next)
    return w - float(lr) * mbar / (np.sqrt(b / (1.0 - 0.999 ** t)) + 1e-7), a, b


# ------------------------------------------------------------------ B1
def optimizer_three_steps(ops, kind):
    """Three consecutive steps of one optimizer at stride scale; returns the worst (update, slot) errors seen."""
    n = N_OPT
    w0, gs = opt_inputs(n)
    w = _padded(ops, w0)
    s1 = None if kind == 'sgd' else _padded(ops, np.full(n, 0.1 if kind == 'adagrad' else 0.0, np.float32))
    s2 = None if kind in ('sgd', 'adagrad') else _padded(ops, np.zeros(n, np.float32))
    it = torch.zeros(1, dtype=torch.int64, device=_dev(ops))
    lr = torch.tensor([LRS[0]], dtype=torch.float32, device=_dev(ops))
    msch = torch.ones(1, dtype=torch.float32, device=_dev(ops))
    prod = 1.0
    worst = (0.0, 0.0)
    for k in range(3):
        t = k + 1
        lr.fill_(LRS[k])
        g = _padded(ops, gs[k])
        _sync(ops)
        lrv = float(lr.item())
        pw = _host(w, n)
        pa = None if s1 is None else _host(s1, n)
        pb = None if s2 is None else _host(s2, n)
        if kind == 'nadam':
            p_prev = float(msch.item())
            rw, ra, rb = _nadam_ref(pw, gs[k], pa, pb, lrv, t, p_prev)
            ops.nadam_step(w, g, s1, s2, n, lr, it, msch, CLIP)
        else:
            rw, ra, rb = _ref_step(kind, pw, gs[k], pa, pb, lrv, t)
            ops.optimizer_step(kind, w, g, s1, s2, n, lr, it, CLIP)
        _sync(ops)
        slots = [(_host(s, n), r, p) for s, r, p in ((s1, ra, pa), (s2, rb, pb)) if s is not None]
        worst = tuple(max(x, y) for x, y in zip(worst, assert_step_close((kind, t), _host(w, n), rw, pw, slots)))
        if k == 0:
            # w = 0 exactly: the first step is -lr u alone, so the stored value carries the update's error and nothing else
            z = pw == 0
            assert z.any() and (np.abs(_host(w, n)[z] - rw[z]) <= (EPS32 + TOL) * np.abs(rw[z])).all()
        for buf in (w, s1, s2):
            assert buf is None or _tail_kept(buf, n), (kind, t, 'wrote past n')
        assert np.array_equal(_host(g, n), gs[k]) and _tail_kept(g, n)
        assert int(it.item()) == k, 'the step itself must not advance *iter'
        if kind == 'nadam':
            prod *= N.nadam_mu(t)
            got = float(msch.item())
            assert abs(got - prod) <= TOL * prod, (t, got, prod)
        ops.counter_add(it, 1)
        _sync(ops)
        assert int(it.item()) == t
    return worst


def counter_add_cases(ops):
    c = torch.tensor([2 ** 40 + 5, -9], dtype=torch.int64, device=_dev(ops))      # 64-bit; the neighbour stays
    ops.counter_add(c, 3)
    ops.counter_add(c, -10)
    _sync(ops)
    assert c.cpu().tolist() == [2 ** 40 - 2, -9]


# ------------------------------------------------------------------ B2
def rmsprop_stride(ops):
    """dcahip_rmsprop_clip at stride scale against fp64 with the update-relative bound, and the same entry with its step-end arguments:
    w, ms bit-identical to it, the bookkeeping bit-identical to dcahip_step_end on the same words, two calls running."""
    n = N_RMS
    w0, g0, ms0 = rms_inputs(n)
    lr = torch.tensor([1e-3], dtype=torch.float32, device=_dev(ops))
    lrv = float(lr.item())
    g = _padded(ops, g0)
    w, ms = _padded(ops, w0), _padded(ops, ms0)
    ops.rmsprop_clip(w, g, ms, n, lr, 0.9, 1e-7, CLIP)
    _sync(ops)
    rw, rms, _ = _ref_step('rmsprop', w0, g0, ms0, None, lrv, 1)
    worst = assert_step_close('rmsprop', _host(w, n), rw, w0, [(_host(ms, n), rms, ms0)])
    assert _tail_kept(w, n) and _tail_kept(ms, n) and _tail_kept(g, n)
    # second step of the plain kernel, then both steps again through the fused one
    ops.rmsprop_clip(w, g, ms, n, lr, 0.9, 1e-7, CLIP)
    we, mse = _padded(ops, w0), _padded(ops, ms0)
    d = _dev(ops)
    words = lambda: (torch.tensor([2.5], dtype=torch.float32, device=d), torch.zeros(8, dtype=torch.float32, device=d),
                     torch.tensor([1.5], dtype=torch.float64, device=d), torch.tensor([64], dtype=torch.int64, device=d))
    loss, hist, acc, cur = words()
    rloss, rhist, racc, rcur = words()
    for val, weight, adv in ((2.5, 32.0, 32), (0.1, 7.0, 7)):      # 0.1f * 7: the product must be formed in fp64
        loss.fill_(val); rloss.fill_(val)
        ops.rmsprop_clip_end(we, g, mse, n, lr, 0.9, 1e-7, CLIP, loss, weight, hist, 32, acc, cur, adv)
        ops.step_end(rloss, weight, rhist, 32, racc, rcur, adv)
    _sync(ops)
    assert torch.equal(we, w) and torch.equal(mse, ms)
    assert torch.equal(hist, rhist) and torch.equal(acc, racc) and torch.equal(cur, rcur)
    # the slot comes from the cursor BEFORE the advance: 64 / 32 = 2, then 96 / 32 = 3
    l2 = float(np.float32(0.1))
    assert hist.cpu().tolist() == [0, 0, 2.5, l2, 0, 0, 0, 0] and cur.item() == 103
    assert acc.item() == 1.5 + 2.5 * 32.0 + l2 * 7.0
    return worst


def rmsprop_end_null_words(ops):
    """loss, hist, acc and cursor may each be NULL independently: the others behave as dcahip_step_end's."""
    n = 1027
    w0, g0, ms0 = (x[:n].copy() for x in rms_inputs(4096))
    d = _dev(ops)
    lr = torch.tensor([1e-3], dtype=torch.float32, device=d)
    g = _t(ops, g0)
    wp, msp = _t(ops, w0), _t(ops, ms0)
    ops.rmsprop_clip(wp, g, msp, n, lr, 0.9, 1e-7, CLIP)
    for drop in ('loss', 'hist', 'acc', 'cursor', 'all'):
        def words():
            v = dict(loss=torch.tensor([0.3], dtype=torch.float32, device=d), hist=torch.full((4,), -1.0, device=d),
                     acc=torch.tensor([0.25], dtype=torch.float64, device=d),
                     cursor=torch.tensor([5], dtype=torch.int64, device=d))
            for k in v:
                if drop in (k, 'all'):
                    v[k] = None
            return v
        a, r = words(), words()
        w, ms = _t(ops, w0), _t(ops, ms0)
        ops.rmsprop_clip_end(w, g, ms, n, lr, 0.9, 1e-7, CLIP, a['loss'], 3.0, a['hist'], 2, a['acc'], a['cursor'], 2)
        ops.step_end(r['loss'], 3.0, r['hist'], 2, r['acc'], r['cursor'], 2)
        _sync(ops)
        assert torch.equal(w, wp) and torch.equal(ms, msp), drop
        for k in a:
            assert (a[k] is None and r[k] is None) or torch.equal(a[k], r[k]), (drop, k)
        if drop == 'cursor':
            assert a['hist'].cpu().tolist() == [np.float32(0.3), -1, -1, -1]          # no cursor: slot 0
        if drop == 'loss':
            assert a['hist'].cpu().tolist() == [-1] * 4 and a['acc'].item() == 0.25 and a['cursor'].item() == 7
        if drop not in ('cursor', 'loss', 'hist', 'all'):
            assert a['hist'].cpu().tolist() == [-1, -1, np.float32(0.3), -1]          # 5 / 2 = 2


# ------------------------------------------------------------------ B3
L1L2_N = 120000
L1L2_SEGS = [
    (3, 40006, 1e-3, 2e-3),            # 40 003 elements from an unaligned start: more than 64 x 256, the stride loop runs
    (40006, 40011, 5e-4, 1e-4),        # 5 elements: 63 of the 64 workgroups add nothing
    (40011, 50000, 1e-3, 0.0),         # l1 only
    (50001, 61000, 0.0, 2e-3),         # l2 only (element 50000: a gap between segments)
    (61000, 70000, 0.0, 0.0),          # both coefficients 0: launches nothing, takes no partial slot
    (70000, 70000, 1e-3, 1e-3),        # empty
    (70001, 70300, 2e-3, 0.0),
    (71000, 71001, 1e-3, 1e-3),        # one element
    (72000, 72999, 0.0, 0.0),          # a second skipped one between used ones
    (73000, 74025, 1e-4, 5e-3),
    (80000, 80257, 3e-3, 1e-3),
    (81000, 81000, 0.0, 0.0),
    (82001, 90000, 0.0, 1e-2),
    (90000, 100000, 1e-2, 0.0),
    (100003, 100004, 0.0, 1.0),
    (110000, 120000, 1e-3, 1e-3),      # up to the buffer's last element
]


def l1l2_inputs(seed=3):
    rng = np.random.RandomState(seed)
    w = rng.normal(0, 0.05, L1L2_N).astype(np.float32)
    w[::7] = 0.0                                        # sign(0) = 0
    w[5:40] = -np.abs(w[5:40]) - np.float32(1e-3)
    g = rng.normal(0, 1, L1L2_N).astype(np.float32)
    g[100:200] = 0.0                                    # the penalty's gradient alone
    g[40006:40011] *= 1e-3                              # of the gradient's own size
    return w, g


def l1l2_reference(w, g, loss_in):
    """g_ref in fp64, the bound on it (1 fp32 ulp -- 2^-23 relative -- of the sum's larger term), the mask of elements
    inside a used segment, and the loss: float(loss_in + sum over fp32-rounded terms), as the kernel forms them."""
    f = np.float32
    gref = g.astype(np.float64)
    bound = np.zeros(w.size)
    inside = np.zeros(w.size, bool)
    pen = 0.0
    for a, b, l1, l2 in L1L2_SEGS:
        if b <= a or (l1 == 0 and l2 == 0):
            continue
        x = w[a:b]
        t = f(l1) * np.sign(x).astype(np.float64) + 2.0 * f(l2) * x.astype(np.float64)
        gref[a:b] += t
        bound[a:b] = EPS32 * np.maximum(np.abs(g[a:b].astype(np.float64)), np.abs(t))
        inside[a:b] = True
        pen += float((f(l1) * np.abs(x)).astype(np.float64).sum()) + float(((f(l2) * x) * x).astype(np.float64).sum())
    return gref, bound, inside, float(f(loss_in + pen)), pen


def l1l2_cases(ops):
    w0, g0 = l1l2_inputs()
    loss_in = 3.25
    gref, bound, inside, loss_ref, pen = l1l2_reference(w0, g0, loss_in)
    assert pen > 0.05 * loss_in                        # the penalty is no rounding error of the loss it joins
    assert len(L1L2_SEGS) == 16
    desc = ops.reg_desc(L1L2_SEGS)
    nws = ops.l1l2_workspace_doubles()
    d = _dev(ops)
    w = _t(ops, w0)

    def run(with_g):
        g = _t(ops, g0) if with_g else None
        loss = torch.tensor([loss_in], dtype=torch.float32, device=d)
        ws = torch.full((nws,), float('nan'), dtype=torch.float64, device=d)    # only this call's slots may be read
        ops.l1l2_apply(desc, w, g, loss, ws)
        _sync(ops)
        return g, loss

    g1, loss1 = run(True)
    got = g1.cpu().numpy()
    err = np.abs(got.astype(np.float64) - gref)
    bad = inside & (err > bound)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].ravel(), got[bad][:5], gref[bad][:5])
    assert np.array_equal(got[~inside].view(np.uint32), g0[~inside].view(np.uint32)), 'g changed outside the segments'
    z = inside & (w0 == 0)
    assert z.any() and np.array_equal(got[z], g0[z])                            # sign(0) = 0 and 2 l2 0 = 0
    assert abs(loss1.item() - loss_ref) <= EPS32 * abs(loss_ref), (loss1.item(), loss_ref)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), w0.view(np.uint32))
    g2, loss2 = run(True)
    assert torch.equal(g1, g2) and torch.equal(loss1, loss2)                    # deterministic
    _, loss3 = run(False)                                                       # validation: g == NULL
    assert torch.equal(loss3, loss1)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), w0.view(np.uint32))
    # nothing to add: the loss word is left alone, the workspace is not read
    none = ops.reg_desc([(0, 100, 0.0, 0.0), (50, 50, 1.0, 1.0)])
    g = _t(ops, g0)
    loss = torch.tensor([loss_in], dtype=torch.float32, device=d)
    ops.l1l2_apply(none, w, g, loss, torch.full((nws,), float('nan'), dtype=torch.float64, device=d))
    _sync(ops)
    assert loss.item() == loss_in and np.array_equal(g.cpu().numpy(), g0)
    # no loss word: the gradient is still regularised
    g = _t(ops, g0)
    ops.l1l2_apply(desc, w, g, None, torch.full((nws,), float('nan'), dtype=torch.float64, device=d))
    _sync(ops)
    assert torch.equal(g, g1)
