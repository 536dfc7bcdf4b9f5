"""Cases, layouts and references of the tests of the stand-alone likelihood entry point (dcahip_zinb_nll in
dca_amd/csrc/dcahip_zinb.hip): tests/test_zinb_nll_forms_gpu.py runs them on the device, tests/test_zinb_nll_cases_cpu.py
checks on the host that every case reaches the kernel form it was written for and that the references are what the device
tests take them for.

Host arithmetic restated from dcahip_zinb_nll (grid(), vec_predicate(), instantiation()):
    Gp   = (G + 3) & ~3
    vec  = lda % 4 == 0, ldy % 4 == 0, lda >= Gp, ldy >= Gp, a_mean / y and every other input the flags read 16-byte aligned;
           with gradients also ldd % 4 == 0, ldd >= Gp and every gradient plane the flags write 16-byte aligned
    V    = 4 if vec else 1;  nvec = ceil(G / V);  nseg = ceil(nvec / 256);  gx = min(nseg, 2048);  gy = min(2048 // gx, B)
    a workgroup (x, y) walks the rows y, y + gy, y + 2 gy, ... of gene segment x and writes partial y * gx + x
    NB / ZINB, vec:      gradients -> zinb_nll_rows_kernel<HAS_PI, CONST_DISP, 0>   (B * ldd < 2^32)
                         loss only -> zinb_nll_compact_kernel<HAS_PI, CONST_DISP>
    NB / ZINB, not vec:  zinb_nll_kernel<HAS_PI, CONST_DISP, GRAD, 1>
    Poisson / MSE:       zinb_nll_kernel<false, false, GRAD, V, LOSS>
(zinb_nll_kernel<HAS_PI, CONST_DISP, true, 4> needs B * ldd >= 2^32, more than 16 GB of gradients: no case reaches it.)

A layout (layout_of) gives every operand a buffer of its own with row stride Gp + 4: the vector form, unless exactly one
trigger of TRIGGERS turns it off -- a row stride of Gp + 5, or one operand `shifted`: the [1:] view of a buffer that is one
float longer, seen with the same row stride.  lay_out() puts a layout on the device.

The gradient bound (grad_bound) is per element
    err <= 2e-4 |ref64| + min(2e-6 max |ref64|, factor R_class)
where R_class = max |oracle32 - oracle64| over the elements of the same head and class (the count value on the edge grid,
y == 0 / y != 0 elsewhere) is what an fp32 evaluation of the reference's own formulas loses in that class -- measured against
the reference, never against a kernel.  factor is RCLASS_FACTOR unless CLASS_FACTORS names the class.
"""
import collections
import types

import numpy as np

from oracle import zinb_np as Z
import _zinb_edge_grid as E

HAS_PI, CONST_DISP, POISSON, MSE = 1, 2, 4, 8
EINVAL = -22
DEVICE = 'cuda'
GRID_CAP = 2048                           # kMaxPartials
NZ_CAP = 64 + 256                         # kNzCap: entries of a wave's queue in the loss-only compact kernel
SENTINEL = np.float32(-1234.5)            # what every gradient word holds before a call
PART_FILL = -7.0                          # ... and every loss partial
GUARD_ROWS = 2                            # gradient rows at and beyond B that no call may touch
SPARE = 4                                 # columns of every row beyond Gp
STORE_EXTRA, CURSOR = 7, 3                # gathered calls: a storage of B + 7 rows, read from perm[3] on
LOSS_RTOL, LOSS_RTOL_EDGE = 3e-6, 3e-5    # test_kernels_gpu.py::test_zinb_nll_vs_oracle states and explains both
GRAD_RTOL, GRAD_CAP = 2e-4, 2e-6          # the project's gradient bound: 2e-4 |ref| + 2e-6 max |ref|
RCLASS_FACTOR = 4.0
CLASS_FACTORS = {}                        # (head, class) -> factor, each with its cause beside it; empty: none needed

HEADS = ('mean', 'disp', 'pi')
INPUTS = ('a_mean', 'a_disp', 'a_pi', 'y', 'theta_w')
GRADS = ('d_mean', 'd_disp', 'd_pi')
TRIGGERS = ('lda', 'ldy', 'ldd') + INPUTS + GRADS

Grid = collections.namedtuple('Grid', 'V nvec nseg gx gy n_partials rows_min rows_max n_long last')
Layout = collections.namedtuple('Layout', 'trigger G Gp lda ldy ldd shifted')
Case = collections.namedtuple('Case', 'name B G gather')


def r4(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------------------------------------- host arithmetic
def grid(B, G, V):
    """The launch of dcahip_zinb_nll.  rows_min / rows_max: the fewest / most rows a workgroup walks, n_long: how many
    blockIdx.y walk rows_max; last: the active lanes of the last gene segment."""
    nvec = -(-G // V)
    nseg = -(-nvec // 256)
    gx = min(nseg, GRID_CAP)
    gy = max(1, min(GRID_CAP // gx, B))
    rows = [len(range(y, B, gy)) for y in range(gy)]
    return Grid(V, nvec, nseg, gx, gy, gx * gy, min(rows), max(rows), rows.count(max(rows)), nvec - (nseg - 1) * 256)


def loss_kind(flags):
    return 1 if flags & POISSON else (2 if flags & MSE else 0)


def operands(flags, grad):
    """The operands the entry point reads / writes under `flags` (every other one is NULL or not looked at)."""
    loss = loss_kind(flags)
    ops = ['a_mean', 'y']
    if loss == 0:
        ops.append('theta_w' if flags & CONST_DISP else 'a_disp')
    if flags & HAS_PI:
        ops.append('a_pi')
    if grad:
        ops.append('d_mean')
        if loss == 0:
            ops.append('d_disp')
        if flags & HAS_PI:
            ops.append('d_pi')
    return tuple(ops)


def vec_predicate(G, flags, grad, lda, ldy, ldd, misaligned=()):
    """The `vec` expression of dcahip_zinb_nll, term by term; `misaligned`: the operands whose pointer is not 16-byte
    aligned."""
    has_pi, cdisp, loss = bool(flags & HAS_PI), bool(flags & CONST_DISP), loss_kind(flags)
    Gp = r4(G)
    al = lambda name: name not in misaligned                               # noqa: E731
    vec = (lda % 4 == 0 and ldy % 4 == 0 and al('a_mean') and al('y')
           and (loss != 0 or (al('theta_w') if cdisp else al('a_disp'))) and (not has_pi or al('a_pi'))
           and lda >= Gp and ldy >= Gp)
    if grad:
        vec = (vec and ldd % 4 == 0 and ldd >= Gp and al('d_mean') and (loss != 0 or al('d_disp'))
               and (not has_pi or al('d_pi')))
    return vec


def instantiation(flags, grad, vec, B=1, ldd=0):
    """The kernel launch_nll / launch_nll_simple choose, as its template name."""
    has_pi, cdisp, loss = int(bool(flags & HAS_PI)), int(bool(flags & CONST_DISP)), loss_kind(flags)
    g = 'true' if grad else 'false'
    if loss:
        return 'zinb_nll_kernel<0,0,%s,%d,%d>' % (g, 4 if vec else 1, loss)
    fits = not grad or B * ldd < 2 ** 32
    if vec and fits and grad:
        return 'zinb_nll_rows_kernel<%d,%d,0>' % (has_pi, cdisp)
    if vec and fits:
        return 'zinb_nll_compact_kernel<%d,%d>' % (has_pi, cdisp)
    return 'zinb_nll_kernel<%d,%d,%s,%d>' % (has_pi, cdisp, g, 4 if vec else 1)


def every_instantiation():
    """Every kernel dcahip_zinb_nll can launch, the 2^32 exception left out."""
    out = set()
    for f in (0, 1, 2, 3):
        out.add(instantiation(f, True, True))
        out.add(instantiation(f, False, True))
        out.add(instantiation(f, True, False))
        out.add(instantiation(f, False, False))
    for f in (POISSON, MSE):
        out |= {instantiation(f, g, v) for g in (True, False) for v in (True, False)}
    return out


def layout_of(G, trigger=None):
    Gp = r4(G)
    ld = Gp + SPARE
    assert trigger is None or trigger in TRIGGERS, trigger
    lds = {k: ld + 1 if trigger == k else ld for k in ('lda', 'ldy', 'ldd')}
    shifted = (trigger,) if trigger in INPUTS + GRADS else ()
    return Layout(trigger, G, Gp, lds['lda'], lds['ldy'], lds['ldd'], shifted)


def applies(trigger, flags, grad):
    """Whether `trigger` touches an operand the call has: a trigger that does not leaves the vector form on."""
    if trigger in (None, 'lda', 'ldy'):
        return True
    if trigger == 'ldd':
        return grad
    return trigger in operands(flags, grad)


def reaches(B, G, flags, grad, trigger=None):
    """(template name, Grid) of the call of a [B, G] batch with the layout of `trigger`."""
    L = layout_of(G, trigger)
    vec = vec_predicate(G, flags, grad, L.lda, L.ldy, L.ldd, L.shifted)
    return instantiation(flags, grad, vec, B, L.ldd), grid(B, G, 4 if vec else 1)


# ----------------------------------------------------------------------------------------------------------- cases
DEEP_K = (0, 1, 63, 64, 65, 255, 256)     # non-zeros per block of 256 genes, cycling by row, in the first grid.y rows
TINY = ((1, 1), (5, 6), (3, 255), (3, 256), (3, 257), (3, 1024), (3, 1025))
CASES = [Case('deep_vec', 1400, 2050, True), Case('deep_scalar', 500, 2050, True), Case('edge', 3, 2880, True)]
CASES += [Case('tiny_%dx%d' % s, s[0], s[1], False) for s in TINY]
BY_NAME = {c.name: c for c in CASES}
TINY_NAMES = tuple(c.name for c in CASES if c.name.startswith('tiny'))
ZINB_FLAGS = (1, 0, 3, 2)


SIMPLE_TRIGGER_SET = ('a_mean', 'y', 'd_mean', 'ldy', 'ldd')       # the triggers whose operand Poisson / MSE have, lda apart


def ridges(name, flags):
    """The ridge values a (case, flags) runs with: the edge grid takes each of its three, where a dropout head exists."""
    if not flags & HAS_PI:
        return (0.0,)
    return E.RIDGES if name == 'edge' else (0.05,)


def _flags_with(trigger):
    return [f for f in ZINB_FLAGS + (POISSON, MSE) if applies(trigger, f, True) and (not loss_kind(f) or trigger in SIMPLE_TRIGGER_SET)]


# what tests/test_zinb_nll_forms_gpu.py runs (tests/test_zinb_nll_cases_cpu.py: together they reach every instantiation)
# test_vector_form: (case, flags, ridge), the loss-only and the gradient call of the aligned layout
VECTOR_RUNS = [(n, f, r) for n in ('deep_vec', 'edge') + TINY_NAMES for f in ZINB_FLAGS for r in ridges(n, f)]
# test_scalar_form: (case, flags, ridge, trigger) -- lda % 4 != 0 for every flag, each other trigger on tiny_5x6 and edge with the
# flags that have its operand
SCALAR_RUNS = [(n, f, r, 'lda') for n in ('deep_scalar', 'edge') + TINY_NAMES for f in ZINB_FLAGS for r in ridges(n, f)]
SCALAR_RUNS += [(n, f, 0.05 if f & HAS_PI else 0.0, t) for n in ('tiny_5x6', 'edge') for t in TRIGGERS if t != 'lda'
                for f in _flags_with(t)]
# test_poisson_mse: (flag, case), each with the layouts of SIMPLE_TRIGGERS
SIMPLE_RUNS = [(f, n) for f in (POISSON, MSE) for n in TINY_NAMES + ('deep_scalar', 'deep_vec')]
SIMPLE_TRIGGERS = (None, 'lda')


def loss_rtol(name):
    return LOSS_RTOL_EDGE if name == 'edge' else LOSS_RTOL


def deep_counts(B, G, gy, seed):
    """Row r < gy: exactly k non-zeros in each block of 256 genes (min(k, width) in a narrower last block), k = DEEP_K[r % 7];
    every row >= gy fully non-zero.  A block of 256 genes is what one wave of the vector kernels takes of a row."""
    rng = np.random.RandomState(seed)
    val = 1.0 + rng.poisson(3.0, (B, G))
    big = rng.random_sample((B, G)) < 0.1                  # counts above 16: the Stirling route of the NB branch
    val[big] *= 9.0
    y = np.zeros((B, G))
    y[gy:] = val[gy:]
    for r in range(min(gy, B)):
        k = DEEP_K[r % len(DEEP_K)]
        for b0 in range(0, G, 256):
            w = min(256, G - b0)
            cols = b0 + rng.permutation(w)[:min(k, w)]
            y[r, cols] = val[r, cols]
    return y


_inputs = {}


def inputs(name):
    """{'am', 'ad', 'ap', 'y' [B, G], 'sf' [B], 'tw' [G]} -- fp32 values held as fp64, made once, read-only."""
    if name in _inputs:
        return _inputs[name]
    c = BY_NAME[name]
    if name == 'edge':
        am, ad, ap, y, sf, tw = E.grid()
    else:
        from test_kernels_gpu import _heads
        am, ad, ap, y, sf = _heads(c.B, c.G, 100 + c.B + c.G, False)
        tw = np.random.RandomState(5 + c.G).normal(0, 1.5, c.G).astype(np.float32).astype(np.float64)
        if name == 'deep_vec':
            y = deep_counts(c.B, c.G, grid(c.B, c.G, 4).gy, 17)
    d = dict(am=am, ad=ad, ap=ap, y=y, sf=sf, tw=tw)
    assert am.shape == (c.B, c.G) and y.shape == (c.B, c.G) and sf.shape == (c.B,) and tw.shape == (c.G,)
    for v in d.values():
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
        v.setflags(write=False)
    _inputs[name] = d
    return d


def compact_queue_walk(y, gy):
    """The queue bookkeeping of zinb_nll_compact_kernel, wave by wave: a wave owns block b of 256 genes of the rows
    blockIdx.y, blockIdx.y + gy, ...; per row it pushes the row's non-zeros of its block, then flushes 64 at a time while it
    holds >= 64.  Returns (largest queue length met, set of the remainders a wave carried INTO a later row)."""
    B, G = y.shape
    nblk = -(-G // 256)
    nzc = np.stack([(y[:, b * 256:(b + 1) * 256] != 0).sum(1) for b in range(nblk)], 1)           # [B, blocks]
    qn = np.zeros((gy, nblk), np.int64)
    peak, carried = 0, set()
    for step in range(-(-B // gy)):
        rows = np.arange(gy) + step * gy
        live = rows < B
        if step:
            carried |= set(qn[live].reshape(-1).tolist())
        qn[live] += nzc[rows[live]]
        peak = max(peak, int(qn.max()))
        qn %= 64                                               # flush(false): 64 at a time while qn >= 64
    return peak, carried


# --------------------------------------------------------------------------------------------------------- oracle
_oracle = {}


def oracle(name, flags, ridge=0.0, dtype=np.float64):
    """oracle.zinb_np on inputs(name) in `dtype`, cached per (case, flags, ridge, dtype): namespace with loss (the mean
    over B G elements), g = {head: d loss / d pre-activation [B, G]} of the heads with a per-element reference, and
    d_theta_w [G] under a constant dispersion (whose 'disp' plane has no per-element reference)."""
    key = (name, flags, float(ridge), np.dtype(dtype).name)
    if key in _oracle:
        return _oracle[key]
    c, d = BY_NAME[name], inputs(name)
    am, ad, ap, y, sf, tw = (d[k].astype(dtype) for k in ('am', 'ad', 'ap', 'y', 'sf', 'tw'))
    has_pi, cdisp, loss = bool(flags & HAS_PI), bool(flags & CONST_DISP), loss_kind(flags)
    g, dth = {}, None
    n = am.size

    def run(fn, rows, **kw):
        # the likelihood is element-wise: deep batches are evaluated in row chunks on a few threads (Z.rows_in_parallel)
        if c.B >= 64:
            return Z.rows_in_parallel(fn, rows, 8, n_total=n, **kw)
        return fn(*rows, n_total=n, **kw)
    with np.errstate(all='ignore'):
        if loss == 1:
            _, lm, g['mean'] = run(Z.poisson_loss_and_grads, (am, y, sf))
        elif loss == 2:
            _, lm, g['mean'] = run(Z.mse_loss_and_grads, (am, y, sf))
        elif has_pi:
            _, lm, g['mean'], dd, g['pi'] = run(Z.zinb_loss_and_grads, (am, None if cdisp else ad, ap, y, sf), ridge=float(ridge),
                                                theta_w=tw if cdisp else None)
        else:
            _, lm, g['mean'], dd = run(Z.nb_loss_and_grads, (am, None if cdisp else ad, y, sf), theta_w=tw if cdisp else None)
        if loss == 0 and cdisp:
            dth = dd
        elif loss == 0:
            g['disp'] = dd
    for v in g.values():
        assert v.dtype == np.dtype(dtype)
        v.setflags(write=False)
    _oracle[key] = types.SimpleNamespace(loss=float(lm), g=g, d_theta_w=dth)
    return _oracle[key]


def classes(name):
    """[B, G] class of every element: its count on the edge grid, y != 0 elsewhere."""
    y = inputs(name)['y']
    return y if name == 'edge' else (y != 0).astype(np.float64)


def r_class(name, flags, ridge, head):
    """{class: max |oracle32 - oracle64|} of the head; an fp32 evaluation that is not finite where the reference is counts
    as an infinite loss (the bound then falls back to the 2e-6 max |ref| cap)."""
    r64, r32 = oracle(name, flags, ridge).g[head], oracle(name, flags, ridge, np.float32).g[head]
    with np.errstate(invalid='ignore'):
        diff = np.abs(r32.astype(np.float64) - r64)
    diff = np.where(np.isfinite(diff), diff, np.inf)
    cls = classes(name)
    return {float(c): float(diff[cls == c].max()) for c in np.unique(cls)}


def grad_bound(name, flags, ridge, head):
    """[B, G] bound of the head's gradient elements."""
    ref = oracle(name, flags, ridge).g[head]
    cls = classes(name)
    room = np.empty_like(ref)
    for c, R in r_class(name, flags, ridge, head).items():
        room[cls == c] = CLASS_FACTORS.get((head, c), RCLASS_FACTOR) * R
    return GRAD_RTOL * np.abs(ref) + np.minimum(GRAD_CAP * np.abs(ref).max(), room)


def grad_report(name, flags, ridge, head, got):
    """Per class: (elements, worst err / bound, R_class) -- the figures to print before asserting -- and the mask of the
    elements beyond the bound."""
    ref, bound, cls = oracle(name, flags, ridge).g[head], grad_bound(name, flags, ridge, head), classes(name)
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    R = r_class(name, flags, ridge, head)
    rep = {c: (int((cls == c).sum()), float(np.nan_to_num(ratio[cls == c], nan=np.inf).max()), R[c]) for c in R}
    return rep, ~(err <= bound)


# ------------------------------------------------------------------------------------------------- device layout
def lay_out(name, flags, trigger=None, grad=True, ridge=0.0):
    """Puts inputs(name) on the device in the layout of `trigger` and returns a namespace with the arguments of
    dcahip_zinb_nll (`args`, for HipOps.zinb_nll minus the partials), the flat gradient buffers `dflat` = {name: 1-D
    tensor} prefilled with SENTINEL, and what describes the call.  Every buffer is a flat tensor four floats longer than
    rows x ld; an operand is the [off:] view of it seen as [rows, ld], off = 1 where the layout shifts it.  Gathered cases
    read counts and size factors through perm / cursor from a storage of B + 7 rows that holds NaN wherever the batch
    does not reach.  A loss-only call is given no gradient buffer; a gradient call all three, so that a plane the flags do
    not write can be seen to keep the sentinel."""
    import torch
    c, d, L = BY_NAME[name], inputs(name), layout_of(BY_NAME[name].G, trigger)
    B, G, Gp = c.B, c.G, L.Gp
    has_pi, cdisp, loss = bool(flags & HAS_PI), bool(flags & CONST_DISP), loss_kind(flags)
    used = operands(flags, grad)

    def place(a, rows, ld, who, fill=0.0, pad=0.0):
        """[rows, ld] host image of `a` (rows it does not reach: fill; padding columns of the rows it reaches: pad)."""
        off = 1 if who in L.shifted else 0
        flat = np.full(rows * ld + SPARE, fill, np.float32)
        img = flat[off:off + rows * ld].reshape(rows, ld)
        r, n = a.shape
        img[:r, :] = pad
        img[:r, :n] = a
        t = torch.as_tensor(flat).to(DEVICE)
        assert t.data_ptr() % 16 == 0
        return t[off:off + rows * ld].view(rows, ld)

    v = types.SimpleNamespace(case=c, layout=L, flags=flags, grad=grad, ridge=float(ridge), inv_n=1.0 / (B * G))
    v.a_mean = place(d['am'], B, L.lda, 'a_mean')
    v.a_disp = place(d['ad'], B, L.lda, 'a_disp') if 'a_disp' in used else None
    v.a_pi = place(d['ap'], B, L.lda, 'a_pi') if 'a_pi' in used else None
    v.theta_w = place(d['tw'][None, :], 1, Gp, 'theta_w').view(-1) if 'theta_w' in used else None
    if c.gather:
        n_store = B + STORE_EXTRA
        perm = np.random.RandomState(5).permutation(n_store)[:B + CURSOR].astype(np.int32)
        rows = perm[CURSOR:CURSOR + B]
        Yst = np.full((n_store, Gp), np.nan)
        Yst[rows] = 0.0
        Yst[rows, :G] = d['y']
        sfst = np.full(n_store, np.nan)
        sfst[rows] = d['sf']
        v.y = place(Yst, n_store, L.ldy, 'y')
        v.sf = torch.as_tensor(sfst.astype(np.float32)).to(DEVICE)
        v.perm = torch.as_tensor(perm).to(DEVICE)
        v.cursor = torch.tensor([CURSOR], dtype=torch.int64, device=DEVICE)
    else:
        v.y = place(d['y'], B, L.ldy, 'y')
        v.sf = torch.as_tensor(d['sf'].astype(np.float32)).to(DEVICE)
        v.perm = v.cursor = None
    v.dflat, v.dview = {}, {}
    if grad:
        for k in GRADS:
            off = 1 if k in L.shifted else 0
            n = (B + GUARD_ROWS) * L.ldd
            flat = torch.full((n + SPARE,), float(SENTINEL), device=DEVICE)
            assert flat.data_ptr() % 16 == 0
            v.dflat[k], v.dview[k] = flat, flat[off:off + n].view(B + GUARD_ROWS, L.ldd)
    dv = v.dview
    v.args = (v.a_mean, v.a_disp, v.a_pi, L.lda, v.theta_w, v.y, L.ldy, v.sf, v.perm, v.cursor, B, G, v.ridge, v.inv_n, flags,
              dv.get('d_mean'), dv.get('d_disp'), dv.get('d_pi'), L.ldd if grad else 0)
    mis = tuple(k for k in L.shifted if k in used)
    v.vec = vec_predicate(G, flags, grad, L.lda, L.ldy, L.ldd, mis)
    v.kernel = instantiation(flags, grad, v.vec, B, L.ldd)
    v.grid = grid(B, G, 4 if v.vec else 1)
    v.written = tuple(k for k in GRADS if k in used)
    return v


def expected_writes(v, k):
    """(written, zero): boolean images [B + GUARD_ROWS, ldd] of the words of gradient plane k a call may write and of those
    it must write as 0 -- the vector form writes whole quads, columns [G, Gp) as 0; the scalar form writes [0, G) alone."""
    L, B = v.layout, v.case.B
    written = np.zeros((B + GUARD_ROWS, L.ldd), bool)
    zero = np.zeros_like(written)
    if k in v.written:
        written[:B, :L.Gp if v.vec else L.G] = True
        if v.vec:
            zero[:B, L.G:L.Gp] = True
    return written, zero
