"""The byte-store first-layer kernels of dca_amd/csrc/dcahip_sparse.hip (K-SPARSE) at their edges, through HipOps, against
the fp64 references of tests/_sparse_cases.py:

  (a) dcahip_enc0_lut          the per-cell table both products look their operand up in
  (b) dcahip_enc0_fwd_lut      32 / 64 units, the shapes of _sparse_cases.FWD_SHAPES
  (c) dcahip_enc0_dw_sparse    32 / 64 (both forms) / 128 units, the shapes of _sparse_cases.DW_SHAPES
  (d) dcahip_counts_compact    its scalar-load branch and the tail of a row
  (e) argument errors          nothing is launched, the outputs stay at the sentinel

Every shape is named for a path of the kernels; that it reaches the path is asserted from the restatement of the launch
plans (_sparse_cases.fl_plan / dw_plan) before anything is launched.

Conventions.  Every output matrix has rows of ld = H1 + 4 floats and one extra row; outputs, pad columns, the extra row and
four floats behind the workspace hold the sentinel 7.0 before the launch, the workspace itself NaN; pads, extra row and the
workspace tail are asserted intact afterwards.  Every element of every output is compared: nothing is masked or dropped.
Every launch runs twice and must reproduce itself bit for bit.  Every test prints its worst error / bound before it asserts.

Bounds (none derived from a kernel's output):
  * the table without log1p is exact: three bf16 pieces hold 24 bits, so p0 + p1 + p2 = fl32(k) / fl32(fac) (IEEE division,
    what __fdiv_rn performs) bit for bit; with log1p |decoded - log1p_64(fl32(k / fac))| <= 3 * 2^-23 relative: 2 ulp is the
    device library's documented bound for log1pf, the rest the final rounding and the quotient's half ulp, which log1p
    never amplifies (d log1p(x) / log1p(x) <= dx / x);
  * products: the project's contract, |err| <= 1e-6 * Z_abs and 1e-6 * gW_abs per element (magnitudes of the terms the
    kernels form: _sparse_cases.reference_fwd / reference_dw), the bias row to 2e-6 * max_j sum_c |dZ[c, j]|.
"""
import functools

import numpy as np
import pytest
import torch

import _sparse_cases as SC
from _judge import Judge

pytestmark = pytest.mark.gpu

SENT = 7.0
F32 = dict(dtype=torch.float32, device='cuda')
EINVAL = 'code -22'


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def mat(rows, cols, a=None, ld=None, offset=0):
    """[rows + 1, ld] of the sentinel (ld = cols + 4) with a in its first rows x cols; offset: the matrix starts that many
    floats behind a 16-byte boundary.  Returns (matrix view, whole buffer)."""
    ld = ld or cols + 4
    buf = torch.full(((rows + 1) * ld + offset,), SENT, **F32)
    t = buf[offset:].view(rows + 1, ld)
    assert t.data_ptr() % 16 == 4 * (offset % 4)
    if a is not None:
        t[:rows, :cols] = dev(a)
    return t, buf


def vec(n, a, offset=0):
    buf = torch.full((n + 3 + offset,), SENT, **F32)
    t = buf[offset:offset + n]
    t[:] = dev(a)
    assert t.data_ptr() % 16 == 4 * (offset % 4)
    return t


def workspace(nbytes):
    ws = torch.full((nbytes // 4 + 4,), float('nan'), **F32)
    ws[nbytes // 4:] = SENT
    return ws


def pads_intact(J, name, t, buf, rows, cols, offset=0):
    J.true('pad columns of ' + name, bool((t[:, cols:] == SENT).all()))
    J.true('extra row of ' + name, bool((t[rows:] == SENT).all()))
    J.true('floats in front of ' + name, bool((buf[:offset] == SENT).all()))


def ws_tail_intact(J, ws, nbytes):
    J.true('workspace tail', bool((ws[nbytes // 4:] == SENT).all()))


# ------------------------------------------------------------------ the options, rotated over the shapes
NORMS = [(True, True), (True, False), (False, True), (False, False)]       # (mean, std)


def options(k):
    return dict(norm=NORMS[k % 4], bias=k % 3 != 1, gather=k % 2 == 0, fac=k % 5 != 2, log=k % 6 != 3, wide_w=(k // 2) % 2 == 1)


def _opt_id(o):
    return '%s%s-%s-%s%s%s%s' % ('m' if o['norm'][0] else '', 's' if o['norm'][1] else '', 'perm' if o['gather'] else 'base',
                                  'fac' if o['fac'] else 'nofac', '-log' if o['log'] else '-lin', '' if o['bias'] else '-nobias',
                                  '-ldw' if o['wide_w'] else '')


FWD_CASES = [(i, H1, options(i + (H1 == 64)), 0) for H1 in (32, 64) for i in range(len(SC.FWD_SHAPES))]
FWD_CASES += [(8, H1, dict(options(0), gather=H1 == 32), 1) for H1 in (32, 64)]     # 70 x 129 with the bias one float off a 16-byte boundary
DW_WIDTHS = [(32, 0), (64, 1), (64, 2), (128, 0)]
DW_OFFSET_SHAPE = 4                                                        # 150 x 520: gW one float off a 16-byte boundary
DW_CASES = [(i, H1, form, options(i + j)) for j, (H1, form) in enumerate(DW_WIDTHS) for i in range(len(SC.DW_SHAPES))]

# every option value occurs for both forward widths and for every weight-gradient kernel
for _w in (32, 64):
    _o = [o for _, h, o, _ in FWD_CASES if h == _w]
    assert {o['norm'] for o in _o} == set(NORMS)
    assert all({o[k] for o in _o} == {True, False} for k in ('bias', 'gather', 'fac', 'log', 'wide_w'))
for _w in DW_WIDTHS:
    _o = [o for _, h, f, o in DW_CASES if (h, f) == _w]
    assert {o['norm'] for o in _o} == set(NORMS) and all({o[k] for o in _o} == {True, False} for k in ('gather', 'fac', 'log'))


def _fwd_id(c):
    (B, G), _ = SC.FWD_SHAPES[c[0]]
    return '%dx%d-h%d-%s%s' % (B, G, c[1], _opt_id(c[2]), '-bias+1' if c[3] else '')


def _dw_id(c):
    (B, G) = SC.DW_SHAPES[c[0]][0]
    return '%dx%d-h%d-form%d-%s' % (B, G, c[1], c[2], _opt_id(dict(c[3], bias=True, wide_w=False)))


# ------------------------------------------------------------------ problems (computed once per shape, never modified)
@functools.lru_cache(maxsize=None)
def _rows(B, gather):
    """perm with *cursor = 3 and row_base = 2, or no perm, no cursor and row_base = 4.  The perm array is long enough for
    the index with or without row_base."""
    n = B + 9
    if gather:
        perm = np.random.RandomState(B).permutation(n)[:B + 5].astype(np.int32)
        return n, perm, 3, 2, perm[5:5 + B].astype(np.int64)
    return n, None, None, 4, np.arange(4, 4 + B)


_stores = {}


def _store(ops, B, G, gather):
    """(Y fp64 [n, G], the byte store of Y) -- one per (shape, row order)."""
    from dca_amd import compact
    key = (B, G, gather)
    if key not in _stores:
        n, _, _, _, rows = _rows(B, gather)
        Y = SC.edge_counts(n, G, 100 * B + G, rows)
        Y.setflags(write=False)
        Gp = (G + 3) // 4 * 4
        Yd = torch.zeros(n, Gp, **F32)
        Yd[:, :G] = dev(Y.astype(np.float32))
        cc = compact.build(ops, Yd, n, G)
        assert cc is not None and cc.ldc == SC.compact_ld(G) and cc.ovf_ptr is not None
        _stores[key] = (Y, cc)
    return _stores[key]


def _input(ops, B, G, o, seed):
    """Counts, normalisation and batch rows of a case: host arrays (fp32 values in fp64) and the store that describes them."""
    n, perm, cur, base, rows = _rows(B, o['gather'])
    Y, cc = _store(ops, B, G, o['gather'])
    rng = np.random.RandomState(seed)
    fac = SC.f32(rng.lognormal(0, 0.4, n)) if o['fac'] else None
    L = SC.dense_input(Y, fac, o['log'], None, None)
    mean = SC.f32(L.mean(0)) if o['norm'][0] else None
    std = SC.f32(np.maximum(L.std(0, ddof=1), 1e-3)) if o['norm'][1] else None
    d = lambda a: dev(a) if a is not None else None
    cci = cc.with_input(d(fac), o['log'], d(mean), d(std), ops=ops)
    dperm = torch.as_tensor(perm).cuda() if perm is not None else None
    dcur = torch.tensor([cur], dtype=torch.int64, device='cuda') if cur is not None else None
    return dict(Y=Y, fac=fac, log=o['log'], mean=mean, std=std, rows=rows, cc=cci, perm=dperm, cur=dcur, base=base)


# ------------------------------------------------------------------ (a) the table
@pytest.mark.parametrize('do_log', [0, 1])
@pytest.mark.parametrize('use_fac', [True, False])
def test_table_entries(ops, use_fac, do_log):
    n, K = 37, 128
    assert ops.enc0_lut_entries() == K
    fac32 = np.logspace(-3, 3, n).astype(np.float32)
    fac32[5], fac32[9], fac32[0], fac32[-1] = 1.0, 0.25, 1e-3, 1e3
    J = Judge('enc0_lut fac=%s log=%d' % (use_fac, do_log))
    runs = []
    for _ in range(2):
        lut = torch.full((n + 1, K, 2), 0x07070707, dtype=torch.int32, device='cuda')
        ops.enc0_lut(dev(fac32) if use_fac else None, do_log, n, lut)
        torch.cuda.synchronize()
        runs.append(lut)
    J.true('bit for bit', torch.equal(runs[0], runs[1]))
    J.true('row behind the table', bool((runs[0][n:] == 0x07070707).all()))
    raw = runs[0][:n].cpu().numpy()
    got = SC.decode_lut(raw)
    q32 = np.arange(K, dtype=np.float32)[None, :] / (fac32[:, None] if use_fac else np.ones((n, 1), np.float32))     # IEEE fp32 division
    assert q32.dtype == np.float32 and q32.shape == (n, K)
    J.true('entry 0 is +0.0', bool((raw[:, 0, :] == 0).all()))
    if do_log:
        ref = np.log1p(q32.astype(np.float64))
        J.bound('log1p', 'table', np.abs(got - ref), 3 * 2.0 ** -23 * ref)
    else:
        J.true('the quotient, bit for bit', np.array_equal(got, q32.astype(np.float64)))
        J.bound('exact', 'table', np.abs(got - q32.astype(np.float64)), 0.0 * got)
    J.report()


# ------------------------------------------------------------------ (b) forward
@pytest.mark.parametrize('case', FWD_CASES, ids=_fwd_id)
def test_forward_edges(ops, case):
    i, H1, o, bias_off = case
    (B, G), want = SC.FWD_SHAPES[i]
    plan = SC.fl_plan(B, G)
    assert {k: plan[k] for k in want} == want, plan
    p = _input(ops, B, G, o, 7 * B + G + H1)
    assert p['cc'].ldc == plan['ldc']
    rng = np.random.RandomState(B + G + H1)
    W, b = SC.f32(rng.normal(0, 0.1, (G, H1))), SC.f32(rng.normal(0, 0.3, H1)) if o['bias'] else None
    Z_ref, Z_abs = SC.reference_fwd(p['Y'], p['fac'], p['log'], p['mean'], p['std'], p['rows'], W, b)
    ldw = H1 + 4 if o['wide_w'] else H1
    Wd, _ = mat(G, H1, W, ld=ldw)
    bd = vec(H1, b, offset=bias_off) if b is not None else None
    nb = ops.enc0_fwd_lut_workspace_bytes(B, G, H1)
    assert nb > 0
    ws = workspace(nb)
    J = Judge('enc0_fwd_lut %s' % _fwd_id(case))
    outs = []
    for _ in range(2):
        Z, Zbuf = mat(B, H1)
        ops.enc0_fwd_lut(p['cc'], p['perm'], p['cur'], p['base'], B, G, H1, Wd, ldw, bd, Z, H1 + 4, ws)
        torch.cuda.synchronize()
        pads_intact(J, 'Z', Z, Zbuf, B, H1)
        outs.append(Z)
    ws_tail_intact(J, ws, nb)
    J.true('bit for bit', torch.equal(outs[0], outs[1]))
    J.bound('Z', 'Z', np.abs(host(outs[0])[:B, :H1] - Z_ref), 1e-6 * Z_abs)
    J.report()


# ------------------------------------------------------------------ (c) weight gradient
@pytest.mark.parametrize('case', DW_CASES, ids=_dw_id)
def test_weight_gradient_edges(ops, case):
    i, H1, form, o = case
    (B, G), first, ring = SC.DW_SHAPES[i]
    plan = SC.dw_plan(B, G, H1, form)
    want = ring if form == 2 else first
    assert plan['ring'] == (form == 2) and {k: plan[k] for k in want} == want, plan
    p = _input(ops, B, G, o, 11 * B + G + H1 + form)
    rng = np.random.RandomState(B + G + H1 + form)
    dZ = SC.f32(rng.normal(0, 1e-3, (B, H1)))
    gW_ref, col_ref, gW_abs, col_mag = SC.reference_dw(p['Y'], p['fac'], p['log'], p['mean'], p['std'], p['rows'], dZ)
    dZd, _ = mat(B, H1, dZ)
    off = 1 if i == DW_OFFSET_SHAPE else 0
    nb = ops.enc0_dw_sparse_workspace_bytes(B, G, H1)
    assert nb > 0
    ws = workspace(nb)
    J = Judge('enc0_dw_sparse %s%s' % (_dw_id(case), ' gW+1' if off else ''))
    outs = []
    for _ in range(2):
        gW, gbuf = mat(G + 1, H1, offset=off)
        ops.enc0_dw_sparse(p['cc'], p['perm'], p['cur'], p['base'], B, G, H1, dZd, H1 + 4, gW, H1 + 4, ws, form=form)
        torch.cuda.synchronize()
        pads_intact(J, 'gW', gW, gbuf, G + 1, H1, off)
        outs.append(gW)
    ws_tail_intact(J, ws, nb)
    J.true('bit for bit', torch.equal(outs[0], outs[1]))
    got = host(outs[0])
    J.bound('gW', 'gW', np.abs(got[:G, :H1] - gW_ref), 1e-6 * gW_abs)
    J.bound('bias row', 'bias row', np.abs(got[G, :H1] - col_ref), 2e-6 * col_mag)
    J.report()


# ------------------------------------------------------------------ (d) the byte store
def _decode(cc, n, G):
    out = cc.Yc.cpu().numpy()[:, :G].astype(np.float64)
    if cc.ovf_ptr is not None:
        ptr, col, val = cc.ovf_ptr.cpu().numpy(), cc.ovf_col.cpu().numpy(), cc.ovf_val.cpu().numpy()
        for r in range(n):
            for k in range(ptr[r], ptr[r + 1]):
                assert out[r, col[k]] == 255
                out[r, col[k]] = val[k]
    return out


def _compact_layouts(G):
    """(name, ldy, offset of the source in floats): a row stride that is no multiple of 4, ldy = G, and a source one float
    off a 16-byte boundary.  All but ldy = G with G % 4 == 0 take the scalar loads; every one ends inside a group of four."""
    ld1 = G + 1 if (G + 1) % 4 else G + 2
    return [('ldy=G+', ld1, 0), ('ldy=G', G, 0), ('src+1', (G + 3) // 4 * 4, 1)]


@pytest.mark.parametrize('G', [1, 15, 16, 17, 33])
def test_compact_store_scalar_loads_and_row_tail(ops, G):
    from dca_amd import compact
    n = 7
    J = Judge('counts_compact G=%d' % G)
    for name, ldy, off in _compact_layouts(G):
        scalar = ldy % 4 != 0 or off % 4 != 0
        assert scalar or G % 4 == 0
        Y = SC.edge_counts(n, G, G)
        for k, v in enumerate((254.0, 255.0, 256.0, 2.0 ** 24, -0.0)):
            Y[k, (k * 5) % G] = v
            Y[(k + 2) % n, G - 1] = v
        # what lies behind a row's G counts (and in front of / behind the matrix) is no count: it must not be looked at
        buf = torch.full((n * ldy + off + 4,), -1.5, **F32)
        Yd = buf[off:off + n * ldy].view(n, ldy)
        Yd[:, :G] = dev(Y)
        assert Yd.data_ptr() % 16 == 4 * off and np.signbit(Y).any() and all((Y == v).any() for v in (254, 255, 256, 2 ** 24))
        ldc = ops.counts_compact_ld(G)
        assert ldc == SC.compact_ld(G)
        runs = []
        for _ in range(2):
            Yc = torch.full((n + 1, ldc), 0x55, dtype=torch.uint8, device='cuda')
            status = torch.tensor([0, 0, 0x0707], dtype=torch.int32, device='cuda')
            ops.counts_compact(Yd, ldy, n, G, Yc, ldc, status)
            torch.cuda.synchronize()
            runs.append((Yc, status))
        J.true(name + ': bit for bit', torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]))
        Yc, status = runs[0]
        J.true(name + ': row behind the store', bool((Yc[n:] == 0x55).all()))
        J.true(name + ': pad bytes are 0', bool((Yc[:n, G:] == 0).all()))
        st = status.cpu().numpy()
        J.true(name + ': status %s' % st, st[0] == 0 and st[1] == int((Y >= 255).sum()) and st[2] == 0x0707)
        J.true(name + ': bytes', np.array_equal(Yc[:n, :G].cpu().numpy(), np.minimum(Y, 255).astype(np.uint8)))
        cc = compact.build(ops, Yd, n, G)
        assert cc is not None
        J.true(name + ': build() writes the same bytes', torch.equal(cc.Yc, Yc[:n]))
        J.true(name + ': round trip', np.array_equal(_decode(cc, n, G), Y))
        # what is not a count, on the same path: stored as 0 and counted exactly
        bad = [(0, 0, 0.5), (1, G - 1, -1.0), (2, G // 2, float('nan')), (3, 0, float('inf')), (4, G - 1, 0.5), (5, G // 3, -1.0),
               (6, G - 1, float('-inf'))]
        Ybuf = buf.clone()
        Ybd = Ybuf[off:off + n * ldy].view(n, ldy)
        assert Ybd.data_ptr() % 16 == 4 * off
        Yh = Y.copy()
        for r, g, v in bad:
            Ybd[r, g] = v
            Yh[r, g] = 0
        Yc = torch.full((n + 1, ldc), 0x55, dtype=torch.uint8, device='cuda')
        status = torch.zeros(2, dtype=torch.int32, device='cuda')
        ops.counts_compact(Ybd, ldy, n, G, Yc, ldc, status)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        J.true(name + ': refused values, status %s' % st, st[0] == len(bad) and st[1] == int((Yh >= 255).sum()))
        J.true(name + ': refused values are stored as 0', np.array_equal(Yc[:n, :G].cpu().numpy(), np.minimum(Yh, 255).astype(np.uint8)))
        J.true(name + ': build() refuses', compact.build(ops, Ybd, n, G) is None)
    J.report()


# ------------------------------------------------------------------ (e) argument errors
def _refused(J, what, call, outputs):
    try:
        call()
        J.true(what + ': not refused', False)
    except RuntimeError as e:
        J.true(what + ': ' + str(e), EINVAL in str(e))
    torch.cuda.synchronize()
    for t in outputs:
        J.true(what + ': output left at the sentinel', bool((t == SENT).all()))


def test_forward_argument_errors(ops):
    from dca_amd.compact import CompactCounts
    B, G, H1 = 40, 20, 32
    o = dict(options(0), gather=False)
    p = _input(ops, B, G, o, 1)
    cc = p['cc']
    cc.ensure_lut(ops)
    J = Judge('enc0_fwd_lut argument errors')
    W = torch.full((G + 1, 132), 0.1, **F32)
    bias = torch.zeros(132, **F32)
    nb = ops.enc0_fwd_lut_workspace_bytes(B, G, H1)
    ws = torch.zeros(nb // 4 + 4, **F32)
    zbuf = torch.full(((B + 1) * 136 + 4,), SENT, **F32)
    Z = zbuf[:(B + 1) * 36].view(B + 1, 36)
    call = lambda **k: (lambda: ops.enc0_fwd_lut(k.get('cc', cc), None, None, 4, B, G, k.get('H1', H1), W, k.get('ldw', 132), bias,
                                                 k.get('Z', Z), k.get('ldz', 36), k.get('ws', ws)))
    for h in (16, 128):
        J.true('no workspace for %d units' % h, ops.enc0_fwd_lut_workspace_bytes(B, G, h) == 0)
        _refused(J, '%d units' % h, call(H1=h, ldz=h + 4), [zbuf])
    _refused(J, 'ldz % 4 != 0', call(ldz=37), [zbuf])
    _refused(J, 'Z misaligned', call(Z=zbuf[1:1 + (B + 1) * 36].view(B + 1, 36)), [zbuf])
    _refused(J, 'ldw < H1', call(ldw=H1 - 1), [zbuf])
    odd = CompactCounts(cc.Yc, cc.ldc - 8, cc.ovf_ptr, cc.ovf_col, cc.ovf_val, cc.fac, cc.do_log, cc.mean, cc.std)
    odd.lutp = cc.lutp
    assert odd.ldc >= G and odd.ldc % 16 == 8
    _refused(J, 'ldc % 16 != 0', call(cc=odd), [zbuf])
    _refused(J, 'workspace 16 bytes short', call(ws=ws[:nb // 4 - 4]), [zbuf])
    call()()                                    # and the same arguments unchanged are taken
    torch.cuda.synchronize()
    J.true('the valid call writes Z', bool((Z[:B, :H1] != SENT).all()) and bool((Z[:, H1:] == SENT).all()))
    J.report()


def test_weight_gradient_argument_errors(ops):
    B, G, H1 = 40, 20, 32
    o = dict(options(0), gather=False)
    p = _input(ops, B, G, o, 1)
    cc = p['cc']
    J = Judge('enc0_dw_sparse argument errors')
    dZ = torch.full((B + 1, 132), 1e-3, **F32)
    nb = ops.enc0_dw_sparse_workspace_bytes(B, G, H1)
    ws = torch.zeros(nb // 4 + 4, **F32)
    gbuf = torch.full(((G + 2) * 136,), SENT, **F32)
    gW = gbuf[:(G + 2) * 36].view(G + 2, 36)
    call = lambda **k: (lambda: ops.enc0_dw_sparse(cc, None, None, 4, B, G, k.get('H1', H1), dZ, k.get('ldz', 132), gW,
                                                   k.get('ldg', 36), k.get('ws', ws), form=k.get('form', 0)))
    _refused(J, 'form = 3', call(form=3), [gbuf])
    _refused(J, 'ldg < H1', call(ldg=H1 - 4), [gbuf])
    _refused(J, 'ldz < H1', call(ldz=H1 - 4), [gbuf])
    J.true('no workspace for 48 units', ops.enc0_dw_sparse_workspace_bytes(B, G, 48) == 0 and not ops.enc0_sparse_supported(48))
    _refused(J, '48 units', call(H1=48, ldg=52), [gbuf])
    _refused(J, 'workspace 16 bytes short', call(ws=ws[:nb // 4 - 4]), [gbuf])
    call()()
    torch.cuda.synchronize()
    J.true('the valid call writes gW', bool((gW[:G + 1, :H1] != SENT).all()) and bool((gW[:, H1:] == SENT).all()))
    J.report()
