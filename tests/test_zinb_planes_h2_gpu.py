"""dcahip_zinb_nll_planes_h2 -- the likelihood kernel that writes the head gradients as two fp16 pieces of g 2^d_exp (the
operand of dcahip_gemm_h2; zinb_nll_rows_kernel's PL == 2 instantiation) -- against the fp64 oracle and against the
piece contract of h2_math.hpp, element by element.

How the pieces are pinned down exactly: inv_n is a free argument, passed here as 2^-16 whatever B G is.  The fp32 planes D
of dcahip_zinb_nll on the same arguments then hold fl32(g) 2^-16 exactly (no D here is an fp32 denormal: asserted), and
the fp16 planes must hold the split of x = D 2^(16 + d_exp), a value the test forms without rounding.
"""
import numpy as np
import pytest
import torch

from conftest import synth_counts
from oracle import zinb_np as Z
import _zinb_edge_grid as E

pytestmark = pytest.mark.gpu

EINVAL = -22
INV_N = 2.0 ** -16
SENT = 0x5A5A                            # bit pattern the planes are prefilled with (fp16 203.25)


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _r4(n):
    return (n + 3) // 4 * 4


def _ulp16(p0):
    """ulp of fp16 at |p0| (the denormal step 2^-24 below 2^-14)."""
    _, e = np.frexp(np.abs(p0))
    return np.where(p0 == 0, 2.0 ** -24, np.ldexp(1.0, np.maximum(e - 1, -14) - 10))


def run_both(ops, flags, am, ad, ap, tw, y, sf, ridge, d_exp, gather):
    """dcahip_zinb_nll (fp32 planes) and dcahip_zinb_nll_planes_h2 (twice) on the same arguments.  With `gather` the
    counts and size factors sit in a storage of B + 7 rows read through perm / cursor, NaN wherever the batch does not
    reach; the planes are two rows taller than the batch and prefilled with a sentinel."""
    has_pi, cdisp = bool(flags & 1), bool(flags & 2)
    B, G = am.shape
    Gp = _r4(G)
    lda = 3 * Gp
    A = np.zeros((B, lda)); A[:, :G] = am; A[:, Gp:Gp + G] = ad; A[:, 2 * Gp:2 * Gp + G] = ap
    if gather:
        n_store, cur = B + 7, 3
        perm = np.random.RandomState(5).permutation(n_store)[:B + 3].astype(np.int32)
        rows = perm[cur:cur + B]
        Yst = np.full((n_store, Gp), np.nan); Yst[rows] = 0.0; Yst[rows, :G] = y
        sfst = np.full(n_store, np.nan); sfst[rows] = sf
        dperm, dcur = torch.as_tensor(perm).cuda(), torch.tensor([cur], dtype=torch.int64, device='cuda')
    else:
        Yst = np.zeros((B, Gp)); Yst[:, :G] = y
        sfst, dperm, dcur = sf, None, None
    dA, dY, dsf, dtw = dev(A), dev(Yst), dev(sfst), dev(tw)
    a_mean, a_disp, a_pi = dA[:, 0:], None if cdisp else dA[:, Gp:], dA[:, 2 * Gp:] if has_pi else None
    dD = torch.full((B, lda), 7.0, device='cuda')
    part = torch.zeros(ops.max_partials, dtype=torch.float64, device='cuda')
    loss = torch.zeros(1, device='cuda')
    n0 = ops.zinb_nll(a_mean, a_disp, a_pi, lda, dtw if cdisp else None, dY, Gp, dsf, dperm, dcur, B, G, ridge, INV_N, flags,
                      dD[:, 0:], dD[:, Gp:], dD[:, 2 * Gp:] if has_pi else None, lda, part)
    ops.loss_finalize(part, n0, INV_N, loss)
    torch.cuda.synchronize()
    loss32 = loss.item()
    cols = {'mean': 0, 'disp': Gp + 8, 'pi': 2 * Gp + 16}
    ldp = (3 * Gp + 16 + 7) // 8 * 8 + 8
    out = []
    for _ in range(2):
        P = torch.empty(2, B + 2, ldp, dtype=torch.float16, device='cuda')
        P.view(torch.int16).fill_(SENT)
        Dth = torch.full((B, Gp), 7.0, device='cuda') if cdisp else None
        part.fill_(-1.0)
        n = ops.zinb_nll_planes_h2(a_mean, a_disp, a_pi, lda, dtw if cdisp else None, dY, Gp, dsf, dperm, dcur, B, G, ridge,
                                   INV_N, flags, d_exp, P, cols['mean'], 0 if cdisp else cols['disp'],
                                   cols['pi'] if has_pi else 0, Dth, Gp, part)
        ops.loss_finalize(part, n, INV_N, loss)
        torch.cuda.synchronize()
        out.append((P, Dth, part[:n].clone(), loss.item()))
    (P, Dth, part1, loss16), (P2, Dth2, part2, _) = out
    # determinism: a second call gives bit-identical pieces and partials
    assert torch.equal(P.view(torch.int16), P2.view(torch.int16)) and torch.equal(part1, part2)
    assert n == n0 and loss16 == loss32                   # the same sums in the same order as the fp32-plane kernel
    dth = None
    if cdisp:                                             # the per-gene dispersion's plane stays fp32 and keeps inv_n
        assert torch.equal(Dth, Dth2)
        dth = (Dth[:, :G].cpu().numpy(), dD[:, Gp:Gp + G].cpu().numpy())
    heads = ['mean'] + ([] if cdisp else ['disp']) + (['pi'] if has_pi else [])
    Pb = P.view(torch.int16).cpu().numpy().view(np.uint16)
    # layout: the padded quad columns of each head are written 0; the gaps between the heads, the columns past the last
    # head and the rows past the batch keep the sentinel
    untouched = np.ones((B + 2, ldp), bool)
    for h in heads:
        c0 = cols[h]
        untouched[:B, c0:c0 + Gp] = False
        assert (P[:, :B, c0 + G:c0 + Gp].float() == 0).all(), h
    assert untouched[:B].any() and (Pb[:, untouched] == SENT).all(), 'wrote outside the head columns'
    D = dD.cpu().numpy()
    Pf = P.cpu()
    res = {}
    for k, h in enumerate(('mean', 'disp', 'pi')):
        if h in heads:
            c0 = cols[h]
            res[h] = (D[:, k * Gp:k * Gp + G], Pf[0, :B, c0:c0 + G], Pf[1, :B, c0:c0 + G])
    return loss32, res, dth


def check_d_theta(dth):
    """Constant dispersion: d_theta is bit for bit dcahip_zinb_nll's d_disp plane (the last check of a test: what it finds
    is reported after everything else about the pieces has been verified).

    This check found a defect.  At (B, G) = (700, 2050), flags 3, 210 of 1 435 000 d_theta values of the PL == 2
    instantiation of zinb_nll_rows_kernel lay one fp32 ulp (at most 1.7e-7 relative) from the PL == 0 instantiation's, all
    at y = 0 with t < 2^-5 (the series of zinb_zero_elem).  In the PL == 0 and PL == 1 kernels the compiler packed -t t and
    t (2/3 - ...) into one two-wide multiplication and then subtracted the rounded product from 0.5; in the PL == 2 kernel,
    whose planes have two scales, it did not pack and fused the same multiplication into the subtraction.  The series
    is now written with explicit fused multiply-adds (zinb_math.hpp), so every kernel rounds it the same way."""
    if dth is not None:
        got, want = dth
        d = got != want
        rel = np.abs(got[d].astype(np.float64) - want[d]) / np.abs(want[d]) if d.any() else np.zeros(1)
        print('d_theta: %d of %d differ from the fp32-plane kernel, rel max %.3g' % (int(d.sum()), d.size, float(rel.max())))
        assert not d.any(), (int(d.sum()), d.size, float(rel.max()), np.argwhere(d)[:5])


def check_pieces(name, D, p0, p1, ref, d_exp, require_normal=True):
    """(a) the reconstruction against the fp64 oracle, (b) the piece contract per element, (c) the first piece is the
    round-to-nearest fp16 of x and the second no larger than half its ulp."""
    nzD = np.abs(D[D != 0])
    assert nzD.size and (not require_normal or nzD.min() >= 2.0 ** -126), (name, 'an fp32 plane value is denormal')
    x = D.astype(np.float64) * 2.0 ** (16 + d_exp)
    x32 = torch.as_tensor(x.astype(np.float32))
    assert np.array_equal(x32.numpy().astype(np.float64), x)
    q0, q1 = p0.double().numpy(), p1.double().numpy()
    assert np.isfinite(q0).all() and np.isfinite(q1).all(), (name, 'a piece is not finite')
    # (a) 2e-4 |ref| + 2e-6 max |ref|: what test_kernels_gpu.py::test_zinb_nll_vs_oracle grants the fp32 kernel
    rec = (q0 + q1) * 2.0 ** -d_exp * INV_N
    fin = np.isfinite(ref)
    err = np.abs(rec - ref)
    tol = 2e-4 * np.abs(ref) + 2e-6 * np.abs(ref[fin]).max()
    bad = fin & ~(err <= tol)
    print(name, 'oracle: worst err / tol = %.3g' % float((err[fin] / np.maximum(tol[fin], 1e-300)).max()))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], rec[bad][:5], ref[bad][:5])
    # (b) h2_math.hpp: 2^-22 relative, 2^-25 absolute where the second piece is an fp16 denormal -- of the ELEMENT
    e = np.abs(q0 + q1 - x)
    lim = 2.0 ** -22 * np.abs(x) + 2.0 ** -25
    print(name, 'pieces: worst err / bound = %.3g' % float((e / lim).max()))
    bad = ~(e <= lim)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], q0[bad][:5], q1[bad][:5], x[bad][:5])
    # (c) round to nearest (not truncation), and a second piece that belongs to this first piece
    want = x32.half()
    assert torch.equal(p0.view(torch.int16), want.view(torch.int16)), (name, int((p0 != want).sum()))
    assert (np.abs(q1) <= 0.5 * _ulp16(q0)).all(), name
    # where the residual is representable the second piece is the residual itself
    r = x - q0
    rep = np.abs(r) >= 2.0 ** -14
    assert np.array_equal(q1[rep], torch.as_tensor(r[rep].astype(np.float32)).half().double().numpy())


_ORACLE = {}


def _case(B, G, flags, dense):
    """Inputs and the oracle's gradients (scaled by INV_N), computed once per (shape, flags)."""
    key = (B, G, flags, dense)
    if key not in _ORACLE:
        rng = np.random.RandomState(11 + B)
        am = rng.normal(0, 1.5, (B, G)); ad = rng.normal(0, 2, (B, G)); ap = rng.normal(0, 2, (B, G))
        y = synth_counts(B, G, 11 + B)
        if dense:
            y = y + 1.0
        sf = rng.lognormal(0, 0.3, B)
        # log-dispersions of N(0, 0.7): theta = exp(tw) stays below ~15, so that (theta / (theta + mu))^theta and with it
        # the y = 0 gradients stay far above the fp32 denormals after the 2^-16 scale (N(0, 1.5) reaches theta ~ 150,
        # where they pass through the denormal range and x = D 2^(16 + d_exp) is no longer exact)
        tw = rng.normal(0, 0.7, G)
        am, ad, ap, y, sf, tw = (a.astype(np.float32).astype(np.float64) for a in (am, ad, ap, y, sf, tw))
        ridge = 0.05 if flags & 1 else 0.0
        lm, g = E.oracle_grads(flags, am, ad, ap, y, sf, tw, ridge, n_total=1.0 / INV_N)
        # the oracle's mean divides the loss sum by n_total as well: what loss_finalize(scale = INV_N) gives
        _ORACLE[key] = (am, ad, ap, tw, y, sf, ridge, lm, g)
    return _ORACLE[key]


# (B, G) = (700, 2050): nvec = 513 -> three gene segments, the last with ONE active lane (the ballots run with 255 lanes
#   outside the row); grid.y = 682 -> rows 682..699 are the second row of a pair for some workgroups and absent for others;
#   G % 4 = 2 -> a partial last quad; gathered through perm / cursor.
# (2500, 1000), every count non-zero: the LDS queue at its 2 x 256 capacity, several row pairs per workgroup.
# (5, 6): a single row pair with one row absent.
CASES = ([(700, 2050, f, d, False, True) for f in (1, 3, 0) for d in (2, -3)]
         + [(2500, 1000, 1, 2, True, False), (2500, 1000, 3, -3, True, False), (2500, 1000, 0, 2, True, False)]
         + [(5, 6, f, d, False, g) for f, d, g in ((1, 2, False), (3, -3, True), (0, -3, False), (1, -3, True))])


@pytest.mark.parametrize('B,G,flags,d_exp,dense,gather', CASES)
def test_planes_h2_vs_oracle_and_piece_contract(ops, B, G, flags, d_exp, dense, gather):
    am, ad, ap, tw, y, sf, ridge, lm, gref = _case(B, G, flags, dense)
    loss, res, dth = run_both(ops, flags, am, ad, ap, tw, y, sf, ridge, d_exp, gather)
    assert abs(loss - lm) <= 3e-6 * abs(lm), (loss, lm)
    assert set(res) == set(gref)
    for h, (D, p0, p1) in res.items():
        check_pieces(h, D, p0, p1, gref[h], d_exp)
    check_d_theta(dth)


@pytest.mark.parametrize('ridge', E.RIDGES)
@pytest.mark.parametrize('flags', [1, 3, 0])
def test_range_bound_on_the_edge_grid(ops, flags, ridge):
    """d_exp = floor(log2(65000 / bound)) exactly as Engine._data_scales computes it from y_max and ridge: on every
    combination of the likelihood's edge inputs no fp16 piece overflows, and the pieces still hold the gradient."""
    assert E.worst_bound_ratio(flags, ridge) <= 1.0           # the oracle alone stays inside the bound (CPU half)
    am, ad, ap, y, sf, tw = E.grid()
    d_exp = E.d_exp_of(y.max(), ridge)
    assert d_exp == (1 if ridge == 1e3 else 2)
    lm, gref = E.oracle_grads(flags, am, ad, ap, y, sf, tw, ridge, n_total=1.0 / INV_N)
    loss, res, dth = run_both(ops, flags, am, ad, ap, tw, y, sf, ridge, d_exp, gather=True)
    # the edge allowance of test_kernels_gpu.py::test_zinb_nll_vs_oracle (y = 5000 next to theta ~ 1e4: one ulp of an
    # fp32 lgamma / log term is already ~4e-3 absolute)
    assert abs(loss - lm) <= 3e-5 * abs(lm), (loss, lm)
    for h, (D, p0, p1) in res.items():
        assert np.isfinite(gref[h]).all()
        assert torch.isfinite(p0).all() and torch.isfinite(p1).all(), h
        big = float(np.abs(p0.double().numpy()).max())
        print(h, 'largest first piece %.1f of 65504' % big)
        # (an fp32 plane value that is denormal here has lost at most 2^-149 2^18 of x: far inside (b)'s absolute term,
        # and x.half() is 0 either way)
        check_pieces(h, D, p0, p1, gref[h], d_exp, require_normal=False)
    check_d_theta(dth)


def test_argument_checks(ops):
    """Return codes only: every refused call returns before a launch; the call they all differ from is accepted."""
    import ctypes
    from dca_amd import hip
    L, p = ops.L, hip.ptr
    B, G, Gp = 6, 10, 12
    lda = 3 * Gp
    A = torch.zeros(B, lda, device='cuda')
    Y = torch.zeros(B, Gp, device='cuda')
    sf = torch.ones(B, device='cuda')
    tw = torch.zeros(Gp, device='cuda')
    ldp = 48
    P = torch.zeros(2, B, ldp, dtype=torch.float16, device='cuda')
    Dth = torch.zeros(B, Gp, device='cuda')
    part = torch.zeros(ops.max_partials, dtype=torch.float64, device='cuda')
    n = ctypes.c_int(0)
    base = dict(flags=1, d_exp=2, ridge=0.05, ldp=ldp, stride=B * ldp, cm=0, cd=Gp, cp=2 * Gp, dth=None)

    def call(**kw):
        a = dict(base); a.update(kw)
        cdisp = bool(a['flags'] & 2)
        return L.dcahip_zinb_nll_planes_h2(p(A), None if cdisp else p(A[:, Gp:]), p(A[:, 2 * Gp:]), lda, p(tw) if cdisp else None,
                                           p(Y), Gp, p(sf), None, None, B, G, a['ridge'], INV_N, a['flags'], a['d_exp'],
                                           p(P), a['ldp'], a['stride'], a['cm'], a['cd'], a['cp'], p(a['dth']), Gp,
                                           p(part), ctypes.byref(n), hip.stream())
    assert call() == 0
    assert call(flags=3, dth=Dth) == 0 and call(flags=0) == 0
    assert call(d_exp=40) == 0 and call(d_exp=-40) == 0 and call(ridge=0.0) == 0
    assert call(d_exp=41) == EINVAL and call(d_exp=-41) == EINVAL
    assert call(ridge=-0.5) == EINVAL and call(ridge=float('nan')) == EINVAL
    assert call(flags=4) == EINVAL and call(flags=8) == EINVAL and call(flags=1 | 4) == EINVAL
    assert call(ldp=ldp - 2, stride=B * ldp) == EINVAL                 # ldp % 4 != 0
    assert call(cm=2) == EINVAL and call(cd=Gp + 2) == EINVAL and call(cp=2 * Gp + 1) == EINVAL
    assert call(cp=ldp - Gp + 4) == EINVAL and call(cd=ldp - 8) == EINVAL and call(cm=ldp - 8) == EINVAL    # col + r4(G) > ldp
    assert call(cp=ldp - Gp) == 0                                      # the last head ends at ldp exactly
    assert call(stride=B * ldp - 4) == EINVAL                          # the second piece would overlap the first
    assert call(flags=3, dth=None) == EINVAL                           # constant dispersion without d_theta
    torch.cuda.synchronize()
