"""Case table and fp64 reference of the inference heads kernel's edge tests (dcahip_zinb_heads_infer, heads_infer_kernel<V>
in dca_amd/csrc/dcahip_score.hip): tests/test_heads_infer_gpu.py runs the cases on the device, tests/test_heads_infer_cases_cpu.py
checks on the host that the table reaches every path of the kernel and that the reference is what the tests take it for.
No torch here, so that the CPU half loads it.

A case lays the three pre-activation planes (mean, dispersion, dropout) out in one [B + GUARD_ROWS, lda] buffer at the column
offsets `offs`, the three outputs at `ooffs` of a [B + GUARD_ROWS, ldo] buffer that starts `out_shift` floats behind a 16-byte
aligned address (in place: the input buffer itself).  `heads_out` are the outputs asked for; the inputs of every other head
are NULL, as in the product's calls (`heads_in` == `heads_out`).  `claim` is the path the case was written for.

Path predicates, restated from the host code of dcahip_zinb_heads_infer:
    Gp   = (G + 3) & ~3
    V    = 4  when lda % 4 == 0, ldo % 4 == 0, lda >= Gp, ldo >= Gp and every non-NULL pointer is 16-byte aligned, else 1
    nvec = ceil(G / V), nseg = ceil(nvec / 256), items = B * nseg, grid = min(items, 4096): items > 4096 takes the
    grid-stride loop.

Tolerance of the device results against the fp64 oracle (RTOL, ATOL): 3e-6 relative, the figure test_kernels_gpu.py's
test_heads_infer holds the kernel to (25 fp32 steps: expf 1 ulp, log1pf 2 ulp, the reciprocal, a product and their sums stay
well inside), plus the smallest normal fp32 absolute: a result below it (the dropout at -104) may be flushed to zero.
"""
import collections
import itertools

import numpy as np

from oracle import zinb_np as Z

MSE = 8                                   # DCAHIP_NLL_MSE: the linear mean of ae_type 'normal'
GRID_CAP = 4096
HEADS = ('mean', 'disp', 'pi')
RTOL, ATOL = 3e-6, 1.2e-38
SENTINEL = np.float32(-1234.5)            # what every word outside the planted planes holds before the call
GUARD_ROWS = 2                            # rows at and beyond B that no call may touch

Case = collections.namedtuple('Case', 'name B G lda ldo offs ooffs out_shift in_place heads_in heads_out flags claim')
Path = collections.namedtuple('Path', 'V nseg items stride last triggers')


def gp(G):
    return (G + 3) & ~3


def expected_path(case):
    """What the host code of dcahip_zinb_heads_infer decides for the case.  `triggers`: every reason for the scalar form;
    `last`: the vectors (quads for V = 4, elements for V = 1) of the last 256-lane segment."""
    Gp = gp(case.G)
    trig = []
    if case.lda % 4:
        trig.append('lda')
    if case.ldo % 4:
        trig.append('ldo')
    if case.lda % 4 == 0 and case.lda < Gp or case.ldo % 4 == 0 and case.ldo < Gp:
        trig.append('ld<Gp')
    # the buffers start 16-byte aligned: a pointer is aligned when its offset in floats is a multiple of 4
    if any(case.offs[HEADS.index(h)] % 4 for h in case.heads_in):
        trig.append('in_ptr')
    if any((case.out_shift + case.ooffs[HEADS.index(h)]) % 4 for h in case.heads_out):
        trig.append('out_ptr')
    V = 1 if trig else 4
    nvec = -(-case.G // V)
    nseg = -(-nvec // 256)
    items = case.B * nseg
    return Path(V, nseg, items, items > GRID_CAP, nvec - (nseg - 1) * 256, tuple(trig))


def _make(name, B, G, claim, lda=None, ldo=None, offs=None, ooffs=None, out_shift=0, in_place=True, heads=HEADS, flags=0):
    Gp = gp(G)
    offs = offs or (0, Gp, 2 * Gp)
    lda = lda or 3 * Gp
    if in_place:
        assert ldo is None and ooffs is None and out_shift == 0
        ldo, ooffs = lda, offs
    else:
        ldo, ooffs = ldo or lda, ooffs or (0, Gp, 2 * Gp)
    heads = tuple(h for h in HEADS if h in heads)
    assert heads
    for o, ld in ((offs, lda), (ooffs, ldo)):              # the planes lie inside a row and beside each other
        assert o[0] >= 0 and o[0] + G <= o[1] and o[1] + G <= o[2] and o[2] + G <= ld, name
    return Case(name, B, G, lda, ldo, tuple(offs), tuple(ooffs), out_shift, in_place, heads, heads, flags, claim)


def _packed(G):
    """Planes side by side without padding and a row stride that is no multiple of 4: the scalar form."""
    return dict(offs=(0, G, 2 * G), lda=3 * G if (3 * G) % 4 else 3 * G + 1)


SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(HEADS, n)]


def _subset_name(prefix, s):
    return prefix + '_' + '+'.join(s)


# claim: (V, nseg, items, triggers)
LAYOUT_CASES = [
    # ---- V = 4, one segment
    _make('v4_1x1', 1, 1, (4, 1, 1, ())),
    _make('v4_7x50_out_lda156_ldo160', 7, 50, (4, 1, 7, ()), in_place=False, lda=156, ldo=160),
    _make('v4_33x1024', 33, 1024, (4, 1, 33, ())),                       # all 256 lanes of the one segment
    # ---- V = 4, several segments, the last one holding a single quad (and, at 1030, two with a ragged last quad)
    _make('v4_5x1028', 5, 1028, (4, 2, 10, ())),
    _make('v4_3x2052', 3, 2052, (4, 3, 9, ())),
    _make('v4_9x3076', 9, 3076, (4, 4, 36, ())),
    _make('v4_3x1030', 3, 1030, (4, 2, 6, ())),
    # ---- V = 4, grid-stride (more work items than the 4096 workgroups the host launches)
    _make('v4_4100x8', 4100, 8, (4, 1, 4100, ())),
    _make('v4_1400x3076', 1400, 3076, (4, 4, 5600, ())),
    # ---- V = 1, each trigger alone, at (9, 37): Gp = 40
    _make('v1_9x37_lda121', 9, 37, (1, 1, 9, ('lda',)), in_place=False, lda=121, ldo=120),
    _make('v1_9x37_ldo121', 9, 37, (1, 1, 9, ('ldo',)), in_place=False, lda=120, ldo=121),
    _make('v1_9x37_in_planes_0_37_74', 9, 37, (1, 1, 9, ('in_ptr',)), in_place=False, lda=112, offs=(0, 37, 74), ldo=120),
    _make('v1_9x37_out_shift1', 9, 37, (1, 1, 9, ('out_ptr',)), in_place=False, lda=120, ldo=120, out_shift=1),
    # lda = 3 * G + 1 = 112 IS a multiple of 4: in place, what turns the vector form off are the planes at columns 37 and 74
    _make('v1_9x37_lda112_inplace', 9, 37, (1, 1, 9, ('in_ptr', 'out_ptr')), lda=3 * 37 + 1, offs=(0, 37, 74)),
    # ---- V = 1, several segments: one and three elements in the last
    _make('v1_4x257', 4, 257, (1, 2, 8, ('lda', 'ldo', 'in_ptr', 'out_ptr')), **_packed(257)),
    _make('v1_3x515', 3, 515, (1, 3, 9, ('lda', 'ldo', 'in_ptr', 'out_ptr')), **_packed(515)),
    # ---- V = 1, grid-stride
    _make('v1_130x8193', 130, 8193, (1, 33, 4290, ('lda', 'ldo', 'in_ptr', 'out_ptr')), **_packed(8193)),
    # ---- the same values on the other form (bit equality of the two forms)
    _make('v1_7x50_packed', 7, 50, (1, 1, 7, ('lda', 'ldo', 'in_ptr', 'out_ptr')), **_packed(50)),
    _make('v4_9x37_inplace', 9, 37, (4, 1, 9, ())),
    # ---- the linear mean on both forms
    _make('v4_7x50_linear', 7, 50, (4, 1, 7, ()), flags=MSE),
    _make('v1_9x37_linear', 9, 37, (1, 1, 9, ('lda', 'ldo', 'in_ptr', 'out_ptr')), flags=MSE, **_packed(37)),
]
# ---- every non-empty subset of the outputs, in place, on both forms ('v4_7x50_mean+disp+pi' is the plain in-place call)
LAYOUT_CASES += [_make(_subset_name('v4_7x50', s), 7, 50, (4, 1, 7, ()), heads=s) for s in SUBSETS]
# (packed: the mean plane alone starts aligned, so a call for the mean only has the row strides as its triggers)
LAYOUT_CASES += [_make(_subset_name('v1_9x37', s), 9, 37,
                       (1, 1, 9, ('lda', 'ldo') + (('in_ptr', 'out_ptr') if set(s) - {'mean'} else ())), heads=s, **_packed(37))
                 for s in SUBSETS]
BY_NAME = {c.name: c for c in LAYOUT_CASES}
assert len(BY_NAME) == len(LAYOUT_CASES)

V4_FULL, V1_FULL = 'v4_7x50_mean+disp+pi', 'v1_9x37_mean+disp+pi'
SAME_BITS_IN_OUT = [(V4_FULL, 'v4_7x50_out_lda156_ldo160'), ('v1_9x37_lda112_inplace', 'v1_9x37_in_planes_0_37_74')]
SAME_BITS_V1_V4 = [('v1_7x50_packed', V4_FULL), (V1_FULL, 'v4_9x37_inplace')]
NAN_CASES = [V4_FULL, V1_FULL, 'v4_7x50_out_lda156_ldo160', 'v1_9x37_out_shift1']


# ------------------------------------------------------------------------------------------------------------- values
def _around(values):
    """Every value as fp32 with its two fp32 neighbours on either side."""
    out = []
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    for v in values:
        x = np.float32(v)
        d1, u1 = np.nextafter(x, lo), np.nextafter(x, hi)
        out += [np.nextafter(d1, lo), d1, x, u1, np.nextafter(u1, hi)]
    return np.array(out, np.float32).astype(np.float64)


MEAN_VALUES = [np.log(1e-5), np.log(1e6), 88.7, -88.7, 88.8, 104.0, -104.0, np.inf, -np.inf, 0.0, -0.0, 1e-40]
DISP_VALUES = [-9.2103, -9.21, 9.3, 9999.999, 1e4, 10000.001, 17.0, -17.0, 88.0, -88.0, -104.0, np.inf, -np.inf, 0.0]
PI_VALUES = [0.0, -0.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0, np.inf, -np.inf]


def value_cases():
    """Pre-activations at the clips, around them and beyond the range of fp32 expf, per head: fp32 values held as fp64."""
    with np.errstate(over='ignore'):
        return {'mean': _around(MEAN_VALUES), 'disp': _around(DISP_VALUES), 'pi': _around(PI_VALUES)}


def nan_positions(B, G):
    """(row, column) of the one NaN of each head's plane: three different places, the mean's in the last column (at G = 50
    and 37 the last valid column of a ragged quad), all behind the planted value cases."""
    assert B >= 7 and G >= 18
    return {'mean': (3, G - 1), 'disp': (4, 2), 'pi': (6, 17)}


_inputs = {}


def inputs(B, G, nan=False):
    """{'mean', 'disp', 'pi': [B, G], 'sf': [B]} -- fp32 values held as fp64: seeded normal data with value_cases() planted
    row-major from (0, 0) on (as many as the shape holds), `nan`: one NaN per plane at nan_positions().  The data depend on
    (B, G) alone, so that cases of one shape can be compared bit for bit; small shapes are made once and must not be
    written to."""
    key = (B, G, nan)
    if key in _inputs:
        return _inputs[key]
    if nan:
        d = {k: v.copy() for k, v in inputs(B, G).items()}
        for h, (r, c) in nan_positions(B, G).items():
            d[h][r, c] = np.nan
    else:
        rng = np.random.default_rng(100003 * B + G)
        d = {h: (s * rng.standard_normal((B, G), dtype=np.float32)).astype(np.float64)
             for h, s in (('mean', np.float32(1.5)), ('disp', np.float32(2.0)), ('pi', np.float32(2.0)))}
        d['sf'] = rng.lognormal(0.0, 0.3, B).astype(np.float32).astype(np.float64)
        for h, v in value_cases().items():
            n = min(len(v), B * G)
            d[h].reshape(-1)[:n] = v[:n]
    for v in d.values():
        v.setflags(write=False)
    if B * G <= 100000:
        _inputs[key] = d
    return d


def oracle(d, flags=0, dtype=np.float64):
    """oracle.zinb_np.heads_forward on the inputs in `dtype` (the linear mean: a_mean * sf): {'mean', 'disp', 'pi'}."""
    am, ad, ap, sf = (d[k].astype(dtype) for k in ('mean', 'disp', 'pi', 'sf'))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        mu, th, pi = Z.heads_forward(am, ad, ap, sf)
        if flags & MSE:
            mu = am * sf.reshape(-1, 1)
    return {'mean': mu, 'disp': th, 'pi': pi}


_refs = {}


def reference(B, G, flags=0, nan=False):
    """The fp64 oracle on inputs(B, G, nan); small shapes are evaluated once."""
    key = (B, G, flags & MSE, nan)
    if key in _refs:
        return _refs[key]
    r = oracle(inputs(B, G, nan), flags)
    for v in r.values():
        v.setflags(write=False)
    if B * G <= 100000:
        _refs[key] = r
    return r


def within(got, ref):
    """Element-wise: got is within RTOL |ref| + ATOL of ref; NaN where and only where ref is NaN; an infinite ref (the
    linear mean of an infinite pre-activation) is met exactly."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid='ignore'):
        ok = np.abs(got - ref) <= RTOL * np.abs(ref) + ATOL
    ok = np.where(np.isinf(ref), got == ref, ok)
    return np.where(np.isnan(ref), np.isnan(got), ok & ~np.isnan(got))


def worst(got, ref):
    """Largest error / bar over the finite reference values (a figure to print before asserting)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = np.isfinite(ref) & np.isfinite(got)
    return float((np.abs(got[m] - ref[m]) / (RTOL * np.abs(ref[m]) + ATOL)).max()) if m.any() else 0.0
