"""The host half of the tests of dcahip_zinb_nll's kernel forms (tests/_zinb_nll_cases.py, run on the device by
tests/test_zinb_nll_forms_gpu.py): the restated host arithmetic sends every case to the form it was written for, the deep
cases walk the rows and fill the queue as their descriptions say, and the references are finite and give a usable bound."""
import numpy as np
import pytest

import _zinb_nll_cases as C

ALL_FLAGS = C.ZINB_FLAGS + (C.POISSON, C.MSE)


def test_the_predicate_follows_the_host_code():
    """vec_predicate against the expression of dcahip_zinb_nll, one term at a time, at G = 37 (Gp = 40)."""
    base = dict(G=37, flags=1, grad=True, lda=44, ldy=44, ldd=44)
    vec = lambda **kw: C.vec_predicate(**dict(base, **kw))                  # noqa: E731
    assert vec()
    assert not vec(lda=45) and not vec(ldy=46) and not vec(ldd=47) and vec(ldd=47, grad=False)
    assert not vec(lda=36) and not vec(ldy=36) and not vec(ldd=36) and vec(lda=40, ldy=40, ldd=40)
    for flags in ALL_FLAGS:
        for grad in (True, False):
            used = C.operands(flags, grad)
            for k in C.INPUTS + C.GRADS:
                assert vec(flags=flags, grad=grad, misaligned=(k,)) == (k not in used), (flags, grad, k)
    assert C.operands(3, True) == ('a_mean', 'y', 'theta_w', 'a_pi', 'd_mean', 'd_disp', 'd_pi')
    assert C.operands(0, False) == ('a_mean', 'y', 'a_disp') and C.operands(C.MSE, True) == ('a_mean', 'y', 'd_mean')
    assert C.instantiation(1, True, True, 2 ** 20, 2 ** 12) == 'zinb_nll_kernel<1,0,true,4>'      # B ldd = 2^32: out of reach
    assert C.instantiation(1, True, True, 2 ** 20, 2 ** 12 - 4) == 'zinb_nll_rows_kernel<1,0,0>'
    assert len(C.every_instantiation()) == 4 * 4 + 2 * 4


def test_every_case_and_trigger_reaches_the_form_it_claims():
    reached = set()
    for c in C.CASES:
        for flags in ALL_FLAGS:
            loss = C.loss_kind(flags)
            for grad in (True, False):
                for trig in (None,) + C.TRIGGERS:
                    kernel, g = C.reaches(c.B, c.G, flags, grad, trig)
                    scalar = trig is not None and C.applies(trig, flags, grad)
                    assert g.V == (1 if scalar else 4), (c.name, flags, grad, trig)
                    if loss:
                        want = 'zinb_nll_kernel<0,0,%s,%d,%d>' % (str(grad).lower(), g.V, loss)
                    elif scalar:
                        want = 'zinb_nll_kernel<%d,%d,%s,1>' % (flags & 1, flags >> 1 & 1, str(grad).lower())
                    else:
                        want = ('zinb_nll_rows_kernel<%d,%d,0>' if grad else 'zinb_nll_compact_kernel<%d,%d>') % (flags & 1, flags >> 1 & 1)
                    assert kernel == want, (c.name, flags, grad, trig, kernel)
                    reached.add(kernel)
                    assert g.n_partials == g.gx * g.gy <= C.GRID_CAP and g.gy <= c.B
                    # a single trigger is the single reason: the same layout without it is the vector form
                    L = C.layout_of(c.G, trig)
                    assert sum(x % 4 != 0 for x in (L.lda, L.ldy, L.ldd)) + len(L.shifted) == (trig is not None)
                    assert min(L.lda, L.ldy, L.ldd) >= L.Gp + C.SPARE
    assert reached == C.every_instantiation()


def test_the_device_runs_reach_every_instantiation():
    """The parameter lists of tests/test_zinb_nll_forms_gpu.py: every kernel dcahip_zinb_nll can launch is launched by a run
    (the V = 4 general kernel behind B * ldd >= 2^32 apart), the deep cases by the form they were built for, and every
    trigger stands alone at least once on tiny_5x6 and on edge."""
    by = {}

    def note(name, flags, trigger):
        c = C.BY_NAME[name]
        for grad in (True, False):
            by.setdefault(C.reaches(c.B, c.G, flags, grad, trigger)[0], set()).add((name, trigger))
    for name, flags, _ in C.VECTOR_RUNS:
        note(name, flags, None)
    for name, flags, _, trig in C.SCALAR_RUNS:
        assert C.applies(trig, flags, True)
        note(name, flags, trig)
        note(name, flags, None)
    for flag, name in C.SIMPLE_RUNS:
        for trig in C.SIMPLE_TRIGGERS:
            note(name, flag, trig)
    assert set(by) == C.every_instantiation()
    for f in (0, 1, 2, 3):
        p, c = f & 1, f >> 1
        assert ('deep_vec', None) in by['zinb_nll_compact_kernel<%d,%d>' % (p, c)]
        assert ('deep_vec', None) in by['zinb_nll_rows_kernel<%d,%d,0>' % (p, c)]
        for g in ('true', 'false'):
            k = by['zinb_nll_kernel<%d,%d,%s,1>' % (p, c, g)]
            assert {('deep_scalar', 'lda'), ('edge', 'lda')} <= k and {(n, 'lda') for n in C.TINY_NAMES} <= k
        have = {t for t in C.TRIGGERS if C.applies(t, f, True)}
        for n in ('tiny_5x6', 'edge'):
            assert {t for m, t in by['zinb_nll_kernel<%d,%d,true,1>' % (p, c)] if m == n} == have, (f, n)
            assert {t for m, t in by['zinb_nll_kernel<%d,%d,false,1>' % (p, c)] if m == n} == have - {'ldd'} - set(C.GRADS)
    for loss in (1, 2):
        for g in ('true', 'false'):
            for V in (4, 1):
                k = by['zinb_nll_kernel<0,0,%s,%d,%d>' % (g, V, loss)]
                assert {m for m, _ in k} >= set(C.TINY_NAMES) | {'deep_scalar', 'deep_vec'}
        assert {t for m, t in by['zinb_nll_kernel<0,0,true,1,%d>' % loss] if m == 'edge'} == set(C.SIMPLE_TRIGGER_SET)
    assert C.reaches(1400, 2050, 1, True)[1].rows_max == 3 and C.reaches(500, 2050, 1, True, 'lda')[1].rows_max == 3


def test_rows_per_workgroup_are_what_the_cases_say():
    g = C.grid(1400, 2050, 4)                      # deep_vec: three segments, the last with one active lane; 2 or 3 rows
    assert (g.nvec, g.nseg, g.gx, g.gy, g.last) == (513, 3, 3, 682, 1) and 2050 % 4 == 2
    assert (g.rows_min, g.rows_max, g.n_long) == (2, 3, 36)
    # the look-ahead (rown = row + gy clamped to row at the batch end): blockIdx.y < 36 clamps in its third row, the others in
    # their second -- so at row y + 682 the clamp holds for some workgroups and not for others
    assert 36 + 2 * 682 == 1400
    g = C.grid(500, 2050, 1)                       # deep_scalar: V = 1
    assert (g.nvec, g.nseg, g.gx, g.gy, g.last) == (2050, 9, 9, 227, 2) and (g.rows_min, g.rows_max, g.n_long) == (2, 3, 46)
    g = C.grid(3, 2880, 4)                         # edge
    assert (g.nseg, g.gy, g.rows_max, g.last) == (3, 3, 1, 208)
    tiny = {s: C.grid(s[0], s[1], 4) for s in C.TINY}
    assert {G % 4 for _, G in C.TINY} == {0, 1, 2, 3}
    assert tiny[(3, 1024)].nseg == 1 and tiny[(3, 1024)].last == 256           # exactly one full segment
    assert tiny[(3, 1025)].nseg == 2 and tiny[(3, 1025)].last == 1             # ... plus one lane
    assert tiny[(3, 256)].last == 64 and tiny[(3, 257)].last == 65             # a full wave; one lane into the second wave
    assert C.grid(3, 257, 1).nseg == 2 and C.grid(3, 257, 1).last == 1
    assert all(g.rows_max == 1 for g in tiny.values())
    for c in C.CASES:
        assert c.gather == (not c.name.startswith('tiny'))


def test_deep_vec_counts_fill_the_compact_queue():
    y = C.inputs('deep_vec')['y']
    gy = C.grid(1400, 2050, 4).gy
    nz = y != 0
    for r in range(gy):
        k = C.DEEP_K[r % 7]
        per_block = [int(nz[r, b:b + 256].sum()) for b in range(0, 2050, 256)]
        assert per_block == [k] * 8 + [min(k, 2)], r
    assert nz[gy:].all()
    peak, carried = C.compact_queue_walk(y, gy)
    # never beyond the 320 entries and one short of them: 63 left over + 256 pushed is the most a wave can hold, so slot 319
    # is a spare and the smallest capacity that would overflow on this case is 64 + 254
    assert peak == 63 + 256 == C.NZ_CAP - 1
    assert {0, 1, 63} <= carried and max(carried) == 63
    # the 64-entry flush boundary from both sides: a first row of 63, 64 and 65 entries
    assert {63, 64, 65} <= set(C.DEEP_K)
    # both routes of the non-zero branch: counts up to 16 (the product form) and above (Stirling)
    assert (y[nz] <= 16).any() and (y[nz] > 16).any() and y.max() < 1000


@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_oracle_is_finite_and_r_class_positive(name):
    d = C.inputs(name)
    assert d['y'].min() >= 0 and (d['y'] == 0).any() == (name != 'tiny_1x1')
    for flags in ALL_FLAGS:
        for ridge in C.ridges(name, flags):
            o = C.oracle(name, flags, ridge)
            assert np.isfinite(o.loss) and o.loss != 0, (name, flags, ridge)
            assert set(o.g) == {h for h, k in zip(C.HEADS, C.GRADS) if k in C.operands(flags, True)} - ({'disp'} if flags & 2 else set())
            assert (o.d_theta_w is not None) == bool(flags & 2) and (o.d_theta_w is None or np.isfinite(o.d_theta_w).all())
            if name == 'deep_vec':
                continue                   # its gradients are held element-wise elsewhere (test_zinb_nll_row_pairs_and_planes' shapes)
            for h, ref in o.g.items():
                assert np.isfinite(ref).all() and ref.dtype == np.float64, (name, flags, ridge, h)
                R = C.r_class(name, flags, ridge, h)
                assert len(R) == (8 if name == 'edge' else len(np.unique(d['y'] != 0)))
                assert all(v > 0 for v in R.values()), (name, flags, ridge, h, R)
                b = C.grad_bound(name, flags, ridge, h)
                existing = C.GRAD_RTOL * np.abs(ref) + C.GRAD_CAP * np.abs(ref).max()
                assert (b <= existing).all() and (b > 0).all()                  # nothing gets looser
                rep, bad = C.grad_report(name, flags, ridge, h, ref)
                assert not bad.any() and all(v[1] == 0 for v in rep.values())
                rep, bad = C.grad_report(name, flags, ridge, h, ref + 1.01 * b)
                assert bad.all()


def _kernel_label(text):
    """'name<a, b, ..>' (demangled or a label of _zinb_nll_cases) -> (name, args) with true / false as 1 / 0 and
    zinb_nll_kernel's defaulted LOSS = 0 written out."""
    import re
    name, args = re.search(r'(\w+)<([^>]*)>', text).groups()
    args = tuple({'true': '1', 'false': '0'}.get(x.strip(), x.strip()) for x in args.split(','))
    return name, args + ('0',) * (name == 'zinb_nll_kernel' and len(args) == 4)


def test_no_kernel_form_is_compiled_that_no_call_reaches():
    """dcahip_zinb.hip compiled for the device alone: the zinb_nll* kernels in the code object are exactly the forms an
    argument list can reach -- every_instantiation(), the four V = 4 general kernels behind B * ldd >= 2^32 and the eight
    plane forms of the row-pair kernel, 36 in all -- and each stays inside what its launch bounds and today's figures allow:
    128 registers for the two __launch_bounds__(256, 4) kernels, 16 bytes of scratch per lane, and for the loss-only kernel
    the 35 872 bytes of LDS of its queue of seven-word entries (4 waves x 320 entries x 28 bytes + 32)."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.join(root, 'include'),
                          '--cuda-device-only', '-c', os.path.join(root, 'dca_amd', 'csrc', 'dcahip_zinb.hip'), '-o', os.devnull,
                          '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    names = list(kernels)
    demangled = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True).stdout.split('\n')
    got = {_kernel_label(d): kernels[n] for n, d in zip(names, demangled) if 'zinb_nll' in d}
    want = {_kernel_label(k) for k in C.every_instantiation()}
    want |= {_kernel_label(C.instantiation(f, True, True, 2 ** 20, 2 ** 12)) for f in (0, 1, 2, 3)}
    want |= {('zinb_nll_rows_kernel', (str(f & 1), str(f >> 1), pl)) for f in (0, 1, 2, 3) for pl in ('1', '2')}
    assert len(want) == 36
    assert set(got) == want, (sorted(set(got) - want), sorted(want - set(got)))
    for (name, args), r in got.items():
        assert r['ScratchSize'] <= 16, (name, args, r)
        if name in ('zinb_nll_compact_kernel', 'zinb_nll_rows_kernel'):              # __launch_bounds__(256, 4)
            assert r['VGPRs'] + r['AGPRs'] <= 128, (name, args, r)
        if name == 'zinb_nll_compact_kernel':
            assert r['LDS Size'] <= 35872, (name, args, r)
