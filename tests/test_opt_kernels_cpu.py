"""The shared K-OPT / step-end cases (tests/_opt_kernel_cases.py) on the oracle-backed ops object: validates the case logic
and the oracle's own contract without a GPU; the basis of the cases' tolerance; and the CPU half of the range bound of the
fp16 x 2 gradient planes (tests/test_zinb_planes_h2_gpu.py holds the GPU half)."""
import pytest

from oracle.cpu_ops import CpuRefOps
import _opt_kernel_cases as C
import _zinb_edge_grid as E


@pytest.fixture(scope='module')
def ops():
    return CpuRefOps()


def test_tol_is_four_times_the_measured_fp32_error():
    """TOL of the shared cases = 4 x the worst relative error of the kernels' fp32 restatement against the fp64 oracle."""
    m = C.measure_f32()
    worst = max(max(v) for v in m.values())
    print({k: '%.3g | %.3g' % v for k, v in m.items()}, 'worst %.4g' % worst, 'TOL %.4g' % C.TOL)
    assert 4 * worst <= C.TOL <= 4.1 * worst, (worst, C.TOL)


@pytest.mark.parametrize('kind', C.KINDS)
def test_optimizer_three_steps(ops, kind):
    C.optimizer_three_steps(ops, kind)


def test_counter_add(ops):
    C.counter_add_cases(ops)


def test_rmsprop_stride_and_fused_end(ops):
    C.rmsprop_stride(ops)


def test_rmsprop_end_null_words(ops):
    C.rmsprop_end_null_words(ops)


def test_l1l2_apply(ops):
    C.l1l2_cases(ops)


@pytest.mark.parametrize('ridge', E.RIDGES)
@pytest.mark.parametrize('flags', [1, 3, 0])
def test_oracle_gradients_stay_inside_the_plane_range_bound(flags, ridge):
    """|g| <= max(1e4, 2 y + 50) + ridge / 2 element-wise for the fp64 oracle on the whole edge grid, extended to
    y = 16 000, with no exclusions: what d_exp = floor(log2(65000 / bound)) of Engine._data_scales rests on."""
    worst = E.worst_bound_ratio(flags, ridge, E.Y + (16000.,))
    print('flags', flags, 'ridge', ridge, 'worst |g| / bound = %.6f' % worst)
    assert worst <= 1.0
