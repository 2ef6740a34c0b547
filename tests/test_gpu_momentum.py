"""The two kernels of ann3depth_amd/csrc/optim.hip (include/a3d_optim.h) held bit for bit: a3do_momentum_apply to the numpy
restatement of the rule (tests/momentum_ref.py) at the sizes that cut its vector body, its grid-stride loop and its scalar tail,
and a3do_dense_bwd_filter_momentum to the two-call form it replaces (a3d_dense_bwd_filter into a scratch gradient, then
a3do_momentum_apply on kernel and bias), and, on small-integer operands whose every float32 sum is exact, element by element to
the float64 form of the rule.  Every tensor a kernel writes is a window of a larger allocation filled with a sentinel."""
import numpy as np
import pytest
import torch

import exact_ops as E
import momentum_ref as MR
from test_gpu_pointwise import Guarded, assert_same_f32, dev

pytestmark = pytest.mark.gpu

BIG = 4096 * 256 * 4 + 3             # a second trip of the grid-stride loop (4096 blocks x 256 vectors) and a scalar tail of 3
SETTINGS = [(0.1, 0.9), (0.125, 0.5), (0.0, 0.9), (0.1, 0.0)]      # (lr, momentum)


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


class Pair:
    """The same var / accum on the device (guarded windows) and on the host."""

    def __init__(self, var, accum):
        self.var, self.accum = var.copy(), accum.copy()
        self.bufs = [Guarded(var.size) for _ in range(3)]                    # var, accum, g
        self.bufs[0].t.copy_(dev(var))
        self.bufs[1].t.copy_(dev(accum))

    def step(self, ops, g, lr, mu, scale):
        self.var, self.accum = MR.step(self.var, self.accum, g, lr, mu, scale)
        self.bufs[2].t.copy_(dev(g))
        ops.momentum_apply(self.bufs[0].t, self.bufs[1].t, self.bufs[2].t, lr, mu, scale)

    def check(self, g):
        assert_same_f32(self.bufs[1].host(), self.accum)
        assert_same_f32(self.bufs[0].host(), self.var)
        assert_same_f32(self.bufs[2].host(), g)                              # the gradient is read only; the guards are checked


@pytest.mark.parametrize('scale', [1.0, 0.125, 1 / 3])
@pytest.mark.parametrize('count', [1, 2, 3, 5, 4003, BIG])
def test_momentum_apply_bit_for_bit(ops, count, scale):
    """Three steps at every (lr, momentum): counts below one vector, the scalar tail, the grid-stride loop, grad_scale first."""
    rng = np.random.default_rng(count)
    for lr, mu in SETTINGS:
        pair = Pair(rng.standard_normal(count).astype(np.float32), rng.standard_normal(count).astype(np.float32))
        for _ in range(3):
            g = rng.standard_normal(count).astype(np.float32)
            pair.step(ops, g, lr, mu, scale)
            pair.check(g)


def test_momentum_apply_has_no_special_cases(ops):
    """NaN, +-inf, -0 and a denormal in each of var, accum and g: the arithmetic alone decides every bit (any NaN is any NaN)."""
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41], np.float32)
    rng = np.random.default_rng(11)
    count = 3 * special.size * 4 + 3
    var, accum, g = (rng.standard_normal(count).astype(np.float32) for _ in range(3))
    for i, a in enumerate((var, accum, g)):
        a[i * special.size:(i + 1) * special.size] = special                 # in the vector body ...
        a[count - 3 + i % 3] = special[i]                                    # ... and in the scalar tail
    g[3 * special.size:4 * special.size] = special                           # a special gradient onto plain state
    var[3 * special.size + 1], accum[3 * special.size + 2] = np.inf, -np.inf   # inf - inf on both lines of the rule
    for lr, mu in SETTINGS:
        for scale in (1.0, 0.125):
            pair = Pair(var, accum)
            pair.step(ops, g, lr, mu, scale)
            pair.check(g)
            assert np.isnan(pair.var).any() and np.isinf(pair.accum).any()


def test_momentum_on_a_slice_leaves_the_rest_alone(ops):
    """A data-parallel rank's call: [a, b) of the group's flat buffers, a a multiple of 64."""
    rng = np.random.default_rng(64)
    total, a, b = 1024, 128, 128 + 4 * 64 + 3
    state = [rng.standard_normal(total).astype(np.float32) for _ in range(3)]
    bufs = [dev(s) for s in state]
    var, accum = MR.step(state[0][a:b], state[1][a:b], state[2][a:b], 0.1, 0.9, 0.5)
    ops.momentum_apply(bufs[0][a:b], bufs[1][a:b], bufs[2][a:b], 0.1, 0.9, 0.5)
    want = [s.copy() for s in state]
    want[0][a:b], want[1][a:b] = var, accum
    for got, w in zip(bufs, want):
        assert_same_f32(got.cpu().numpy(), w)


def test_momentum_apply_refusals(ops):
    from ann3depth_amd._lib import A3dError
    t = torch.zeros(64, device='cuda')
    with pytest.raises(ValueError):
        ops.momentum_apply(t, t[:32], t, 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.momentum_apply(t[:0], t[:0], t[:0], 0.1, 0.9)
    with pytest.raises(TypeError):
        ops.momentum_apply(t, t.double(), t, 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.momentum_apply(t[::2], t[:32], t[:32], 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.momentum_apply(t, t.cpu(), t, 0.1, 0.9)
    with pytest.raises(A3dError):
        ops.momentum_apply(t[1:33], t[:32], t[:32], 0.1, 0.9)                 # 4 bytes off the 16-byte grid


# ---------------------------------------------------------------------------------------------- the fused launch
class Layer:
    """var_w, accum_w [k, n] and var_b, accum_b [n] of one dense layer in guarded windows."""

    def __init__(self, state, k, n):
        self.k, self.n = k, n
        self.bufs = [Guarded(a.size) for a in state]
        for buf, a in zip(self.bufs, state):
            buf.t.copy_(dev(a.ravel()))

    def tensors(self):
        k, n = self.k, self.n
        return [self.bufs[0].view(k, n), self.bufs[1].view(k, n), self.bufs[2].t, self.bufs[3].t]

    def host(self):
        return [b.host() for b in self.bufs]


def two_calls(ops, x, dz, layer, lr, mu, scale, bias=True):
    k, n = layer.k, layer.n
    dw, db = torch.empty((k, n), device='cuda'), torch.empty(n, device='cuda')
    ops.dense_bwd_filter(x, dz, dw, db if bias else None)
    var_w, acc_w, var_b, acc_b = layer.tensors()
    ops.momentum_apply(var_w, acc_w, dw, lr, mu, scale)
    if bias:
        ops.momentum_apply(var_b, acc_b, db, lr, mu, scale)


def layer_state(rng, k, n):
    return [rng.standard_normal((k, n)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)]


def run_both(ops, m, k, n, scale, bias=True, plant=None, lr=0.1, mu=0.9):
    rng = np.random.default_rng(1000 * m + k + n)
    x = rng.standard_normal((m, k)).astype(np.float32)
    dz = rng.standard_normal((2, m, n)).astype(np.float32)
    if plant is not None:
        dz[1, m - 1, min(3, n - 1)] = plant
    state = layer_state(rng, k, n)
    fused, plain = Layer(state, k, n), Layer(state, k, n)
    xd = dev(x)
    for step in range(2):
        dzd = dev(dz[step])
        var_w, acc_w, var_b, acc_b = fused.tensors()
        ops.dense_bwd_filter_momentum(xd, dzd, var_w, acc_w, var_b if bias else None, acc_b if bias else None, lr, mu, scale)
        two_calls(ops, xd, dzd, plain, lr, mu, scale, bias)
        pairs = list(zip(('var_w', 'accum_w', 'var_b', 'accum_b'), fused.host(), plain.host()))
        for name, a, b in pairs:               # every figure first
            print(f'm {m} k {k} n {n} scale {scale} step {step} {name}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} of '
                  f'{a.size} bit patterns differ')
        for name, a, b in pairs:
            assert_same_f32(a, b)
    return fused.host(), state


# (33, 67): one partial row group and an odd n, so the rows are 4-byte aligned only and the last lanes partly out of range;
# (130, 128): a second block of rows with empty waves, full columns; (256, 70)
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('k,n', [(33, 67), (130, 128), (256, 70)])
@pytest.mark.parametrize('m', [1, 31, 32, 33, 64])
def test_fused_launch_equals_the_two_calls(ops, m, k, n, scale):
    """Two consecutive steps, bit for bit in var_w, accum_w, var_b and accum_b.  Here k n < 2^16, where a3d_dense_bwd_filter is
    the implicit-GEMM route: the fused kernel feeds the batch rows in that route's order (with the dense kernels' ascending order
    53-68 % of accum_w differed in the last bits at every m > 1, the biases never)."""
    got, state = run_both(ops, m, k, n, scale)
    assert not any(np.array_equal(g, s.ravel()) for g, s in zip(got, state))      # everything moved


# The same edges where a3d_dense_bwd_filter is the dense kernel itself (k n >= 2^16): (1000, 67) an odd n, rows 4-byte aligned
# only, a last lane with one column, a last row group of 8 rows; (130, 512): a second block of rows with three empty waves, full
# columns; (1028, 70): a last column block of 6 columns, a last row group of 4 rows
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('k,n', [(1000, 67), (130, 512), (1028, 70)])
@pytest.mark.parametrize('m', [1, 31, 32, 33, 64])
def test_fused_launch_equals_the_two_calls_of_the_dense_kernels(ops, m, k, n, scale):
    assert k * n >= 1 << 16
    got, state = run_both(ops, m, k, n, scale)
    assert not any(np.array_equal(g, s.ravel()) for g, s in zip(got, state))


def test_fused_launch_with_an_infinite_gradient(ops):
    got, _ = run_both(ops, 33, 130, 512, 0.5, plant=np.inf)
    assert all(np.isinf(g).any() or np.isnan(g).any() for g in got)


def test_fused_launch_without_a_bias(ops):
    got, state = run_both(ops, 31, 1000, 67, 1.0, bias=False)
    assert_same_f32(got[2], state[2])
    assert_same_f32(got[3], state[3])


def test_fused_launch_at_the_layers_own_widths(ops):
    """dense_1's row length (4070: 8-byte rows) and a 16-byte one."""
    run_both(ops, 32, 384, 520, 0.5)
    run_both(ops, 5, 130, 4070, 1.0)


def test_fused_launch_refusals(ops):
    from ann3depth_amd._lib import A3dError
    x, dz = torch.zeros((65, 8), device='cuda'), torch.zeros((65, 4), device='cuda')
    w, b = torch.zeros((8, 4), device='cuda'), torch.zeros(4, device='cuda')
    with pytest.raises(A3dError, match='a3d_dense_bwd_filter and a3do_momentum_apply'):
        ops.dense_bwd_filter_momentum(x, dz, w, w.clone(), b, b.clone(), 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.dense_bwd_filter_momentum(x[:4], dz[:4], w, w.clone(), b, None, 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.dense_bwd_filter_momentum(x[:4], dz[:5], w, w.clone(), b, b.clone(), 0.1, 0.9)
    with pytest.raises(ValueError):
        ops.dense_bwd_filter_momentum(x[:4], dz[:4], w[:4], w.clone(), b, b.clone(), 0.1, 0.9)
    with pytest.raises(TypeError):
        ops.dense_bwd_filter_momentum(x[:4], dz[:4], w, w.double(), b, b.clone(), 0.1, 0.9)


EXACT_LR, EXACT_MU, EXACT_SCALE = 0.25, 0.5, 0.5      # powers of two


@pytest.mark.parametrize('m,k,n', [s for s in E.DENSE if s[0] <= 64] + [(3, 1, 1), (33, 33, 67), (64, 130, 128)])
def test_fused_launch_on_exact_integers(ops, m, k, n):
    """Ternary operands (exact_ops.dense_case): the gradient is an integer below 2^24 in any summation order.  With lr, momentum
    and grad_scale powers of two and small-integer state, two steps stay multiples of 1/64 whose 64-fold is below 2^24 (asserted):
    every float32 operation of the rule is exact, and the results equal the float64 form element by element."""
    cs = E.dense_case(m, k, n)
    rng = np.random.default_rng(m + k + n)
    state = [rng.integers(-8, 9, s).astype(np.float32) for s in ((k, n), (k, n), (n,), (n,))]
    layer = Layer(state, k, n)
    want = [E.f64(a).ravel() for a in state]
    for step, dz in enumerate((cs.dz, np.roll(cs.dz, (1, 3), axis=(0, 1)))):
        g_w, g_b = (E.f64(cs.x).T @ E.f64(dz)).ravel(), E.f64(dz).sum(0)
        assert max(E.amax(g_w), E.amax(g_b)) < E.F32_EXACT
        want[0], want[1] = MR.step64(want[0], want[1], g_w, EXACT_LR, EXACT_MU, EXACT_SCALE)
        want[2], want[3] = MR.step64(want[2], want[3], g_b, EXACT_LR, EXACT_MU, EXACT_SCALE)
        for a in want:                                # what makes every operation exact
            E.require_integers(f'{cs.what} step {step} x 64', 64 * a)
            assert 64 * E.amax(a) < E.F32_EXACT
        var_w, acc_w, var_b, acc_b = layer.tensors()
        ops.dense_bwd_filter_momentum(dev(cs.x), dev(dz), var_w, acc_w, var_b, acc_b, EXACT_LR, EXACT_MU, EXACT_SCALE)
        for got, w in zip(layer.host(), want):
            np.testing.assert_array_equal(got.astype(np.float64), w)
