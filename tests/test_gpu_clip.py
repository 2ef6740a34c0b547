"""The kernels of ann3depth_amd/csrc/clip.hip (include/a3d_clip.h).  a3dn_grad_norm_scale: the float64 sum of squares bit for
bit on integer-valued gradients (every order of addition is exact there) at the counts that cut its vectors, its tail, its
blocks and its capped grid, with a single non-zero at every seam; the scale's exact cases; norm and scale within one float32 ulp
of tests/clip_ref.py on random gradients, the same bits from run to run; the skip on NaN and +-inf.  The four *_ctl applies: bit
for bit the existing entry points called with the scale read back, and not one byte written on a skip.  Every tensor a kernel
reads or writes is a window of a larger allocation filled with a sentinel."""
import numpy as np
import pytest
import torch

import clip_ref as CR
from ann3depth_amd import _lib
from test_gpu_pointwise import Guarded, assert_same_f32, dev

pytestmark = pytest.mark.gpu

BLOCK, CAP = _lib.CLIP_BLOCK_ELEMS, _lib.CLIP_MAX_BLOCKS      # floats of a block's one sweep; the grid's cap (include/a3d_clip.h)
SWEEP = BLOCK * CAP                                           # 2^22: from here on a block takes more than BLOCK floats
COUNTS = [1, 2, 3, 4, 5, 7, 1021, 1024, 1025, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 4, 3 * BLOCK + 4 * 5 + 2, SWEEP + 5]
FMAX = np.finfo(np.float32).max


def blocks_of(count):
    """(blocks, vectors per block) of the launch, restated from the header."""
    nvec = count // 4
    grid = min(CAP, max(1, -(-nvec // (BLOCK // 4))))
    return grid, -(-nvec // grid)


def placements(count):
    """Element 0, the last element of the vector body, the first tail element, the last element, and both sides of every kind of
    block seam the count has (the first, and the last block's)."""
    grid, per = blocks_of(count)
    body = count // 4 * 4
    at = {0, count - 1}
    if body:
        at.add(body - 1)
    if body < count:
        at.add(body)
    if grid > 1:
        at |= {4 * per - 1, 4 * per, 4 * per * (grid - 1) - 1, min(4 * per * (grid - 1), count - 1)}
    return sorted(at)


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


class Norm:
    """One control block and one workspace, as a ParamGroup owns them."""

    def __init__(self, ops, most=SWEEP + 5):
        self.ops, self.ctl, self.ws = ops, ops.clip_ctl('cuda'), ops.grad_norm_ws(most, 'cuda')

    def __call__(self, g, gs=1.0, C=np.inf):
        buf = g if isinstance(g, Guarded) else Guarded(g.size)
        if buf is not g:
            buf.t.copy_(dev(g))
        self.ops.grad_norm_scale(buf.t, gs, C, self.ctl, self.ws)
        st = self.ops.clip_read(self.ctl)
        assert int(self.ws[0]) == 0, 'the ticket wraps to 0'
        if buf is not g:
            assert_same_f32(buf.host(), g)                                   # read only, and the guards are whole
        return st


def bits(x):
    return np.float32(x).view(np.uint32)


def within_one_ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return np.nextafter(want, np.float32(-np.inf)) <= got <= np.nextafter(want, np.float32(np.inf))


# ---------------------------------------------------------------------------------------------- exact S
@pytest.fixture(scope='module')
def integers():
    """Integer-valued float32 in [-2^10, 2^10]: S < 2^22 * 2^20 < 2^53, every order of addition is exact."""
    return np.random.default_rng(1).integers(-1024, 1025, SWEEP + 5).astype(np.float32)


@pytest.mark.parametrize('count', COUNTS)
def test_sumsq_is_exact_on_integers(ops, integers, count):
    g = integers[-count:]
    st = Norm(ops, count)(g)
    want = CR.clip(g, 1.0, np.inf)
    assert want.sumsq == float(np.sum(g.astype(np.int64) ** 2)) < 2.0 ** 53
    assert st.sumsq == want.sumsq and (st.skip, st.skipped) == (0, 0)
    assert bits(st.norm) == bits(want.norm) and bits(st.scale) == bits(1.0)


@pytest.mark.parametrize('count', COUNTS)
def test_a_single_non_zero_is_found_wherever_it_lies(ops, count):
    norm = Norm(ops, count)
    buf = Guarded(count)
    for k, at in enumerate(placements(count)):
        x = np.float32(3 + k)
        buf.t.zero_()
        buf.t[at] = float(x)
        st = norm(buf)
        assert st.sumsq == float(x) ** 2 and bits(st.norm) == bits(x) and st.skip == 0, (count, at)
    buf.host()


# ---------------------------------------------------------------------------------------------- exact scale
def test_scale_exact_cases(ops):
    norm = Norm(ops, 1 << 12)
    g = np.zeros(37, np.float32)
    g[0], g[1] = 3, 4
    assert bits(norm(g, 1.0, 5.0).scale) == bits(1.0)                        # equality does not clip
    assert bits(norm(g, 1.0, 2.5).scale) == bits(0.5)
    below = np.nextafter(np.float32(5), np.float32(0))
    st = norm(g, 1.0, below)
    assert st.scale < 1 and bits(st.scale) == bits(CR.clip(g, 1.0, below).scale)
    assert bits(norm(g, 1.0, np.inf).scale) == bits(1.0)
    for gs in (0.5, 0.125):
        st = norm(g, gs, np.inf)
        assert bits(st.scale) == bits(gs) and bits(st.norm) == bits(5 * gs) and st.sumsq == 25.0
        assert bits(norm(g, gs, 5 * gs).scale) == bits(gs)                    # n == C
        assert bits(norm(g, gs, 2.5 * gs).scale) == bits(gs / 2)
        assert bits(norm(g, -gs, 2.5 * gs).scale) == bits(-gs / 2)            # n is |gs| sqrt(S); the sign stays in the scale
    for j, v in ((0, 7.0), (1, -3.0), (3, 0.75), (5, 1.5), (6, -0.125)):
        g = np.full(4 ** j, v, np.float32)
        st = norm(g, 1.0, abs(v))                                             # n = 2^j |v| exactly
        assert bits(st.norm) == bits(2 ** j * abs(v)) and bits(st.scale) == bits(1.0 if j == 0 else 2.0 ** -j), (j, v)
        assert bits(norm(g, 1.0, np.inf).scale) == bits(1.0)
    assert norm(np.zeros(9, np.float32), 1.0, 1.0)[:4] == (0.0, 0.0, 1.0, 0)  # nothing to clip in a zero gradient


# ---------------------------------------------------------------------------------------------- random gradients
def mixed(count, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(count) * 10.0 ** rng.uniform(-30, 30, count)).astype(np.float32)
    g[rng.integers(0, count, max(1, count // 16))] = np.float32(1e-41) * rng.integers(-9, 10, max(1, count // 16))   # denormals
    return g


@pytest.mark.parametrize('count', [5, 1025, BLOCK + 4, 3 * BLOCK + 4 * 5 + 2, SWEEP + 5])
def test_random_gradients_within_one_ulp_and_the_same_bits_every_run(ops, count):
    """A float64 sum of <= 2^27 non-negative terms is within 2^-26 relative of the exact sum in any order, so n = |gs| sqrt(S) is
    within 2^-26 of the reference's: one float32 ulp once both are rounded."""
    norm, other = Norm(ops), np.ones(2 * BLOCK + 3, np.float32)
    for seed, gs in ((count, 1.0), (count + 1, 0.5)):
        g = mixed(count, seed)
        n = float(np.sqrt(CR.sumsq(g))) * gs
        for C in (np.inf, n / 3, 1e-3):
            want = CR.clip(g, gs, C)
            st = norm(g, gs, C)
            assert abs(st.sumsq - want.sumsq) <= 2.0 ** -26 * want.sumsq and st.skip == 0
            assert within_one_ulp(st.norm, want.norm) and within_one_ulp(st.scale, want.scale), (C, st, want)
            norm(other, 1.0, 1.0)                                             # another count through the same workspace
            assert norm(g, gs, C) == st == Norm(ops, count)(g, gs, C)         # and a fresh one: the same bits


def test_denormals_and_values_near_the_largest(ops):
    norm = Norm(ops, 1 << 12)
    tiny = np.full(1027, 1e-41, np.float32)                                   # every square is far below float32, not below float64
    st, want = norm(tiny, 1.0, 1e-44), CR.clip(tiny, 1.0, 1e-44)
    assert want.sumsq > 0 and abs(st.sumsq - want.sumsq) <= 2.0 ** -26 * want.sumsq
    assert within_one_ulp(st.norm, want.norm) and within_one_ulp(st.scale, want.scale) and st.scale < 1
    huge = np.full(1027, FMAX, np.float32)
    huge[5], huge[1026] = -FMAX, np.float32(0.9) * FMAX
    for gs, C in ((1.0, 1.0), (0.5, np.inf), (1.0, FMAX)):
        st, want = norm(huge, gs, C), CR.clip(huge, gs, C)
        assert np.isinf(st.norm) and np.isfinite(st.sumsq) and (st.skip, st.skipped) == (0, 0)      # inf as reported is no skip
        assert within_one_ulp(st.scale, want.scale) and (0 < st.scale < 1 or C == np.inf)


# ---------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize('count', [1, 5, 1025, BLOCK + 4, 3 * BLOCK + 4 * 5 + 2, SWEEP + 5])
def test_a_non_finite_element_anywhere_skips_and_counts_once(ops, integers, count):
    norm = Norm(ops, count)
    buf = Guarded(count)
    buf.t.copy_(dev(integers[:count]))
    skipped = 0
    for k, at in enumerate(placements(count)):
        bad = (np.nan, np.inf, -np.inf)[k % 3]
        for C in ((1.0, np.inf) if k < 3 else (1.0,)):
            keep = float(buf.t[at])
            buf.t[at] = bad
            st = norm(buf, 0.5, C)
            skipped += 1
            assert (st.skip, st.skipped) == (1, skipped) and bits(st.scale) == bits(0.0) and not np.isfinite(st.sumsq), (at, bad)
            assert not np.isfinite(st.norm)
            buf.t[at] = keep
            st = norm(buf, 0.5, C)                                            # a finite call afterwards
            assert (st.skip, st.skipped) == (0, skipped) and st.sumsq == CR.sumsq(integers[:count]) and st.scale > 0
    buf.host()


# ---------------------------------------------------------------------------------------------- the four rules under a control block
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41], np.float32)
APPLY_COUNTS = [1, 3, 4, 5, 1027]


def laden(count, seed, n):
    """n arrays of `count` values with the special values in the vector body and in the scalar tail, as tests/test_gpu_momentum.py
    places them (where the count has the room)."""
    rng = np.random.default_rng(seed)
    arrays = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    if count >= n * SPECIAL.size * 4 + 3:
        for i, a in enumerate(arrays):
            a[i * SPECIAL.size:(i + 1) * SPECIAL.size] = SPECIAL
            a[count - 3 + i % 3] = SPECIAL[i % SPECIAL.size]
    elif count > 1:
        arrays[-1][count - 1] = np.inf                                         # the gradient's last element
    return arrays


def controls(ops, count):
    """[(control block, its state)]: scale exactly 1, a scale that is no power of two, and a skip — each left by a norm launch."""
    rng = np.random.default_rng(77)
    clean = rng.standard_normal(max(count, 9)).astype(np.float32)
    out = []
    for g, C in ((clean, np.inf), (clean, float(np.sqrt(CR.sumsq(clean))) / 3), (np.append(clean, np.float32(np.nan)), 1.0)):
        norm = Norm(ops, g.size)
        st = norm(g, 1.0, C)
        out.append((norm.ctl, st))
    assert bits(out[0][1].scale) == bits(1.0) and 0.3 < out[1][1].scale < 0.34 and out[2][1].skip == 1
    return out


def windows(arrays):
    bufs = [Guarded(a.size) for a in arrays]
    for b, a in zip(bufs, arrays):
        b.t.copy_(dev(a))
    return bufs


def assert_windows_equal(got, want):
    """Bit for bit, the guards included; any NaN matches any NaN, as everywhere in these tests."""
    for a, b in zip(got, want):
        assert_same_f32(a.big.cpu().numpy(), b.big.cpu().numpy())


def assert_windows_untouched(got, want):
    for a, b in zip(got, want):
        assert torch.equal(a.big.view(torch.int32), b.big.view(torch.int32))   # every byte


@pytest.mark.parametrize('count', APPLY_COUNTS)
def test_momentum_ctl_is_the_existing_rule_at_the_scale_read_back(ops, count):
    arrays = laden(count, count, 3)                                            # var, accum, g
    for ctl, st in controls(ops, count):
        new, old, untouched = windows(arrays), windows(arrays), windows(arrays)
        ops.momentum_apply_ctl(new[0].t, new[1].t, new[2].t, 0.1, 0.9, ctl)
        if st.skip:
            assert_windows_untouched(new, untouched)
            continue
        ops.momentum_apply(old[0].t, old[1].t, old[2].t, 0.1, 0.9, float(st.scale))
        assert_windows_equal(new, old)
        var, accum = CR.momentum(*arrays, 0.1, 0.9, CR.Clip(0.0, 0.0, st.scale, 0))
        assert_same_f32(new[0].host(), var)
        assert_same_f32(new[1].host(), accum)
        assert not torch.equal(new[0].big, untouched[0].big)


@pytest.mark.parametrize('beta2', [0.999, 1.0], ids=['general', 'frozen'])
@pytest.mark.parametrize('count', APPLY_COUNTS)
def test_adam_ctl_is_the_existing_rule_at_the_scale_read_back(ops, count, beta2):
    arrays = laden(count, 10 + count, 4)                                       # var, m, v, g
    arrays[2] = np.abs(arrays[2])
    hyper = (0.1, 0.9, beta2, 1e-8, 0.9, beta2)                                # the first step's beta powers
    for ctl, st in controls(ops, count):
        new, old, untouched = windows(arrays), windows(arrays), windows(arrays)
        flags = torch.zeros(3, dtype=torch.int32, device='cuda')
        ops.adam_apply_tf1_ctl(*(w.t for w in new), *hyper, ctl, poisoned=flags[0:1])
        if st.skip:
            assert_windows_untouched(new, untouched)
            assert flags.tolist() == [0, 0, 0]                                 # not `poisoned` either, NaN-laden gradient or not
            continue
        ops.adam_apply_tf1(*(w.t for w in old), *hyper, float(st.scale), poisoned=flags[1:2])
        assert_windows_equal(new, old)
        assert int(flags[0]) == int(flags[1]) and int(flags[2]) == 0
        assert not torch.equal(new[1].big, untouched[1].big)                   # m moved under either kernel


@pytest.mark.parametrize('floor', [None, 0.0], ids=['plain', 'floored'])
@pytest.mark.parametrize('count', APPLY_COUNTS)
def test_sgd_ctl_is_the_existing_rule_at_the_rate_lr_times_scale(ops, count, floor):
    arrays = laden(count, 20 + count, 2)                                       # var, g
    for ctl, st in controls(ops, count):
        new, old, untouched = windows(arrays), windows(arrays), windows(arrays)
        ops.sgd_apply_ctl(new[0].t, new[1].t, 0.1, ctl, floor=floor)
        if st.skip:
            assert_windows_untouched(new, untouched)
            continue
        lr = float(np.float32(0.1) * np.float32(st.scale))                     # one float32 product
        if floor is None:
            ops.sgd_apply(old[0].t, old[1].t, lr)
        else:
            ops.sgd_apply_floor(old[0].t, old[1].t, lr, floor)
        assert_windows_equal(new, old)
        assert_same_f32(new[0].host(), CR.sgd(*arrays, 0.1, CR.Clip(0.0, 0.0, st.scale, 0), floor=floor))


def test_python_layer_refusals(ops):
    from ann3depth_amd._lib import A3dError
    t = torch.zeros(64, device='cuda')
    ctl, ws = ops.clip_ctl('cuda'), ops.grad_norm_ws(64, 'cuda')
    assert ctl.numel() * 8 == _lib.CLIP_CTL_BYTES and not ctl.any() and not ws.any()
    for gs, C in ((0.0, 1.0), (np.inf, 1.0), (np.nan, 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, np.nan)):
        with pytest.raises(ValueError):
            ops.grad_norm_scale(t, gs, C, ctl, ws)
    with pytest.raises(ValueError):
        ops.grad_norm_scale(t[:0], 1.0, 1.0, ctl, ws)
    with pytest.raises(TypeError):
        ops.grad_norm_scale(t.double(), 1.0, 1.0, ctl, ws)
    with pytest.raises(TypeError):
        ops.grad_norm_scale(t, 1.0, 1.0, ctl[:2], ws)
    with pytest.raises(TypeError):
        ops.grad_norm_scale(t, 1.0, 1.0, ctl, ws.int())
    with pytest.raises(ValueError):
        ops.grad_norm_scale(t, 1.0, 1.0, ctl.cpu(), ws)
    with pytest.raises(A3dError, match='16-byte aligned'):
        ops.grad_norm_scale(t[1:33], 1.0, 1.0, ctl, ws)
    with pytest.raises(A3dError, match='workspace bytes'):
        ops.grad_norm_scale(torch.zeros(2 * BLOCK + 4, device='cuda'), 1.0, 1.0, ctl, ws[:1])
    with pytest.raises(ValueError):
        ops.momentum_apply_ctl(t, t[:32], t, 0.1, 0.9, ctl)
    with pytest.raises(TypeError):
        ops.momentum_apply_ctl(t, t, t, 0.1, 0.9, t)
    with pytest.raises(ValueError):
        ops.sgd_apply_ctl(t, t[:32], 0.1, ctl)
    with pytest.raises(ValueError):
        ops.adam_apply_tf1_ctl(t, t, t[:32], t, 0.1, 0.9, 0.999, 1e-8, 0.9, 0.999, ctl)
    torch.cuda.synchronize()
    assert not ctl.any() and not ws.any()                                      # nothing was launched
