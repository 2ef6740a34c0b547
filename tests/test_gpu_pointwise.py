"""The HBM-bound kernels of ann3depth_amd/csrc/pointwise.hip, pool.hip and resample.hip held to exact host references at
their edges: tails of the
vector bodies, grid-stride loops past the launch's block cap, pitches wider than the channel count, odd sizes, ties,
signed zeros, denormals, non-finite values.  Every comparison is bit-exact (values, or the uint16 / uint8 bits) except the
loss and its gradient, which keep the 2e-6 / 1e-5 of tests/test_gpu_ops.py::test_silog_loss against the float64 oracle.
Every output tensor is a window of a larger allocation filled with a sentinel: pad channels, pad columns and the elements
before and after the tensor must keep it.  References: oracle/tf13_ops.py (T) and tests/pointwise_ref.py (R), the latter
pinned on the CPU by tests/test_pointwise_ref.py.

That the file bites was checked with mutated copies of the sources, one value changed per build (never an index, bound
or stride), bound through A3D_LIB; each made the tests named here fail and no other (kernels under the names they had
then: maxpool_bwd_bf16_kernel is now maxpool_bwd_kernel<__bf16>, the bf16 -> fp32 idx form maxpool_bwd_idx_kernel<__bf16>):
  a Philox multiplier; k1 += the other Weyl constant; c[j] >> 9; step_lo / step_hi swapped
                                                   -> test_dropout_keep_mask_is_the_philox_stream_of_its_contract (all 8),
                                                      _seed_and_step_use_all_64_bits, _rates (all 3)
  floorf(keep_prob + u) again (a byte of 2)        -> test_dropout_keep_mask_at_rate_zero_writes_ones_only
  v1 >= best in maxpool_bwd_bf16_kernel            -> test_maxpool2x2_bwd_bf16_against_the_oracle (7 of 8; 2 x 2 x 2 x 1 has no tie there)
  e & 1 halves swapped in the bf16 -> bf16 idx form -> test_maxpool2x2_bwd_idx_routes_by_the_argmax_byte[bf16_bf16-*] (all 6)
  relu_mask ignored in the bf16 -> fp32 idx form   -> test_maxpool2x2_bwd_idx_routes_by_the_argmax_byte[bf16_f32-*] (all 10)
  (__bf16)g -> truncation in silog_bwd_kernel      -> test_silog_loss_and_gradient_at_the_shapes_that_cut_its_loops (6 of 7),
                                                      test_silog_gradient_of_a_sample_that_holds_a_minus_infinite_log
  inv_b dropped                                    -> the same, and test_silog_loss_bwd_plain_entry_point (b = 1 cannot see it)
  the arrival ticket at ws[2b] again               -> test_silog_workspace_serves_another_batch_size_in_between
  gscale ignored in adam_kernel's scalar tail      -> test_adam_apply_tf1_bit_for_bit[*-0.125 | 1/3-0.999] (all 4),
                                                      test_adam_on_a_slice_leaves_the_rest_alone[0.999]
  bad |= !isfinite(var) again in adam_kernel       -> test_adam_poisoned_flag_means_the_update_turned_something_non_finite[0.999]
  the scalar tail of cast_bf16_kernel writing +0   -> test_cast_bf16_both_ways (every count with a tail)
  pad_t rounded up in a3d_extract_patches          -> test_extract_patches_with_uneven_padding[2-241-323-3-100-40]"""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_ref as R
from oracle import tf13_ops as T
from test_pointwise_ref import NAN_BITS, SPECIAL_BITS

pytestmark = pytest.mark.gpu

SENT = 7.0                       # float32 / bf16 (bits 0x40E0) sentinel; uint8 buffers use 9
BF16 = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


@pytest.fixture(scope='module')
def A3dError():
    from ann3depth_amd._lib import A3dError
    return A3dError


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev16(bits):
    """uint16 bf16 bits -> bfloat16 device tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(BF16)


def host(t):
    """Device tensor -> numpy; bfloat16 as its uint16 bits."""
    if t.dtype == BF16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


class Guarded:
    """`numel` elements inside a larger allocation filled with a sentinel (`offset` elements before, `guard` after)."""

    def __init__(self, numel, dtype=torch.float32, guard=512, offset=0):
        self.sentinel = 9 if dtype == torch.uint8 else SENT
        self.big = torch.full((offset + numel + guard,), self.sentinel, dtype=dtype, device='cuda')
        self.lo, self.hi = offset, offset + numel
        self.t = self.big[self.lo:self.hi]

    def view(self, *shape):
        return self.t.view(*shape)

    def host(self, *shape):
        """The window on the host (bf16: bits), after checking that nothing around it was written."""
        a = host(self.big)
        s = host(torch.full((1,), self.sentinel, dtype=self.big.dtype))[0]
        assert (a[:self.lo] == s).all() and (a[self.hi:] == s).all(), 'a kernel wrote outside its tensor'
        a = a[self.lo:self.hi]
        return a.reshape(shape) if shape else a


SENT16 = int(R.bf16_round(np.array([SENT], np.float32))[0])


def assert_same_f32(got, want):
    """float32 arrays equal bit for bit, except that any NaN matches any NaN."""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    ok = (g == w) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f'{(~ok).sum()} of {ok.size} differ, first at {np.flatnonzero(~ok.ravel())[:5]}'


def assert_same_bf16(got_bits, want_bits):
    ok = R.same_bf16(got_bits, want_bits)
    bad = np.flatnonzero(~ok.ravel())
    assert ok.all(), (f'{bad.size} of {ok.size} differ, first at {bad[:5]}: got {np.asarray(got_bits).ravel()[bad[:5]]}, '
                      f'want {np.asarray(want_bits).ravel()[bad[:5]]}')


# ================================================================================================ dropout keep mask
def draw_mask(ops, count, seed, step, rate):
    g = Guarded(count, torch.uint8, guard=64)
    ops.dropout_keep_mask(g.t, seed, step, rate)
    return g.host()


MASK_BIG = 8192 * 256 * 4 + 4099          # past the launch's 8192 blocks x 256 quads, and a last quad of 3 bytes


@pytest.mark.parametrize('count', [1, 2, 3, 4, 5, 4095, 32 * 4096, MASK_BIG])
def test_dropout_keep_mask_is_the_philox_stream_of_its_contract(ops, count):
    """a3d_dropout_keep_mask (dropout_mask_kernel) against R.keep_mask: counter (q lo, q hi, step lo, step hi), key (seed lo,
    seed hi), word i % 4, 24 bits; tails of 1..3 bytes, the grid-stride loop, the byte after `count` untouched."""
    got = draw_mask(ops, count, 3000, 2, 0.5)
    np.testing.assert_array_equal(got, R.keep_mask(count, 3000, 2, 0.5))
    assert set(np.unique(got)) <= {0, 1}
    np.testing.assert_array_equal(draw_mask(ops, count, 3000, 2, 0.5), got)                 # same call, same bytes


def test_dropout_keep_mask_seed_and_step_use_all_64_bits(ops):
    count = 4099
    keys = [(3000, 2), (4000, 2), (3000, 3), (3000 + 2 ** 32, 2), (3000, 2 + 2 ** 32), (2 ** 63 + 5, 2 ** 40 + 7),
            (2 ** 64 - 1, 2 ** 64 - 1)]
    masks = []
    for seed, step in keys:
        got = draw_mask(ops, count, seed, step, 0.5)
        np.testing.assert_array_equal(got, R.keep_mask(count, seed, step, 0.5), err_msg=f'seed {seed} step {step}')
        masks.append(got)
    for i in range(len(masks)):
        for j in range(i):
            # 4099 fair bits: two independent masks differ in about half, 5 sigma = 0.04
            assert abs((masks[i] != masks[j]).mean() - 0.5) < 5 * np.sqrt(0.25 / count), (keys[i], keys[j])


@pytest.mark.parametrize('rate', [0.5, 0.25, 0.9])
def test_dropout_keep_mask_rates(ops, rate):
    count = 32 * 4096
    got = draw_mask(ops, count, 3000, 7, rate)
    np.testing.assert_array_equal(got, R.keep_mask(count, 3000, 7, rate))
    p = 1 - rate
    assert abs(got.mean() - p) < 5 * np.sqrt(p * (1 - p) / count)


def test_dropout_keep_mask_at_rate_zero_writes_ones_only(ops):
    """keep_prob = 1 and u = 1 - 2^-24 round to fl(1 + u) = 2: seed 3000 (the product's default), step 2 draws that u at
    element 3768265, where floor() would write a byte of 2.  The header's mask is {0, 1}."""
    i = 3768265
    count = i + 7
    ref = R.keep_mask(count, 3000, 2, 0.0)
    assert R.keep_mask(count, 3000, 2, 0.0, form='floor')[i] == 2 and ref[i] == 1
    got = draw_mask(ops, count, 3000, 2, 0.0)
    assert got[i] == 1
    np.testing.assert_array_equal(got, ref)
    assert (got == 1).all()


def test_dropout_keep_mask_refuses_bad_rates(ops, A3dError):
    g = Guarded(16, torch.uint8)
    for rate in (1.0, -0.125, 1.5, float('nan')):
        with pytest.raises(A3dError):
            ops.dropout_keep_mask(g.t, 3000, 0, rate)
    assert (g.host() == 9).all()


# ================================================================================================ scale-invariant log loss
def loss_inputs(b, npix, seed=11):
    rng = np.random.default_rng(seed + b * 100003 + npix)
    o = (rng.standard_normal((b, npix)) * 0.05).astype(np.float32)          # about half negative -> NaN-masked logs
    t = (rng.integers(0, 256, (b, npix)) / 255).astype(np.float32)          # contains exact zeros
    return o, t


def run_loss(ops, o, t, ws=None, ld16=None):
    """loss bits, gradient, bf16 gradient bits (or None) of one forward + backward; outputs guarded."""
    b, npix = o.shape
    od, td = dev(o), dev(t)
    ws = ops.silog_ws(b, 'cuda') if ws is None else ws
    loss = Guarded(1)
    dout = Guarded(b * npix)
    ops.silog_loss_fwd(od, td, loss.t, ws)
    d16 = None
    if ld16:
        d16 = Guarded(b * ld16, BF16)
        ops.silog_loss_bwd(od, td, ws, dout.view(b, npix), d16.view(b, ld16))
    else:
        ops.silog_loss_bwd(od, td, ws, dout.view(b, npix))
    return loss.host().copy(), dout.host(b, npix).copy(), None if d16 is None else d16.host(b, ld16).copy()


LOSS_SHAPES = [(1, 1), (3, 7), (5, 4070), (65, 4070), (64, 1023), (33, 8193), (2, 40000)]


@pytest.mark.parametrize('b,npix', LOSS_SHAPES)
def test_silog_loss_and_gradient_at_the_shapes_that_cut_its_loops(ops, b, npix):
    """a3d_silog_loss_fwd / a3d_silog_loss_bwd_ex: npix smaller than the 8 parts and not a multiple of them, b > 64 (the last
    block's loop over samples), chunk tails of the 4 x 256 unroll; the bf16 copy at a pitch of whole 16-byte pieces."""
    o, t = loss_inputs(b, npix)
    ld16 = -(-npix // 8) * 8                                                 # 4070 -> 4072, 7 -> 8
    loss, g, g16 = run_loss(ops, o, t, ld16=ld16)
    ref = T.silog_loss_fwd(o.astype(np.float64), t.astype(np.float64))
    g_ref = T.silog_loss_bwd(o.astype(np.float64), t.astype(np.float64))
    print(f'silog b={b} npix={npix}: loss rel err {abs(loss[0] - ref) / abs(ref):.2e}, grad rel-L2 {rel_l2(g, g_ref):.2e}')
    assert abs(loss[0] - ref) < 2e-6 * abs(ref)
    assert rel_l2(g, g_ref) < 1e-5
    assert (g[o < -1e-8] == 0).all()
    np.testing.assert_array_equal(g16[:, :npix], R.bf16_round(g))            # the same gradient, rounded to nearest even
    assert (g16[:, npix:] == SENT16).all()                                   # pad columns are the caller's
    loss2, g2, _ = run_loss(ops, o, t)
    assert loss2.view(np.uint32)[0] == loss.view(np.uint32)[0]               # fixed part order: the same bits
    np.testing.assert_array_equal(g2, g)


def test_silog_loss_bwd_plain_entry_point(ops):
    """a3d_silog_loss_bwd (no bf16 copy) is the same kernel: same bits as a3d_silog_loss_bwd_ex."""
    from ann3depth_amd import _lib
    o, t = loss_inputs(5, 4070)
    od, td = dev(o), dev(t)
    ws = ops.silog_ws(5, 'cuda')
    loss = torch.empty(1, device='cuda')
    ops.silog_loss_fwd(od, td, loss, ws)
    dout = Guarded(o.size)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().a3d_silog_loss_bwd(5, 4070, od.data_ptr(), td.data_ptr(), ws.data_ptr(), dout.t.data_ptr(), stream),
               'a3d_silog_loss_bwd')
    g = dout.host(5, 4070)
    assert rel_l2(g, T.silog_loss_bwd(o.astype(np.float64), t.astype(np.float64))) < 1e-5
    np.testing.assert_array_equal(g, run_loss(ops, o, t)[1])


def test_silog_workspace_serves_another_batch_size_in_between(ops):
    """One workspace of silog_ws(65) used for b = 65, then b = 3, then b = 65 again: the same three results as fresh
    workspaces (the arrival ticket sits where no batch size puts a sum, and returns to zero after every call)."""
    o65, t65 = loss_inputs(65, 4070)
    o3, t3 = loss_inputs(3, 7)
    fresh65, fresh3 = run_loss(ops, o65, t65), run_loss(ops, o3, t3)
    ws = ops.silog_ws(65, 'cuda')
    for (o, t), want in (((o65, t65), fresh65), ((o3, t3), fresh3), ((o65, t65), fresh65)):
        loss, g, _ = run_loss(ops, o, t, ws=ws)
        assert np.isfinite(loss[0])
        assert loss.view(np.uint32)[0] == want[0].view(np.uint32)[0]
        np.testing.assert_array_equal(g, want[1])


def test_silog_gradient_of_a_sample_that_holds_a_minus_infinite_log(ops):
    """o[0, 0] = -1e-8: fl(o + 1e-8f) = 0, log = -inf.  Position by position against the FLOAT32 oracle (in float64 the sum is
    not zero): the same elements are NaN, +inf, -inf and exactly 0; every other sample is finite and within 1e-5."""
    b, npix = 4, 4070
    o, t = loss_inputs(b, npix)
    o[0, 0] = -1e-8
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ref = T.silog_loss_bwd(o, t)
        assert not np.isfinite(T.silog_loss_fwd(o, t))
    assert np.isnan(ref[0, 0]) and np.isnan(ref).sum() == 1                   # what the oracle gives (computed on the CPU)
    assert np.isposinf(ref[0][o[0] > 0]).all() and (ref[0][o[0] < -1e-8] == 0).all() and np.isfinite(ref[1:]).all()
    loss, g, g16 = run_loss(ops, o, t, ld16=4072)
    assert not np.isfinite(loss[0])
    for name, cls in (('nan', np.isnan), ('+inf', np.isposinf), ('-inf', np.isneginf), ('zero', lambda a: a == 0)):
        np.testing.assert_array_equal(cls(g), cls(ref), err_msg=name)
    assert np.isfinite(g[1:]).all()
    assert rel_l2(g[1:], T.silog_loss_bwd(o.astype(np.float64), t.astype(np.float64))[1:]) < 1e-5
    assert_same_bf16(g16[:, :npix], R.bf16_round(g))


# ================================================================================================ pool kernels
def pool_values(rng, shape, pad_from=None):
    """bf16-valued float32: post-ReLU normals (about half exact zeros, ties everywhere) with a few -0.0; channels from
    `pad_from` on (pad channels of a wider pitch) hold a huge value no kernel may read."""
    x = R.bf16_values(np.maximum(rng.standard_normal(shape), 0).astype(np.float32))
    x[rng.random(shape) < 0.03] = -0.0
    if pad_from is not None:
        x[..., pad_from:] = 3e38
    return x


POOL16_CASES = [
    # n, h, w, c, ldx, ldy
    (2, 55, 74, 96, 104, 104), (2, 27, 37, 63, 64, 64), (3, 5, 4, 3, 3, 4), (2, 2, 2, 1, 1, 2), (2, 3, 3, 64, 64, 72),
    (1, 27, 37, 96, 96, 96), (2, 4, 6, 1, 1, 1),
    (24, 55, 74, 96, 96, 96),               # 2.30 M outputs: past 8192 blocks x 256
]
# The float32 entry points run the same templated bodies on a dense x: the small cases with ldx == c.  The bf16 cases keep
# the ids they always had.
POOL_FP32_CASES = [(3, 5, 4, 3, 3, 4), (2, 2, 2, 1, 1, 2), (2, 4, 6, 1, 1, 1), (2, 3, 3, 64, 64, 72)]
POOL_DTYPE_CASES = ([pytest.param('bf16', *case, id='-'.join(map(str, case))) for case in POOL16_CASES] +
                    [pytest.param('fp32', *case, id='fp32-' + '-'.join(map(str, case))) for case in POOL_FP32_CASES])


@pytest.mark.parametrize('dtype,n,h,w,c,ldx,ldy', POOL_DTYPE_CASES)
def test_maxpool2x2_fwd_bf16_against_the_oracle(ops, dtype, n, h, w, c, ldx, ldy):
    """a3d_maxpool2x2_fwd_bf16 vs T.maxpool2x2_fwd (exact on bf16 values), the concatenated float32 channel vs R.bf16_round.
    fp32: a3d_maxpool2x2_fwd, the same body, on the same values; its concatenated channel is `extra` itself."""
    rng = np.random.default_rng(h * 1000 + w * 10 + c)
    ho, wo = h // 2, w // 2
    x = pool_values(rng, (n, h, w, ldx), pad_from=c)
    ref = T.maxpool2x2_fwd(x[..., :c])
    extras = [None]
    if ldy > c:
        e = (rng.standard_normal((n, ho, wo)) * 3).astype(np.float32)        # not bf16-representable
        e.reshape(-1)[:2] = np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)[:e.size]     # ties
        extras.append(e)
    if dtype == 'fp32':
        xd = dev(x)
        for extra in extras:
            y = Guarded(n * ho * wo * ldy)
            ops.maxpool2x2_fwd(xd, y.view(n, ho, wo, ldy), None if extra is None else dev(extra))
            got = y.host(n, ho, wo, ldy)
            np.testing.assert_array_equal(got[..., :c], ref)
            used = c
            if extra is not None:
                np.testing.assert_array_equal(got[..., c].view(np.uint32), extra.view(np.uint32))       # a copy: no rounding
                used = c + 1
            assert (got[..., used:] == SENT).all()
        return
    xd = dev16(R.bf16_round(x))
    for extra in extras:
        y = Guarded(n * ho * wo * ldy, BF16)
        ops.maxpool2x2_fwd_bf16(xd, y.view(n, ho, wo, ldy), None if extra is None else dev(extra), c=c)
        got = y.host(n, ho, wo, ldy)
        np.testing.assert_array_equal(R.bf16_to_f32(got[..., :c]), ref)
        used = c
        if extra is not None:
            np.testing.assert_array_equal(got[..., c], R.bf16_round(extra))
            used = c + 1
        assert (got[..., used:] == SENT16).all()


@pytest.mark.parametrize('dtype,n,h,w,c,ldx,ldy', POOL_DTYPE_CASES)
def test_maxpool2x2_bwd_bf16_against_the_oracle(ops, dtype, n, h, w, c, ldx, ldy):
    """a3d_maxpool2x2_bwd_bf16 vs T.maxpool2x2_bwd / T.relu_grad: first maximum in scan order on exact ties (-0.0 and +0.0
    are a tie), dx at x's pitch with its pad channels untouched, the row / column VALID flooring cuts zero.
    fp32: a3d_maxpool2x2_bwd, the same body, on the same values (x and dx dense, dy at its pitch)."""
    rng = np.random.default_rng(h * 1000 + w * 10 + c + 1)
    ho, wo = h // 2, w // 2
    lddy = ldy
    x = pool_values(rng, (n, h, w, ldx), pad_from=c)
    dy = R.bf16_values(rng.standard_normal((n, ho, wo, lddy)).astype(np.float32))
    dy[..., c:] = 3e38
    plain = T.maxpool2x2_bwd(x[..., :c], dy[..., :c])
    if dtype == 'fp32':
        xd, dyd = dev(x), dev(dy)
        for relu_mask, ref in ((False, plain), (True, T.relu_grad(plain, x))):
            dx = Guarded(n * h * w * c)
            ops.maxpool2x2_bwd(xd, dyd, dx.view(n, h, w, c), relu_mask=relu_mask)
            got = dx.host(n, h, w, c)
            np.testing.assert_array_equal(got, ref)              # 3e38 in dy's pad channels would show if one were read
            if h % 2:
                assert (got[:, -1].view(np.uint32) & 0x7FFFFFFF == 0).all()
            if w % 2:
                assert (got[:, :, -1].view(np.uint32) & 0x7FFFFFFF == 0).all()
        return
    xd, dyd = dev16(R.bf16_round(x)), dev16(R.bf16_round(dy))
    for relu_mask, ref in ((False, plain), (True, T.relu_grad(plain, x[..., :c]))):
        dx = Guarded(n * h * w * ldx, BF16)
        ops.maxpool2x2_bwd_bf16(xd, dyd, dx.view(n, h, w, ldx), relu_mask=relu_mask, c=c)
        got = dx.host(n, h, w, ldx)
        np.testing.assert_array_equal(R.bf16_to_f32(got[..., :c]), ref)
        assert (got[..., c:] == SENT16).all()
        if h % 2:
            assert (got[:, -1, :, :c] & 0x7FFF == 0).all()
        if w % 2:
            assert (got[:, :, -1, :c] & 0x7FFF == 0).all()


def idx_inputs(rng, n, h, w, c, ldy, lddy):
    ho, wo = h // 2, w // 2
    arg = rng.integers(0, 4, (n, ho, wo, c)).astype(np.uint8)               # random: routed by the byte, not by values
    y = pool_values(rng, (n, ho, wo, ldy))
    y[rng.random(y.shape) < 0.05] = -1.0
    dy = R.bf16_values(rng.standard_normal((n, ho, wo, lddy)).astype(np.float32))
    return arg, y, dy


IDX_CASES = [
    # n, h, w, c, ldy, lddy
    (2, 55, 74, 96, 104, 112), (2, 27, 37, 64, 72, 80), (3, 5, 4, 8, 16, 24), (2, 2, 2, 8, 8, 16), (2, 3, 3, 16, 24, 32),
    (1, 27, 37, 63, 64, 63), (2, 5, 5, 3, 4, 3), (2, 4, 6, 1, 1, 2), (1, 7, 9, 12, 12, 16),
    (24, 55, 74, 96, 96, 104),              # 2.39 M cells x channels: past the block cap in the one-channel-per-thread forms
]


# the bf16 -> bf16 form takes whole 16-byte pieces only (its refusal of anything else is tested below)
IDX_FORM_CASES = [(form,) + case for case in IDX_CASES for form in ('f32', 'bf16_f32', 'bf16_bf16')
                  if form != 'bf16_bf16' or not (case[3] % 8 or case[4] % 8 or case[5] % 8)]


@pytest.mark.parametrize('form,n,h,w,c,ldy,lddy', IDX_FORM_CASES)
def test_maxpool2x2_bwd_idx_routes_by_the_argmax_byte(ops, form, n, h, w, c, ldy, lddy):
    """a3d_maxpool2x2_bwd_idx (scalar and vec4 by alignment), a3d_maxpool2x2_bwd_idx_bf16 (bf16 -> fp32) and
    a3d_maxpool2x2_bwd_idx_bf16s (bf16 -> bf16, eight channels per thread) vs R.maxpool2x2_bwd_from_argmax."""
    rng = np.random.default_rng(h * 1000 + w * 10 + c + 2)
    ho, wo = h // 2, w // 2
    arg, y, dy = idx_inputs(rng, n, h, w, c, ldy, lddy)
    argd = dev(arg)
    in16 = form != 'f32'
    yd, dyd = (dev16(R.bf16_round(y)), dev16(R.bf16_round(dy))) if in16 else (dev(y), dev(dy))
    for relu_mask in (True, False):
        ref = R.maxpool2x2_bwd_from_argmax(arg, y[..., :c], dy[..., :c], h, w, relu_mask)
        dx = Guarded(n * h * w * c, BF16 if form == 'bf16_bf16' else torch.float32)
        ops.maxpool2x2_bwd_idx(argd, yd, dyd, dx.view(n, h, w, c), relu_mask=relu_mask)
        got = dx.host(n, h, w, c)
        np.testing.assert_array_equal(R.bf16_to_f32(got) if form == 'bf16_bf16' else got, ref)
        if form == 'f32':
            # the same tensors one float further on: no longer 16-byte aligned, the scalar kernel runs; same bits
            dx1 = Guarded(n * h * w * c, offset=1)
            y1 = Guarded(y.size, offset=1)
            y1.t.copy_(yd.view(-1))
            ops.maxpool2x2_bwd_idx(argd, y1.view(*y.shape), dyd, dx1.view(n, h, w, c), relu_mask=relu_mask)
            np.testing.assert_array_equal(dx1.host(n, h, w, c).view(np.uint32), got.view(np.uint32))


def test_maxpool2x2_bwd_idx_bf16s_refuses_what_it_cannot_vectorise(ops, A3dError):
    rng = np.random.default_rng(4)
    n, h, w = 1, 4, 4
    for c, ldy, lddy, off in ((12, 16, 16, 0), (8, 12, 16, 0), (8, 16, 16, 4)):
        arg, y, dy = idx_inputs(rng, n, h, w, c, ldy, lddy)
        dyg = Guarded(dy.size, BF16, offset=8 + off)                         # off = 4 elements: 8 bytes off 16-byte alignment
        dyg.t.copy_(dev16(R.bf16_round(dy)).view(-1))
        dx = Guarded(n * h * w * c, BF16)
        with pytest.raises(A3dError):
            ops.maxpool2x2_bwd_idx(dev(arg), dev16(R.bf16_round(y)), dyg.view(*dy.shape), dx.view(n, h, w, c))
        assert (dx.host() == SENT16).all()


def test_maxpool2x2_fp32_past_the_block_cap(ops):
    """a3d_maxpool2x2_fwd / a3d_maxpool2x2_bwd at the benchmark's conv2d_0 size: 3.07 M elements, more than 8192 x 256."""
    n, h, w, c = 32, 55, 74, 96
    rng = np.random.default_rng(55)
    x = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32)
    ho, wo = h // 2, w // 2
    xd = dev(x)
    y = Guarded(n * ho * wo * c)
    ops.maxpool2x2_fwd(xd, y.view(n, ho, wo, c))
    np.testing.assert_array_equal(y.host(n, ho, wo, c), T.maxpool2x2_fwd(x))
    dy = rng.standard_normal((n, ho, wo, c)).astype(np.float32)
    plain = T.maxpool2x2_bwd(x, dy)
    for relu_mask, ref in ((False, plain), (True, T.relu_grad(plain, x))):
        dx = Guarded(x.size)
        ops.maxpool2x2_bwd(xd, dev(dy), dx.view(n, h, w, c), relu_mask=relu_mask)
        np.testing.assert_array_equal(dx.host(n, h, w, c), ref)


# ================================================================================================ casts and copies
CAST_BIG = 4096 * 256 * 4 + 5             # past the 4096 blocks x 256 threads x 4 elements of one sweep, tail of 1
CAST_COUNTS = list(range(1, 10)) + [4 * 1000 + 3, CAST_BIG]
FLUSH_DENORMALS = False                    # the casts keep float32 denormals (measured; include/a3d.h, a3d_cast_bf16)


def cast_source(count, seed=0):
    """float32 with every special of tests/test_pointwise_ref.py (signed zeros and infinities, overflow, ties, denormals,
    NaNs) at both ends — in the vector body and in the scalar tail — and normals between; the last element is always the
    tie 0x3F818000 (-> 0x3F82), so a tail that is not converted shows."""
    s = np.concatenate([SPECIAL_BITS, NAN_BITS]).view(np.float32)
    last = int(np.flatnonzero(SPECIAL_BITS == 0x3F818000)[0])
    if count < 2 * s.size:
        return s[(np.arange(count) - (count - 1) + last) % s.size].copy()
    x = (np.random.default_rng(count + seed).standard_normal(count) * 3).astype(np.float32)
    x[:s.size] = s
    x[-s.size:] = np.roll(s, s.size - 1 - last)
    return x


def round_ref(x):
    return R.bf16_round(x, flush_denormals=FLUSH_DENORMALS)


@pytest.mark.parametrize('count', CAST_COUNTS)
def test_cast_bf16_both_ways(ops, count):
    """a3d_cast_bf16: float32 -> bf16 is round to nearest even on the bits (ties, overflow to infinity, -0.0, denormals kept,
    NaN stays NaN); bf16 -> float32 is exact for every bit pattern."""
    x = cast_source(count)
    d16 = Guarded(count, BF16)
    ops.cast_bf16(dev(x), d16.t)
    got = d16.host()
    assert_same_bf16(got, round_ref(x))
    bits = np.random.default_rng(count).integers(0, 1 << 16, count).astype(np.uint16)
    bits[:min(count, got.size)] = np.where(np.arange(count) % 2 == 0, got, bits)[:count]
    d32 = Guarded(count)
    ops.cast_bf16(dev16(bits), d32.t)
    assert_same_f32(d32.host(), R.bf16_to_f32(bits))


CAST_ROWS_CASES = [(1, 1, 1, 1), (5, 7, 9, 8), (3, 8, 8, 16), (33, 4070, 4070, 4072), (600, 4070, 4072, 4072)]   # last: 2.44 M > 8192 x 256


@pytest.mark.parametrize('s16,d16', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('rows,cols,ld_src,ld_dst', CAST_ROWS_CASES)
def test_cast_rows_all_type_pairs(ops, rows, cols, ld_src, ld_dst, s16, d16):
    """a3d_cast_rows: dst[r, :cols] = src[r, :cols] in dst's type, dst[r, cols:] = +0, nothing past the last row; the source's
    pad columns (NaN here) are not read."""
    x = cast_source(rows * ld_src, seed=1).reshape(rows, ld_src)
    if s16:
        x = R.bf16_to_f32(np.where(np.isnan(x), np.uint16(0x7FC1), R.bf16_round(x)).astype(np.uint16))
    x[:, cols:] = np.nan
    src = dev16(R.bf16_round(x)) if s16 else dev(x)
    dst = Guarded(rows * ld_dst, BF16 if d16 else torch.float32)
    ops.cast_rows(src, dst.view(rows, ld_dst), cols=cols)
    got = dst.host(rows, ld_dst)
    if d16:
        assert_same_bf16(got[:, :cols], round_ref(x[:, :cols]))
    else:
        assert_same_f32(got[:, :cols], x[:, :cols])
    assert (got[:, cols:].view(np.uint16 if d16 else np.uint32) == 0).all()


# one oversized case (past 4096 blocks x 256 pixels), at the 3 channels the product pads
@pytest.mark.parametrize('pixels,c_src', [(p, c) for p in (1, 5, 1000) for c in (1, 2, 3, 4)] + [(4096 * 256 + 3, 3)])
def test_pad_channels_bf16(ops, c_src, pixels):
    """a3d_pad_channels_bf16: float32 [pixels, c_src] -> bf16 [pixels, 4], rounded to nearest even, missing channels +0."""
    x = cast_source(pixels * c_src, seed=2).reshape(pixels, c_src)
    dst = Guarded(pixels * 4, BF16)
    ops.pad_channels_bf16(dev(x), dst.view(pixels, 4))
    got = dst.host(pixels, 4)
    assert_same_bf16(got[:, :c_src], round_ref(x))
    assert (got[:, c_src:] == 0).all()


COPY_CASES = [
    # npix, ld_src, c_src, ld_dst, c_dst
    (1, 1, 0, 1, 0), (1000, 1, 0, 1, 0), (1000, 2, 1, 64, 63), (1000, 64, 31, 2, 0), (1000, 1, 0, 64, 32), (1000, 64, 63, 64, 0),
    (37, 2, 0, 2, 1), (2048 * 256 + 5, 1, 0, 2, 1),                          # last: past 2048 blocks x 256 pixels
]


@pytest.mark.parametrize('to16', [False, True])
@pytest.mark.parametrize('npix,ld_src,c_src,ld_dst,c_dst', COPY_CASES)
def test_copy_channel(ops, npix, ld_src, c_src, ld_dst, c_dst, to16):
    """a3d_copy_channel / a3d_copy_channel_bf16: one channel of every pixel, every other element of dst untouched."""
    x = cast_source(npix * ld_src, seed=3).reshape(npix, ld_src)
    dst = Guarded(npix * ld_dst, BF16 if to16 else torch.float32)
    ops.copy_channel(dev(x), c_src, dst.view(npix, ld_dst), c_dst)
    got = dst.host(npix, ld_dst)
    if to16:
        assert_same_bf16(got[:, c_dst], round_ref(x[:, c_src]))
    else:
        assert_same_f32(got[:, c_dst], x[:, c_src])
    others = np.delete(got, c_dst, axis=1)
    assert (others == (SENT16 if to16 else np.float32(SENT))).all()


# ================================================================================================ ApplyAdam
ADAM_BIG = 4096 * 256 * 4 + 3             # the grid-stride loop (dense_0 has 50 M weights) and a scalar tail of 3


class AdamPair:
    """The same optimizer state on the device (guarded windows) and in the oracle's AdamTF1."""

    def __init__(self, var, v0, beta2, lr=0.1):
        self.beta2, self.lr = beta2, lr
        count = var.size
        self.opt = T.AdamTF1(lr, 0.9, beta2)
        self.opt.m['w'] = np.zeros(count, np.float32)
        self.opt.v['w'] = v0.copy()
        self.ref = {'w': var.copy()}
        self.bufs = [Guarded(count) for _ in range(4)]                       # var, m, v, g
        for buf, a in zip(self.bufs, (var, np.zeros(count, np.float32), v0)):
            buf.t.copy_(dev(a))
        self.b1p, self.b2p = np.float32(0.9), np.float32(beta2)

    def step(self, ops, g, scale=1.0, poisoned=None):
        before = (self.ref['w'].copy(), self.opt.v['w'].copy())
        with np.errstate(invalid='ignore', over='ignore'):
            self.opt.apply(self.ref, {'w': g * np.float32(scale) if scale != 1.0 else g})
        self.bufs[3].t.copy_(dev(g))
        var, m, v, gd = (b.t for b in self.bufs)
        ops.adam_apply_tf1(var, m, v, gd, self.lr, 0.9, self.beta2, 1e-8, float(self.b1p), float(self.b2p), scale,
                           poisoned=poisoned)
        self.b1p, self.b2p = self.b1p * np.float32(0.9), self.b2p * np.float32(self.beta2)
        return R.adam_poisoned(before[0], before[1], self.ref['w'], self.opt.v['w'])

    def check(self):
        np.testing.assert_array_equal(self.bufs[1].host(), self.opt.m['w'], err_msg='m')
        np.testing.assert_array_equal(self.bufs[2].host(), self.opt.v['w'], err_msg='v')
        np.testing.assert_array_equal(self.bufs[0].host(), self.ref['w'], err_msg='var')
        self.bufs[3].host()


ADAM_CASES = [(c, 1.0) for c in (1, 2, 3, 5, 4003, ADAM_BIG)] + [(5, 0.125), (5, 1 / 3), (4003, 0.125), (4003, 1 / 3)]


@pytest.mark.parametrize('beta2', [0.999, 1.0])
@pytest.mark.parametrize('count,scale', ADAM_CASES)
def test_adam_apply_tf1_bit_for_bit(ops, count, scale, beta2):
    """a3d_adam_apply_tf1 (adam_kernel for beta2 < 1, adam_frozen_kernel for beta2 = 1) vs T.AdamTF1 over three steps: counts
    below one vector, the scalar tail, the grid-stride loop, grad_scale applied to g first."""
    rng = np.random.default_rng(count)
    pair = AdamPair(rng.standard_normal(count).astype(np.float32), (rng.random(count) * 0.01).astype(np.float32), beta2)
    for _ in range(3):
        pair.step(ops, rng.standard_normal(count).astype(np.float32), scale)
        pair.check()


@pytest.mark.parametrize('beta2', [0.999, 1.0])
def test_adam_on_a_slice_leaves_the_rest_alone(ops, beta2):
    """A data-parallel rank's call: var[a:b] of the group's flat buffers, a a multiple of 64."""
    rng = np.random.default_rng(64)
    total, a, b = 1024, 128, 128 + 4 * 64 + 3
    state = [rng.standard_normal(total).astype(np.float32), np.zeros(total, np.float32),
             (rng.random(total) * 0.01).astype(np.float32), rng.standard_normal(total).astype(np.float32)]
    bufs = [dev(s) for s in state]
    opt = T.AdamTF1(0.1, 0.9, beta2)
    opt.m['w'], opt.v['w'] = state[1][a:b].copy(), state[2][a:b].copy()
    ref = {'w': state[0][a:b].copy()}
    opt.apply(ref, {'w': state[3][a:b] * np.float32(0.5)})
    ops.adam_apply_tf1(bufs[0][a:b], bufs[1][a:b], bufs[2][a:b], bufs[3][a:b], 0.1, 0.9, beta2, 1e-8, 0.9, beta2, 0.5)
    for buf, before, inner in zip(bufs, state, (ref['w'], opt.m['w'], opt.v['w'], state[3][a:b])):
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(got[:a], before[:a])
        np.testing.assert_array_equal(got[b:], before[b:])
        np.testing.assert_array_equal(got[a:b], inner)


@pytest.mark.parametrize('beta2', [0.999, 1.0])
def test_adam_poisoned_flag_means_the_update_turned_something_non_finite(ops, beta2):
    """a3d_adam_apply_tf1_flag: bit 0 is R.adam_poisoned — the update CHANGED an element of var or v into a non-finite value —
    on both kernels; the state itself stays bit-identical to the oracle with and without the flag pointer."""
    count = 4 * 16 + 2
    rng = np.random.default_rng(29)

    def fresh(var_nan_at=None):
        var = rng.standard_normal(count).astype(np.float32)
        if var_nan_at is not None:
            var[var_nan_at] = np.nan
        return (AdamPair(var, (rng.random(count) * 0.01).astype(np.float32), beta2),
                AdamPair(var, (rng.random(count) * 0.01).astype(np.float32) * 0 + 0.005, beta2))

    def run(pair, g, expect=None):
        flag = torch.zeros(4, dtype=torch.int32, device='cuda')
        want = pair.step(ops, g, poisoned=flag[1:2])
        pair.check()
        got = flag.cpu().numpy()
        assert got[0] == 0 and got[2] == 0 and got[3] == 0
        assert got[1] == want, f'flag {got[1]}, the statement gives {want}'
        if expect is not None:
            assert want == expect
        return want

    finite = lambda: rng.standard_normal(count).astype(np.float32)
    pair, _ = fresh()
    run(pair, finite(), expect=0)                                            # all finite
    for bad in (np.inf, np.nan, 3e19):                                       # 3e19: finite, its square is not
        pair, _ = fresh()
        g = finite(); g[5] = bad
        run(pair, g, expect=1)
        g = finite(); g[5] = bad
        run(pair, g)                                                         # the same element a second step
        run(pair, finite())                                                  # and a finite step after it
    pair, _ = fresh()
    g = finite(); g[9] = np.inf
    assert run(pair, g) == 1
    # beta2 = 1: var and v are NaN after the first step and stay so; beta2 < 1: v = inf first and turns NaN in the second
    assert run(pair, g) == (0 if beta2 == 1.0 else 1)
    assert run(pair, g) == 0                                                 # NaN stays NaN: nothing new to tell the other ranks
    pair, _ = fresh(var_nan_at=7)                                            # var NaN on entry, finite gradient
    run(pair, finite(), expect=0)
    pair, _ = fresh()
    g = finite(); g[count - 1] = -np.inf                                     # only in the scalar tail
    run(pair, g, expect=1)
    # poisoned = None: the same update
    a, b = fresh()
    b = AdamPair(a.ref['w'].copy(), a.opt.v['w'].copy(), beta2)
    g = finite(); g[3] = np.inf; g[count - 2] = np.nan
    run(a, g, expect=1)
    b.step(ops, g)
    b.check()
    for x, y in zip(a.bufs[:3], b.bufs[:3]):
        np.testing.assert_array_equal(x.host(), y.host())


# ================================================================================================ resize and patches
def test_resize_rows_past_the_block_cap(ops):
    """a3d_resize_bilinear_tf1 with 80 x 228 = 18240 output rows (one block per row, 16384 blocks at most), and
    a3d_resize_bilinear_tf1_pair with its two outputs on different sides of that cap."""
    rng = np.random.default_rng(80)
    n = 80
    img = (rng.integers(0, 256, (n, 12, 16, 3)) / 255).astype(np.float32)
    dep = (rng.integers(0, 256, (n, 12, 16, 1)) / 255).astype(np.float32)
    y = Guarded(n * 228 * 20 * 3)
    ops.resize_bilinear_tf1(dev(img), y.view(n, 228, 20, 3))
    np.testing.assert_array_equal(y.host(n, 228, 20, 3), T.resize_bilinear_tf1(img, 228, 20))
    for (oh0, ow0), (oh1, ow1) in (((55, 74), (228, 20)), ((228, 20), (55, 74))):
        y0, y1 = Guarded(n * oh0 * ow0 * 3), Guarded(n * oh1 * ow1)
        ops.resize_bilinear_tf1_pair(dev(img), y0.view(n, oh0, ow0, 3), dev(dep), y1.view(n, oh1, ow1, 1))
        np.testing.assert_array_equal(y0.host(n, oh0, ow0, 3), T.resize_bilinear_tf1(img, oh0, ow0))
        np.testing.assert_array_equal(y1.host(n, oh1, ow1, 1), T.resize_bilinear_tf1(dep, oh1, ow1))


def test_resize_from_uint8_pixels_past_the_block_cap(ops):
    """a3d_resize_bilinear_tf1_ex: uint8 pixel values k read as fl(fl(fl(k / 255) - 0.5) + 0.5), one and two tensors."""
    rng = np.random.default_rng(81)
    n = 80
    k3 = rng.integers(0, 256, (n, 12, 16, 3)).astype(np.uint8)
    k1 = rng.integers(0, 256, (n, 12, 16, 1)).astype(np.uint8)
    as_float = lambda k: (k.astype(np.float32) / np.float32(255) - np.float32(0.5)) + np.float32(0.5)
    y = Guarded(n * 228 * 20 * 3)
    ops.resize_bilinear_tf1(dev(k3), y.view(n, 228, 20, 3))
    np.testing.assert_array_equal(y.host(n, 228, 20, 3), T.resize_bilinear_tf1(as_float(k3), 228, 20))
    y0, y1 = Guarded(n * 55 * 74 * 3), Guarded(n * 228 * 20)
    ops.resize_bilinear_tf1_pair(dev(k3), y0.view(n, 55, 74, 3), dev(k1), y1.view(n, 228, 20, 1))
    np.testing.assert_array_equal(y0.host(n, 55, 74, 3), T.resize_bilinear_tf1(as_float(k3), 55, 74))
    np.testing.assert_array_equal(y1.host(n, 228, 20, 1), T.resize_bilinear_tf1(as_float(k1), 228, 20))


@pytest.mark.parametrize('n,h,w,c,k,stride', [(2, 241, 323, 3, 100, 40),    # total padding 99 and 97: odd both ways
                                              (2, 50, 70, 3, 16, 24),         # k < stride: no padding at all (the clamp)
                                              (3, 33, 47, 1, 5, 3)])
def test_extract_patches_with_uneven_padding(ops, n, h, w, c, k, stride):
    """a3d_extract_patches vs T.extract_patches: SAME padding puts pad // 2 above / left and the rest below / right."""
    rng = np.random.default_rng(h + k)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    ref = T.extract_patches(x, k, stride, 'SAME')
    y = Guarded(ref.size)
    ops.extract_patches(dev(x), k, stride, y.view(ref.shape[0] * ref.shape[1], k, k, c))
    np.testing.assert_array_equal(y.host(*ref.shape), ref)


# ================================================================================================ collective stand-in
def test_comm_standin_keeps_to_its_destination_when_blocks_outnumber_the_pieces(ops):
    """a3d_comm_standin with more workgroups than 16-byte pieces to write: a block whose write share is empty (its first
    piece lies past the end) must write nothing.  The reduce-scatter of an 8 KB bucket at world size 8 (1 KB written) over
    24 workgroups, and 16 bytes written for 1 MB read."""
    from ann3depth_amd import _lib
    for read_bytes, write_bytes in ((8192, 1024), (1 << 20, 16)):
        src = torch.ones(read_bytes // 4, device='cuda')
        dst = Guarded(write_bytes // 4, guard=4096, offset=4096)
        rc = _lib.load().a3d_comm_standin(ctypes.c_void_p(src.data_ptr()), read_bytes, ctypes.c_void_p(dst.t.data_ptr()),
                                          write_bytes, 24, 400.0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0                          # A3D_OK
        torch.cuda.synchronize()
        dst.host()                              # asserts the guard elements before and after
