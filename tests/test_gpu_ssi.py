"""a3di_ssi_loss_fwd / a3di_ssi_loss_bwd_ex on the GPU against tests/ssi_ref.py in float64, at 8 x the error the float32
restatement shows on the same inputs, and bit for bit where include/a3d_ssi.h promises exact values: integer-valued inputs,
an exact fit, constant outputs, invariance under a scale and shift of the output, zeros at holes, poisoned samples, halves of
a batch, a shared workspace; and the fit against a3da_depth_align's A3DA_AFFINE on the same grids."""
import numpy as np
import pytest
import torch

import ssi_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
# fewer pixels than parts x 4; around a thread count (255, 256, 257) and around a part's 8 x 256 pixels (2047, 2049); the
# model's grid, rows that start off the 16-byte grid; a chunk of 37 rounds
SHAPES = [(2, 15), (3, 255), (3, 256), (3, 257), (2, 2047), (2, 2049), (5, 4070), (1, 300001)]


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


_CASES = {}


def case(b, npix, masked):
    """Inputs of one shape, computed once and shared."""
    key = (b, npix, masked)
    if key not in _CASES:
        _CASES[key] = R.case(b, npix, seed=b + npix, masked=masked)
    return _CASES[key]


def run(ops, o, t, masked, ws=None, ld16=None):
    b, npix = o.shape
    ws = ops.ssi_ws(b, 'cuda') if ws is None else ws
    od, td = dev(o), dev(t)
    loss = torch.full((6,), 7.0, device='cuda')
    dout = torch.full((b, npix), 7.0, device='cuda')
    d16 = None if ld16 is None else torch.full((b, ld16), 7.0, device='cuda', dtype=torch.bfloat16)
    ops.ssi_loss_fwd(od, td, masked, loss[:4], ws)
    ops.ssi_loss_bwd(od, td, masked, ws, dout, d16)
    torch.cuda.synchronize()
    assert float(loss[4]) == 7.0 and float(loss[5]) == 7.0, 'the forward writes four floats'
    assert float(ws[0]) == 0 and float(ws[1]) == 0, 'the ticket wrapped back'
    return loss[:4].cpu().numpy(), dout.cpu().numpy(), d16, ws


def per_sample(ws, b):
    """(s, t, n, flag), each [b], from the workspace of a call of batch b."""
    w = ws.cpu().numpy()[2:2 + 4 * b].reshape(b, 4)
    return w[:, 0], w[:, 1], w[:, 2], w[:, 3]


@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('b,npix', SHAPES)
def test_loss_and_gradient_against_the_reference(ops, b, npix, masked):
    o, t = case(b, npix, masked)
    ref, b_loss, b_s, b_t, b_grad = R.bound(o, t, masked)
    l64, g64, s64, t64, flag64, n64 = ref
    l32, g32, s32, t32, _, _ = R.loss32(o, t, masked)
    cnt = R.counting(t, masked)
    loss, g, d16, ws = run(ops, o, t, masked, ld16=npix + 5)
    s, sh, n, flag = per_sample(ws, b)
    e_loss, e_s, e_t, e_grad = R.errors(loss, g, ref)
    same = ((bits(loss) == bits(l32)).all() and (bits(g) == bits(g32)).all() and (bits(s) == bits(s32)).all()
            and (bits(sh) == bits(t32)).all())
    print(f'ssi ({b},{npix}) masked={masked}: loss {e_loss:.2e} (bound {b_loss:.2e}), scale {e_s:.2e} ({b_s:.2e}), shift '
          f'{e_t:.2e} ({b_t:.2e}), gradient {e_grad:.2e} ({b_grad:.2e}); loss {l64[0]:.6g} scale {l64[2]:.6g} shift {l64[3]:.6g}; '
          f'the bits of the float32 restatement: {"yes" if same else "no"}')
    assert np.isfinite(loss).all() and l64[0] > 0
    assert e_loss <= b_loss and e_s <= b_s and e_t <= b_t
    assert e_grad <= b_grad
    # exact: the fraction of counting pixels, the counts, the flags, zeros at holes
    assert loss[1] == (F(cnt.sum() / (b * npix)) if masked else F(1))
    np.testing.assert_array_equal(n, cnt.sum(axis=1).astype(F))
    np.testing.assert_array_equal(flag, flag64.astype(F))
    assert (bits(g[~cnt]) == 0).all()
    fitted = flag64 == R.FITTED
    assert fitted.any() and (g[fitted][cnt[fitted]] != 0).mean() > 0.99
    if masked and b >= 3:                                                   # the sample without a finite target: degenerate
        m = b // 2
        assert (bits(g[m]) == 0).all() and bits(s[m]) == 0 and bits(sh[m]) == 0 and flag[m] == 1 and n[m] == 0
    # the bf16 copy: the (__bf16) cast of dout, the pitch columns untouched
    h16 = d16.float().cpu().numpy()
    np.testing.assert_array_equal(h16[:, :npix], torch.from_numpy(g).to(torch.bfloat16).float().numpy())
    assert (h16[:, npix:] == 7.0).all()


@pytest.mark.parametrize('b', [1, 2, 4])
def test_integer_inputs_bit_for_bit(ops, b):
    """Whole numbers, every other pixel a hole (with a large error on it), s = 2, t = 3, r in {-3 .. 3}, r_n = 2, h = 1: every
    operation is exact, so the float64 reference is the answer element by element."""
    o, t = R.integer_case(b, 4072, seed=b)
    R.exact_conditions(o, t)
    l64, g64 = R.loss64(o, t, 1)[:2]
    loss, g, _, ws = run(ops, o, t, 1)
    np.testing.assert_array_equal(bits(loss), bits(l64))
    np.testing.assert_array_equal(bits(g), bits(g64))
    s, sh, n, flag = per_sample(ws, b)
    assert (s == 2).all() and (sh == 3).all() and (n == 2036).all() and (flag == 0).all()
    assert loss[1] == 0.5 and loss[2] == 2 and loss[3] == 3 and loss[0] > 0
    cnt = np.isfinite(t)
    assert set(np.unique(np.abs(g[cnt]))) == {0, 4 / b, 8 / b, 12 / b}


def test_invariance_under_a_scale_and_shift_of_the_output(ops):
    """The feature's point, exactly: 4 o + 8 is exact in float32 on the integer case.  The loss is the same bits, s becomes
    s / 4, t absorbs the shift, and the gradient is the gradient / 4."""
    o, t = R.integer_case(2, 4072, seed=7)
    o2 = (F(4) * o + F(8)).astype(F)
    loss, g, _, ws = run(ops, o, t, 1)
    loss2, g2, _, ws2 = run(ops, o2, t, 1)
    np.testing.assert_array_equal(bits(loss[:2]), bits(loss2[:2]))
    s, sh, _, _ = per_sample(ws, 2)
    s2, sh2, _, flag2 = per_sample(ws2, 2)
    assert (s == 2).all() and (s2 == 0.5).all() and (sh == 3).all() and (sh2 == -1).all() and (flag2 == 0).all()
    np.testing.assert_array_equal(bits(g2), bits(g / F(4)))
    assert loss[0] > 0 and (g != 0).any()
    # the residuals themselves: the aligned outputs are the same bits
    q, q2 = (s[:, None] * o).astype(F) + sh[:, None], (s2[:, None] * o2).astype(F) + sh2[:, None]
    np.testing.assert_array_equal(bits(q), bits(q2))


def test_one_pixel_and_an_exact_fit_through_two(ops):
    for masked in (0, 1):
        loss, g, _, ws = run(ops, np.array([[0.75]], F), np.array([[0.25]], F), masked)       # (1, 1): degenerate
        s, sh, n, flag = per_sample(ws, 1)
        assert bits(loss[0]) == 0 and (bits(g) == 0).all() and flag[0] == 1 and bits(s)[0] == 0 and sh[0] == 0.25 and n[0] == 1
        assert loss[1] == 1 and bits(loss[2]) == 0 and loss[3] == 0.25
        loss, g, _, ws = run(ops, np.array([[1, 3]], F), np.array([[5, 9]], F), masked)      # (1, 2): s = 2, t = 3
        s, sh, n, flag = per_sample(ws, 1)
        assert s[0] == 2 and sh[0] == 3 and n[0] == 2 and flag[0] == 0
        assert loss[0] == 0 and (g == 0).all() and loss[2] == 2 and loss[3] == 3


@pytest.mark.parametrize('masked', [0, 1])
def test_a_constant_output_is_degenerate(ops, masked):
    o, t = case(3, 257, masked)
    o = o.copy()
    o[0] = F(0.7)
    o[2] = (F(0.7) + np.random.default_rng(5).integers(-1, 2, 257).astype(F) * np.spacing(F(0.7))).astype(F)   # +-1 ulp of noise
    l32, g32, s32, t32, flag32, _ = R.loss32(o, t, masked)
    loss, g, _, ws = run(ops, o, t, masked)
    s, sh, n, flag = per_sample(ws, 3)
    assert flag[0] == 1 and flag[2] == 1 and flag32[0] == 1 and flag32[2] == 1
    assert (bits(g[[0, 2]]) == 0).all() and (bits(s[[0, 2]]) == 0).all()
    np.testing.assert_array_equal(bits(sh), bits(t32))
    np.testing.assert_array_equal(bits(loss), bits(l32))                    # per = h sum (d - t)^2 to the restatement's bits
    np.testing.assert_array_equal(bits(g), bits(g32))
    cnt = R.counting(t, masked)
    d0 = t[0][cnt[0]].astype(np.float64)
    assert abs(float(sh[0]) - d0.mean()) <= 2.0 ** -23 * d0.mean() and loss[0] > 0


@pytest.mark.parametrize('what', ['nan_output', 'inf_output', 'nan_target', 'inf_target', 'nan_output_masked'])
def test_poison_stays_in_its_sample(ops, what):
    """NaN and inf as input VALUES."""
    masked = int(what == 'nan_output_masked')
    o, t = R.case(3, 257, seed=6, masked=masked)
    clean_loss, clean, _, clean_ws = run(ops, o, t, masked)
    o2, t2 = o.copy(), t.copy()
    row = 2 if masked else 1                                                # masked: sample 1 has no finite target
    k = int(np.flatnonzero(np.isfinite(t[row]))[100])
    if what.endswith('target'):
        t2[row, k] = np.nan if what == 'nan_target' else np.inf
    else:
        o2[row, k] = np.inf if what == 'inf_output' else np.nan
    loss, g, d16, ws = run(ops, o2, t2, masked, ld16=262)
    assert np.isnan(g[row]).all() and np.isnan(d16.float().cpu().numpy()[row, :257]).all()
    others = [r for r in range(3) if r != row]
    np.testing.assert_array_equal(bits(g[others]), bits(clean[others]))
    assert np.isnan(loss[[0, 2, 3]]).all() and loss[1] == clean_loss[1] and np.isfinite(clean_loss).all()
    s, sh, n, flag = per_sample(ws, 3)
    cs, csh, cn, cflag = per_sample(clean_ws, 3)
    assert np.isnan(s[row]) and np.isnan(sh[row]) and flag[row] == 2 and (flag[others] == cflag[others]).all()
    np.testing.assert_array_equal(bits(s[others]), bits(cs[others]))
    np.testing.assert_array_equal(bits(sh[others]), bits(csh[others]))
    if masked:                                                              # what sits on a hole poisons nobody
        o3 = o.copy()
        o3[~np.isfinite(t)] = np.inf
        loss3, g3, _, _ = run(ops, o3, t, 1)
        np.testing.assert_array_equal(bits(loss3), bits(clean_loss))
        np.testing.assert_array_equal(bits(g3), bits(clean))


@pytest.mark.parametrize('npix', [4070, 4071])
@pytest.mark.parametrize('masked', [0, 1])
def test_no_sample_sees_another(ops, masked, npix):
    """The rows of a b = 4 call are the rows of two b = 2 calls on its halves times 0.5, and of four calls of one sample times
    0.25, bit for bit (at 4071 pixels the rows also start at other offsets from the 16-byte grid than in the whole)."""
    o, t = R.case(4, npix, seed=8, masked=masked)
    if masked:
        t[2] = R.case(4, npix, seed=9, masked=1)[1][0]                      # an ordinary sample in place of the empty one
    loss, g, _, ws = run(ops, o, t, masked)
    whole = ws.cpu().numpy()[2:18].reshape(4, 4)
    for half in (0, 1):
        rows = slice(2 * half, 2 * half + 2)
        loss_h, g_h, _, ws_h = run(ops, o[rows], t[rows], masked)
        np.testing.assert_array_equal(bits(g[rows]), bits(g_h * F(0.5)))
        np.testing.assert_array_equal(bits(whole[rows]), bits(ws_h.cpu().numpy()[2:10].reshape(2, 4)))
    for i in range(4):
        loss_1, g_1, _, ws_1 = run(ops, o[i:i + 1], t[i:i + 1], masked)
        np.testing.assert_array_equal(bits(g[i:i + 1]), bits(g_1 * F(0.25)))
        np.testing.assert_array_equal(bits(whole[i]), bits(ws_1.cpu().numpy()[2:6]))
    assert (g != 0).any()


@pytest.mark.parametrize('masked', [0, 1])
def test_two_calls_on_one_workspace_and_two_runs_give_the_same_bits(ops, masked):
    o5, t5 = case(5, 4070, masked)
    o2, t2 = case(2, 2049, masked)
    ws = ops.ssi_ws(5, 'cuda')
    first = run(ops, o5, t5, masked, ws=ws)
    small = run(ops, o2, t2, masked, ws=ws)                                 # a smaller batch on the same workspace
    again = run(ops, o5, t5, masked, ws=ws)
    fresh = run(ops, o2, t2, masked)
    for x, y in ((first, again), (small, fresh)):
        np.testing.assert_array_equal(bits(x[0]), bits(y[0]))
        np.testing.assert_array_equal(bits(x[1]), bits(y[1]))
    assert float(ws[0]) == 0


@pytest.mark.parametrize('masked', [0, 1])
def test_the_fit_is_the_affine_alignment_of_evaluate(ops, masked):
    """a3da_depth_align in A3DA_AFFINE mode on the same grids, every finite target valid: per image the same float32 (s, t) or
    the adjacent ones — the two float64 sums differ only in their order."""
    import align_ref as A
    b, h, w = 5, 55, 74
    o, t = case(b, h * w, masked)
    if masked:
        t = t.copy()
        t[b // 2] = case(b, h * w, 0)[1][0]                                 # align reports an image without pixels as (1, 0)
    coef, count, status = ops.depth_align(dev(o).view(b, h, w), dev(t).view(b, h, w), 'affine', min_depth=-np.inf,
                                          max_depth=np.inf)
    loss, g, _, ws = run(ops, o, t, masked)
    s, sh, n, flag = per_sample(ws, b)
    coef = coef.cpu().numpy()
    assert (status.cpu().numpy() == 0).all() and (flag == 0).all()
    np.testing.assert_array_equal(count.cpu().numpy(), n.astype(np.int32))
    steps = A.ulps(np.stack([s, sh], axis=1), coef)
    print(f'ssi against A3DA_AFFINE, masked={masked}: float32 steps apart, scale {steps[:, 0].max()}, shift {steps[:, 1].max()}')
    assert (steps <= 1).all()


def test_bad_arguments(ops):
    x = torch.ones((2, 15), device='cuda')
    loss, ws = torch.zeros(4, device='cuda'), ops.ssi_ws(2, 'cuda')
    assert ws.numel() == 4 * 2 + 2 + 10 * 2 * 8                             # A3DI_WS_FLOATS(2)
    with pytest.raises(AssertionError, match='workspace too small'):
        ops.ssi_loss_fwd(x, x, 1, loss, ws[:-1])
    with pytest.raises(AssertionError, match='four floats'):
        ops.ssi_loss_fwd(x, x, 1, loss[:3], ws)
    with pytest.raises(AssertionError, match='values'):
        ops.ssi_loss_bwd(x, x[:, :14], 1, ws, x.clone())
    torch.cuda.synchronize()
    assert float(ws.abs().sum()) == 0 and float(loss.abs().sum()) == 0      # nothing was launched
