"""a3dh_berhu_loss_fwd / a3dh_berhu_loss_bwd_ex on the GPU against tests/berhu_ref.py in float64, at 8 x the error the float32
restatement shows on the same inputs, and bit for bit where include/a3d_berhu.h promises exact values: integer-valued inputs,
zeros at holes, poisoned samples, halves of a batch, a shared workspace."""
import numpy as np
import pytest
import torch

import berhu_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
# one pixel; two; fewer pixels than parts x 4; around a thread count (255, 256, 257) and around a part's 8 x 256 pixels
# (2047, 2049); the model's grid, rows that start off the 16-byte grid; a chunk of 37 rounds
SHAPES = [(1, 1), (1, 2), (2, 15), (3, 255), (3, 256), (3, 257), (2, 2047), (2, 2049), (5, 4070), (1, 300001)]


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
    """Inputs of one shape, computed once and shared by the fractions."""
    key = (b, npix, masked)
    if key not in _CASES:
        _CASES[key] = R.case(b, npix, seed=b + npix, masked=masked)
    return _CASES[key]


def run(ops, o, t, masked, fraction, ws=None, ld16=None):
    b, npix = o.shape
    ws = ops.berhu_ws(b, 'cuda') if ws is None else ws
    od, td = dev(o), dev(t)
    loss = torch.full((6,), 7.0, device='cuda')
    dout = torch.full((b, npix), 7.0, device='cuda')
    d16 = None if ld16 is None else torch.full((b, ld16), 7.0, device='cuda', dtype=torch.bfloat16)
    ops.berhu_loss_fwd(od, td, masked, fraction, loss[:4], ws)
    ops.berhu_loss_bwd(od, td, masked, fraction, ws, dout, d16)
    torch.cuda.synchronize()
    assert float(loss[4]) == 7.0 and float(loss[5]) == 7.0, 'the forward writes four floats'
    assert float(ws[0]) == 0, 'the ticket wrapped back'
    return loss[:4].cpu().numpy(), dout.cpu().numpy(), d16, ws


@pytest.mark.parametrize('fraction', [0.2, 1.0])
@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('b,npix', SHAPES)
def test_loss_and_gradient_against_the_reference(ops, b, npix, masked, fraction):
    o, t = case(b, npix, masked)
    l64, g64, b_loss, b_grad = R.bound(o, t, masked, fraction)
    l32, g32, _ = R.loss32(o, t, masked, fraction)
    cnt = R.counting(t, masked)
    loss, g, d16, ws = run(ops, o, t, masked, fraction, ld16=npix + 5)
    e_loss, e_c, e_grad = R.rel(loss[0], l64[0]), R.rel(loss[2], l64[2]), R.grad_err(g, g64)
    same = (bits(loss) == bits(l32)).all() and (bits(g) == bits(g32)).all()
    print(f'berhu ({b},{npix}) masked={masked} fraction={fraction}: loss {e_loss:.2e} threshold {e_c:.2e} (bound {b_loss:.2e}), '
          f'gradient {e_grad:.2e} (bound {b_grad:.2e}); loss {l64[0]:.6g} threshold {l64[2]:.6g} quadratic {l64[3]:.4g}; '
          f'the bits of the float32 restatement: {"yes" if same else "no"}')
    assert np.isfinite(loss).all() and l64[0] > 0
    assert e_loss <= b_loss and e_c <= b_loss
    assert e_grad <= b_grad
    # exact: the fraction of counting pixels, the counts, zeros at holes, a pull on every counting output that is off its target
    assert loss[1] == (F(cnt.sum() / (b * npix)) if masked else F(1))
    total = int(cnt.sum())
    assert abs(float(loss[3]) * total - l64[3] * total) <= R.ambiguous(o, t, masked, fraction) + 0.5
    assert loss[3] == 0 if fraction == 1.0 else npix < 15 or 0 < loss[3] < 1            # fraction 1: nothing is quadratic
    assert (bits(g[~cnt]) == 0).all()
    assert (g[cnt & (o != t)] != 0).all()
    neg = cnt & (o <= 0)
    assert npix < 15 or (neg.any() and (g[neg] < 0).all())                  # where the log loss has no gradient
    wsh = ws.cpu().numpy()
    np.testing.assert_array_equal(wsh[2:2 + 3 * b:3], cnt.sum(axis=1).astype(F))
    assert (wsh[3:3 + 3 * b:3] == 0).all()                                  # nobody is poisoned
    if masked and b >= 3:                                                   # the sample without a finite target
        assert (bits(g[b // 2]) == 0).all() and bits(wsh[1 + 3 * (b // 2)]) == 0
    # the bf16 copy: the (__bf16) cast of dout, the pitch columns untouched
    h16 = d16.float().cpu().numpy()
    np.testing.assert_array_equal(h16[:, :npix], torch.from_numpy(g).to(torch.bfloat16).float().numpy())
    assert (h16[:, npix:] == 7.0).all()


@pytest.mark.parametrize('b', [1, 2, 4])
def test_integer_inputs_bit_for_bit(ops, b):
    """|e| in {0 .. 4}, fraction 0.5: c = 2, rho in {0, 1, 2, 3.25, 5}, every other pixel a hole (with a larger error on it),
    r_n = 2: every float32 operation is exact, so the float64 reference is the answer element by element."""
    o, t = R.integer_case(b, 4070, seed=b)
    R.exact_conditions(o, t)
    l64, g64, c64 = R.loss64(o, t, 1, 0.5)
    l32, g32, _ = R.loss32(o, t, 1, 0.5)
    assert (bits(l32) == bits(l64)).all() and (bits(g32) == bits(g64)).all()
    loss, g, _, ws = run(ops, o, t, 1, 0.5)
    np.testing.assert_array_equal(bits(loss), bits(l64))
    np.testing.assert_array_equal(bits(g), bits(g64))
    assert loss[2] == 2 and loss[1] == 0.5 and (ws.cpu().numpy()[1:1 + 3 * b:3] == 2).all()
    cnt = np.isfinite(t)
    a = np.abs(o - np.where(cnt, t, 0))
    assert (np.abs(g[cnt & (a == 2)]) == F(2 / b)).all() and (cnt & (a == 2)).any()      # a == c: the pixel is linear
    assert (np.abs(g[cnt & (a == 3)]) == F(3 / b)).all()


def spike_case(where, npix=4070, hole_on_spike=False):
    """o == t but for whole-number errors: 8 at pixel `where`, 5 and -6 (quadratic against c = 4) and 4, -4, 2 (linear)."""
    t = np.full((1, npix), 3, F)
    o = t.copy()
    for k, e in ((where, 8), (npix // 2, 5), (npix // 2 + 1, -6), (npix // 3, 4), (npix // 3 + 1, -4), (7, 2)):
        o[0, k] = t[0, k] + e
    if hole_on_spike:
        t[0, where] = np.nan
    return o, t


@pytest.mark.parametrize('where', ['first', 'last'])
def test_the_maximum_at_either_end_of_a_sample(ops, where):
    npix = 4070
    o, t = spike_case(0 if where == 'first' else npix - 1)
    l64, g64, c64 = R.loss64(o, t, 0, 0.5)
    loss, g, _, ws = run(ops, o, t, 0, 0.5)
    assert c64[0] == 4 and float(ws[1]) == 4 and loss[2] == 4
    np.testing.assert_array_equal(bits(loss), bits(l64))          # whole numbers and eighths: exact
    np.testing.assert_array_equal(bits(g), bits(g64))
    assert loss[3] == F(3 / npix)                                  # 8, 5 and -6 are quadratic; 4 == c and -4 are linear


def test_the_largest_error_on_a_hole_does_not_set_the_threshold(ops):
    o, t = spike_case(0, hole_on_spike=True)
    l64, g64, c64 = R.loss64(o, t, 1, 0.5)
    loss, g, _, ws = run(ops, o, t, 1, 0.5)
    assert c64[0] == 3 and float(ws[1]) == 3 and bits(g[0, 0]) == 0
    assert R.rel(loss[0], l64[0]) <= 2 ** -22 and R.grad_err(g, g64) <= 2 ** -22      # r_n = 4070 / 4069 is not exact
    unmasked = run(ops, o, np.where(np.isfinite(t), t, F(3)), 0, 0.5)
    assert float(unmasked[3][1]) == 4 and unmasked[1][0, 0] != 0


def test_no_error_at_all(ops):
    t = R.case(3, 257, seed=2, masked=1)[1]
    o = np.where(np.isfinite(t), t, F(0.5)).astype(F)
    for masked in (0, 1):
        tt = t if masked else o
        loss, g, _, ws = run(ops, o, tt, masked, 0.2)
        assert (bits(g) == 0).all()
        assert bits(loss[0]) == 0 and bits(loss[2]) == 0 and bits(loss[3]) == 0 and not np.isnan(loss).any()
        assert (bits(ws.cpu().numpy()[1:1 + 9:3]) == 0).all()


def test_negative_errors_give_negative_gradients_of_the_same_magnitude(ops):
    o, t = R.integer_case(2, 258, seed=9)
    mirrored = np.where(np.isfinite(t), 2 * t - o, o).astype(F)             # whole numbers: e -> -e exactly
    loss, g, _, _ = run(ops, o, t, 1, 0.5)
    loss_m, g_m, _, _ = run(ops, mirrored, t, 1, 0.5)
    np.testing.assert_array_equal(bits(loss), bits(loss_m))
    np.testing.assert_array_equal(bits(g_m), bits(np.where(g == 0, g, -g)))
    assert (g < 0).any() and (g > 0).any() and ((o < t) == (g < 0))[np.isfinite(t)].all()


@pytest.mark.parametrize('what', ['nan_output', 'inf_output', 'nan_target', 'nan_output_masked'])
def test_poison_stays_in_its_sample(ops, what):
    masked = int(what == 'nan_output_masked')
    o, t = R.case(3, 257, seed=6, masked=masked)
    clean_loss, clean, _, _ = run(ops, o, t, masked, 0.2)
    o2, t2 = o.copy(), t.copy()
    row = 2 if masked else 1                                                # masked: sample 1 has no finite target
    k = int(np.flatnonzero(np.isfinite(t[row]))[100])
    if what == 'nan_target':
        t2[row, k] = np.nan
    else:
        o2[row, k] = np.inf if what == 'inf_output' else np.nan
    loss, g, d16, ws = run(ops, o2, t2, masked, 0.2, ld16=262)
    assert np.isnan(g[row]).all() and np.isnan(d16.float().cpu().numpy()[row, :257]).all()
    others = [r for r in range(3) if r != row]
    np.testing.assert_array_equal(bits(g[others]), bits(clean[others]))
    assert np.isnan(loss[[0, 2, 3]]).all() and loss[1] == clean_loss[1] and np.isfinite(clean_loss).all()
    wsh = ws.cpu().numpy()
    assert np.isnan(wsh[1 + 3 * row]) and wsh[3 + 3 * row] == 1 and (wsh[[3 + 3 * r for r in others]] == 0).all()
    if masked:                                                              # what sits on a hole poisons nobody
        o3 = o.copy()
        o3[~np.isfinite(t)] = np.inf
        loss3, g3, _, _ = run(ops, o3, t, 1, 0.2)
        np.testing.assert_array_equal(bits(loss3), bits(clean_loss))
        np.testing.assert_array_equal(bits(g3), bits(clean))


@pytest.mark.parametrize('npix', [4070, 4071])
@pytest.mark.parametrize('masked', [0, 1])
def test_no_sample_sees_another(ops, masked, npix):
    """The rows of a b = 4 call are the rows of two b = 2 calls on its halves times 0.5, bit for bit (at 4071 pixels the halves'
    rows also start at other offsets from the 16-byte grid than in the whole)."""
    o, t = R.case(4, npix, seed=8, masked=masked)
    if masked:
        t[2] = R.case(4, npix, seed=9, masked=1)[1][0]                      # an ordinary sample in place of the empty one
    loss, g, _, ws = run(ops, o, t, masked, 0.2)
    for half in (0, 1):
        rows = slice(2 * half, 2 * half + 2)
        loss_h, g_h, _, ws_h = run(ops, o[rows], t[rows], masked, 0.2)
        np.testing.assert_array_equal(bits(g[rows]), bits(g_h * F(0.5)))
        np.testing.assert_array_equal(bits(ws.cpu().numpy()[1 + 6 * half:7 + 6 * half]), bits(ws_h.cpu().numpy()[1:7]))
    assert (g != 0).any()


@pytest.mark.parametrize('masked', [0, 1])
def test_two_calls_on_one_workspace_and_two_runs_give_the_same_bits(ops, masked):
    o5, t5 = case(5, 4070, masked)
    o2, t2 = case(2, 2049, masked)
    ws = ops.berhu_ws(5, 'cuda')
    first = run(ops, o5, t5, masked, 0.2, ws=ws)
    small = run(ops, o2, t2, masked, 0.2, ws=ws)                            # a smaller batch on the same workspace
    again = run(ops, o5, t5, masked, 0.2, ws=ws)
    fresh = run(ops, o2, t2, masked, 0.2)
    for x, y in ((first, again), (small, fresh)):
        np.testing.assert_array_equal(bits(x[0]), bits(y[0]))
        np.testing.assert_array_equal(bits(x[1]), bits(y[1]))
    assert float(ws[0]) == 0


def test_bad_arguments(ops):
    x = torch.ones((2, 15), device='cuda')
    loss, ws = torch.zeros(4, device='cuda'), ops.berhu_ws(2, 'cuda')
    assert ws.numel() == 3 * 2 + 1 + 3 * 2 * 8                              # A3DH_WS_FLOATS(2)
    for bad in (0.0, -0.2, 1.5, float('nan')):
        with pytest.raises(ValueError, match='fraction'):
            ops.berhu_loss_fwd(x, x, 1, bad, loss, ws)
        with pytest.raises(ValueError, match='fraction'):
            ops.berhu_loss_bwd(x, x, 1, bad, ws, x.clone())
    torch.cuda.synchronize()
    assert float(ws[0]) == 0 and float(loss.abs().sum()) == 0               # nothing was launched
