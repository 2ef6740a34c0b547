"""a3dg_silog_grad_loss_fwd / a3dg_silog_grad_loss_bwd_ex on the GPU against tests/gradloss_ref.py in float64, at 8 x the error
the float32 restatement shows on the same inputs (never looser than the 2e-6 / 1e-5 of tests/test_gpu_masked_loss.py), exactly
where the header promises exact values, and bit for bit against the plain and the masked kernels where it promises their bits."""
import numpy as np
import pytest
import torch

import gradloss_ref as G

pytestmark = pytest.mark.gpu

F = np.float32
# no pair; one row; one column; end-of-row pairs a large share; a row longer than a part's chunk; more samples than the last
# block's lanes; the model grid; and two the walk over a chunk needs: a part of two rounds with rows longer than a round, and
# parts of 132 rounds with more bands than the backward launch has blocks
SHAPES = [(2, 1, 1), (2, 1, 7), (2, 7, 1), (3, 3, 5), (2, 2, 600), (65, 3, 11), (3, 55, 74), (2, 9, 1100), (2, 2100, 513)]
BIT_SHAPES = [(32, 55, 74), (2, 3, 5), (2, 2, 600), (2, 9, 1100)]


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CASES = {}


def case(b, h, w, masked):
    """Inputs, float64 references and bounds of one shape, computed once and shared by the weights."""
    key = (b, h, w, masked)
    if key not in _CASES:
        o, t = G.loss_case(b, h, w, seed=b + h, invalid=None if masked else 0)
        _CASES[key] = (o, t) + G.tolerances(o, t, h, w, masked)
    return _CASES[key]


def run(ops, o, t, h, w, masked, weight, ws=None, ld16=None):
    b = o.shape[0]
    ws = ops.silog_grad_ws(b, 'cuda') if ws is None else ws
    od, td = dev(o), dev(t)
    loss = torch.full((6,), 7.0, device='cuda')
    dout = torch.full((b, h * w), 7.0, device='cuda')
    d16 = None if ld16 is None else torch.full((b, ld16), 7.0, device='cuda', dtype=torch.bfloat16)
    ops.silog_grad_loss_fwd(od, td, h, w, masked, weight, loss[:4], ws)
    ops.silog_grad_loss_bwd(od, td, h, w, masked, weight, ws, dout, d16)
    torch.cuda.synchronize()
    assert float(loss[4]) == 7.0 and float(loss[5]) == 7.0, 'the forward writes four floats'
    return loss[:4].cpu().numpy(), dout.cpu().numpy(), d16, ws


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('weight', G.WEIGHTS)
@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_loss_and_gradient_against_the_reference(ops, b, h, w, masked, weight):
    o, t, refs, b_loss, b_grad = case(b, h, w, masked)
    (ref, g_ref), npix = refs[weight], h * w
    valid = np.isfinite(t) if masked else np.ones(t.shape, bool)
    ld16 = (npix + 7) // 8 * 8 + 8
    loss, g, d16, ws = run(ops, o, t, h, w, masked, weight, ld16=ld16)
    assert b_loss > 0 and b_grad > 0
    b_loss, b_grad = min(b_loss, 2e-6), min(b_grad, 1e-5)           # never looser than the masked loss's tolerances
    errs = {k: G.rel(loss[k], ref[k]) for k in (0, 2, 3)}
    e_grad = G.rel_l2(g, g_ref)
    print(f'gradloss ({b},{h},{w}) masked={masked} weight={weight}: total {errs[0]:.2e} silog {errs[2]:.2e} grad term '
          f'{errs[3]:.2e} (bound {b_loss:.2e}), gradient rel-L2 {e_grad:.2e} (bound {b_grad:.2e}); total {ref[0]:.6g} '
          f'silog {ref[2]:.6g} grad term {ref[3]:.6g}')
    assert np.isfinite(loss).all() and max(errs.values()) <= b_loss
    assert e_grad <= b_grad
    # exact: zeros, the fraction, the counts, the total's two roundings
    assert (g[~valid] == 0).all() and (g[o < -1e-8] == 0).all() and (not masked or (g[-1] == 0).all())
    assert (g[valid & (o > 0)] != 0).any()
    assert loss[1] == (F(valid.sum() / (b * npix)) if masked else F(1))
    assert bits(loss[:1])[0] == bits(np.array([F(loss[2] + F(F(weight) * loss[3]))]))[0]
    wsh = ws.cpu().numpy()
    v3 = valid.reshape(b, h, w)
    pairs = (v3[:, :, 1:] & v3[:, :, :-1]).reshape(b, -1).sum(axis=1) + (v3[:, 1:] & v3[:, :-1]).reshape(b, -1).sum(axis=1)
    np.testing.assert_array_equal(wsh[3:3 + 5 * b:5], valid.sum(axis=1).astype(F))
    np.testing.assert_array_equal(wsh[5:5 + 5 * b:5], pairs.astype(F))
    assert masked or (pairs == h * (w - 1) + (h - 1) * w).all()
    assert wsh[0] == 0                                                      # the ticket wrapped back
    # the bf16 copy: the (__bf16) cast of dout, the pitch columns untouched
    h16 = d16.float().cpu().numpy()
    np.testing.assert_array_equal(h16[:, :npix], torch.from_numpy(g).to(torch.bfloat16).float().numpy())
    assert (h16[:, npix:] == 7.0).all()
    if npix == 1:                                                           # no pair: the silog gradient alone
        assert loss[3] == 0 and (wsh[5:5 + 5 * b:5] == 0).all() and (wsh[4:4 + 5 * b:5] == 0).all()
        np.testing.assert_array_equal(bits(g), bits(run(ops, o, t, h, w, masked, 0.0)[1]))


@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('b,h,w', BIT_SHAPES)
def test_silog_part_and_weight_zero_are_the_existing_kernels_bits(ops, b, h, w, masked):
    npix = h * w
    o, t = G.loss_case(b, h, w, seed=5, invalid=None if masked else 0)
    assert (o < -1e-8).any() and np.isfinite(t).all() != bool(masked)
    od, td = dev(o), dev(t)
    ld16 = (npix + 7) // 8 * 8
    want = torch.zeros(2, device='cuda')
    g = torch.empty((b, npix), device='cuda')
    g16 = torch.zeros((b, ld16), device='cuda', dtype=torch.bfloat16)
    if masked:
        ws = ops.silog_masked_ws(b, 'cuda')
        ops.silog_masked_loss_fwd(od, td, want, ws)
        ops.silog_masked_loss_bwd(od, td, ws, g, g16)
    else:
        ws = ops.silog_ws(b, 'cuda')
        ops.silog_loss_fwd(od, td, want[:1], ws)
        ops.silog_loss_bwd(od, td, ws, g, g16)
        want[1] = 1.0
    for weight in (0.0, 0.5):
        loss = torch.zeros(4, device='cuda')
        wsg = ops.silog_grad_ws(b, 'cuda')
        gg = torch.empty((b, npix), device='cuda')
        gg16 = torch.zeros((b, ld16), device='cuda', dtype=torch.bfloat16)
        ops.silog_grad_loss_fwd(od, td, h, w, masked, weight, loss, wsg)
        ops.silog_grad_loss_bwd(od, td, h, w, masked, weight, wsg, gg, gg16)
        torch.cuda.synchronize()
        assert torch.equal(loss[2:3].view(torch.int32), want[:1].view(torch.int32)) and np.isfinite(float(loss[2]))
        assert torch.equal(loss[1:2], want[1:2])
        assert float(loss[3]) > 0
        if weight == 0:
            assert torch.equal(loss[:1].view(torch.int32), loss[2:3].view(torch.int32))
            assert torch.equal(gg.view(torch.int32), g.view(torch.int32)) and torch.equal(gg16.view(torch.int16), g16.view(torch.int16))
            assert float(gg.abs().sum()) > 0
        else:
            assert not torch.equal(gg, g)


@pytest.mark.parametrize('masked', [0, 1])
def test_a_constant_error_has_no_gradient_term(ops, masked):
    b, h, w = 3, 55, 74
    o, t = G.constant_case(b, h, w, masked)
    loss1, g1, _, ws = run(ops, o, t, h, w, masked, 1.0)
    loss0, g0, _, _ = run(ops, o, t, h, w, masked, 0.0)
    assert loss1[3] == 0 and loss0[3] == 0 and (ws.cpu().numpy()[4:4 + 5 * b:5] == 0).all()          # sg == 0.0
    np.testing.assert_array_equal(bits(g1), bits(g0))
    np.testing.assert_array_equal(bits(loss1[[0, 2]]), bits(loss0[[0, 2]]))
    assert (g0 != 0).any() and loss0[2] > 0


@pytest.mark.parametrize('masked', [0, 1])
def test_two_calls_on_one_workspace_give_the_same_bits(ops, masked):
    o, t = case(65, 3, 11, masked)[:2]
    o3, t3 = case(3, 55, 74, masked)[:2]
    ws = ops.silog_grad_ws(65, 'cuda')
    first = run(ops, o, t, 3, 11, masked, 0.5, ws=ws)
    small = run(ops, o3, t3, 55, 74, masked, 0.5, ws=ws)                     # a smaller batch in between
    again = run(ops, o, t, 3, 11, masked, 0.5, ws=ws)
    np.testing.assert_array_equal(bits(first[0]), bits(again[0]))
    np.testing.assert_array_equal(bits(first[1]), bits(again[1]))
    fresh = run(ops, o3, t3, 55, 74, masked, 0.5)
    np.testing.assert_array_equal(bits(small[0]), bits(fresh[0]))
    np.testing.assert_array_equal(bits(small[1]), bits(fresh[1]))
    assert float(ws[0]) == 0


def test_bad_arguments(ops):
    x = torch.ones((2, 15), device='cuda')
    loss, ws = torch.zeros(4, device='cuda'), ops.silog_grad_ws(2, 'cuda')
    assert ws.numel() == 5 * 2 + 1 + 5 * 2 * 8                              # A3DG_WS_FLOATS(2)
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='grad_weight'):
            ops.silog_grad_loss_fwd(x, x, 3, 5, 1, bad, loss, ws)
        with pytest.raises(ValueError, match='grad_weight'):
            ops.silog_grad_loss_bwd(x, x, 3, 5, 1, bad, ws, x.clone())
    from ann3depth_amd import _lib
    with pytest.raises(_lib.A3dError, match='A3DG_MAX_W'):
        ops.silog_grad_loss_fwd(torch.ones((1, 4096), device='cuda'), torch.ones((1, 4096), device='cuda'), 1, 4096, 0, 0.5, loss, ws)
    torch.cuda.synchronize()
    assert float(ws[0]) == 0 and float(loss.abs().sum()) == 0               # nothing was launched
