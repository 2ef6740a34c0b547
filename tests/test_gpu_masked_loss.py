"""a3dx_silog_masked_loss_fwd / a3dx_silog_masked_loss_bwd_ex on the GPU against tests/valid_ref.py in float64, at the
tolerances tests/test_gpu_ops.py::test_silog_loss holds the plain kernels to (2e-6 on the loss, 1e-5 rel-L2 on the gradient;
tests/test_valid_cpu.py shows a float32 numpy run of the formula near 1e-7 on these shapes), and bit for bit against the
plain kernels where no target is missing."""
import numpy as np
import pytest
import torch

import valid_ref as V

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4070), (2, 7), (65, 33)]       # the model grid; most of the 8 parts empty; more samples than the last block's lanes


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, o, t, ws=None, ld16=None):
    b, npix = o.shape
    ws = ops.silog_masked_ws(b, 'cuda') if ws is None else ws
    od, td = dev(o), dev(t)
    loss = torch.full((4,), 7.0, device='cuda')
    dout = torch.full((b, npix), 7.0, device='cuda')
    d16 = None if ld16 is None else torch.full((b, ld16), 7.0, device='cuda', dtype=torch.bfloat16)
    ops.silog_masked_loss_fwd(od, td, loss[:2], ws)
    ops.silog_masked_loss_bwd(od, td, ws, dout, d16)
    torch.cuda.synchronize()
    assert float(loss[2]) == 7.0 and float(loss[3]) == 7.0, 'the forward writes two floats'
    return loss[:2].cpu().numpy(), dout.cpu().numpy(), d16, ws


@pytest.mark.parametrize('b,npix', SHAPES)
def test_masked_loss_and_gradient_against_the_reference(ops, b, npix):
    o, t = V.loss_case(b, npix, seed=b)
    valid = np.isfinite(t)
    assert not valid[-1].any() and all(0.05 < 1 - v.mean() < 0.95 or npix < 10 for v in valid[:-1]) and (o < -1e-8).any()
    ref, frac = V.masked_silog_fwd(o.astype(np.float64), t.astype(np.float64))
    g_ref = V.masked_silog_bwd(o.astype(np.float64), t.astype(np.float64))
    ld16 = (npix + 7) // 8 * 8 + 8
    loss, g, d16, ws = run(ops, o, t, ld16=ld16)
    e_loss, e_grad = abs(float(loss[0]) - ref) / abs(ref), V.rel_l2(g, g_ref)
    print(f'masked silog b={b} npix={npix}: loss rel err {e_loss:.2e}, grad rel-L2 {e_grad:.2e}, valid {frac:.4f}')
    assert np.isfinite(loss[0]) and e_loss < 2e-6
    assert e_grad < 1e-5
    assert (g[~valid] == 0).all() and (g[o < -1e-8] == 0).all() and (g[-1] == 0).all()
    assert (g[valid & (o > 0)] != 0).any()
    assert loss[1] == np.float32(valid.sum() / (b * npix))                  # the exact valid fraction
    # the bf16 copy: the (__bf16) cast of dout, the pitch columns untouched
    h16 = d16.float().cpu().numpy()
    np.testing.assert_array_equal(h16[:, :npix], torch.from_numpy(g).to(torch.bfloat16).float().numpy())
    assert (h16[:, npix:] == 7.0).all()
    # per-sample sums left for the backward: n is the third
    w = ws.cpu().numpy()
    np.testing.assert_array_equal(w[3:3 + 3 * b:3], valid.sum(axis=1).astype(np.float32))
    assert w[0] == 0                                                        # the ticket wrapped back


def test_two_calls_on_one_workspace_give_the_same_bits(ops):
    o, t = V.loss_case(65, 33, seed=3)
    ws = ops.silog_masked_ws(65, 'cuda')
    first = run(ops, o, t, ws=ws)
    o3, t3 = V.loss_case(3, 4070, seed=4)
    small = run(ops, o3, t3, ws=ws)                                          # a smaller batch in between
    again = run(ops, o, t, ws=ws)
    np.testing.assert_array_equal(first[0].view(np.uint32), again[0].view(np.uint32))
    np.testing.assert_array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
    fresh = run(ops, o3, t3)
    np.testing.assert_array_equal(small[0].view(np.uint32), fresh[0].view(np.uint32))
    np.testing.assert_array_equal(small[1].view(np.uint32), fresh[1].view(np.uint32))
    assert float(ws[0]) == 0


def test_without_holes_at_the_model_grid_the_bits_are_the_plain_kernels(ops):
    b, npix = 32, 4070
    o, t = V.loss_case(b, npix, seed=5, invalid=0.0)
    assert np.isfinite(t).all() and (o < -1e-8).any()
    od, td = dev(o), dev(t)
    loss, lossm = torch.zeros(1, device='cuda'), torch.zeros(2, device='cuda')
    ws, wsm = ops.silog_ws(b, 'cuda'), ops.silog_masked_ws(b, 'cuda')
    g, gm = torch.empty((b, npix), device='cuda'), torch.empty((b, npix), device='cuda')
    g16 = torch.zeros((b, 4072), device='cuda', dtype=torch.bfloat16)
    gm16 = torch.zeros((b, 4072), device='cuda', dtype=torch.bfloat16)
    ops.silog_loss_fwd(od, td, loss, ws)
    ops.silog_loss_bwd(od, td, ws, g, g16)
    ops.silog_masked_loss_fwd(od, td, lossm, wsm)
    ops.silog_masked_loss_bwd(od, td, wsm, gm, gm16)
    torch.cuda.synchronize()
    assert torch.equal(loss, lossm[:1]) and float(lossm[1]) == 1.0
    assert torch.equal(g, gm) and torch.equal(g16, gm16)
    assert np.isfinite(float(loss)) and float(g.abs().sum()) > 0


def test_bad_arguments(ops):
    from ann3depth_amd import _lib
    lib = _lib.load()
    x = torch.ones((2, 8), device='cuda')
    loss, ws = torch.zeros(2, device='cuda'), ops.silog_masked_ws(2, 'cuda')
    assert lib.a3dx_silog_masked_loss_fwd(2, 8, x.data_ptr(), None, loss.data_ptr(), ws.data_ptr(), None) == -1
    assert lib.a3dx_silog_masked_loss_fwd(0, 8, x.data_ptr(), x.data_ptr(), loss.data_ptr(), ws.data_ptr(), None) == -1
    assert lib.a3dx_silog_masked_loss_bwd_ex(2, 8, x.data_ptr(), x.data_ptr(), ws.data_ptr(), x.data_ptr(), x.data_ptr(), 4,
                                            None) == -1                      # a bf16 pitch below npix
    assert ws.numel() == 3 * 2 + 1 + 3 * 2 * 8                              # A3DX_SILOG_MASKED_WS_FLOATS(2)
