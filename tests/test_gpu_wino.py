"""A3D_PREC_F32_WINOGRAD ('fp32w', csrc/wino.hip) on the GPU: forward (bias + ReLU) and bwd-data (with a ReLU mask) against
oracle.tf13_ops in float64 — rel-L2 below RTOL_F32 on normal operands, element for element on ternary ones (exact: the headroom
bound is asserted in tests/test_wino_cpu.py for these very cases) — with the filter transformed per call and prepared; guard
columns; the calls the route does not take; the timing record; run-to-run bits."""

import numpy as np
import pytest
import torch

import wino_ref as W
from oracle import tf13_ops as T

pytestmark = pytest.mark.gpu

RTOL_F32 = 1e-5
GUARD = 7.0


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def padded(a, ld):
    """a [..., c] on the device as the first c channels of pixels `ld` apart; the other channels hold GUARD"""
    t = torch.full(a.shape[:-1] + (ld,), GUARD, device='cuda')
    t[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def run(case, x, g, b, dz, mask, prepared, precision='fp32w'):
    """forward (bias + ReLU) and bwd-data (masked) of the case -> y [n,ho,wo,ldy], dx [n,h,w,ldx] as numpy"""
    from ann3depth_amd import ops
    n, h, w, c, k, padding, ldx, ldy = case
    ldx, ldy = ldx or c, ldy or k
    d = ops.conv_desc(n, h, w, c, k, 3, 3, 1, padding, ldx=ldx, ldy=ldy, precision=precision)
    xd, dzd, maskd = padded(x, ldx), padded(dz, ldy), padded(mask, ldx)
    gd, bd = torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda()
    y = torch.full((n, d.ho, d.wo, ldy), GUARD, device='cuda')
    dx = torch.full((n, h, w, ldx), GUARD, device='cuda')
    df, wf, db, wb = d, gd, d, gd
    if prepared:
        pf, pb = ops.PreparedFilter(d, xd.device), ops.PreparedFilter(d, xd.device, 'bwd_d')
        assert pf.ok and pb.ok
        pf.refresh(gd)
        pb.refresh(gd)
        df, wf, db, wb = pf.desc_prepared, pf.buf, pb.desc_prepared, pb.buf
    ops.conv2d_fwd(df, xd, wf, bd, y, 'relu')
    ops.conv2d_bwd_data(db, dzd, wb, dx, relu_mask=maskd)
    return y.cpu().numpy(), dx.cpu().numpy()


def operands(case, ternary):
    n, h, w, c, k, padding = case[:6]
    ho, wo, _, _ = W.geometry(h, w, padding)
    rng = np.random.default_rng(11)
    if ternary:
        draw = lambda shape: W.ternary(rng, shape)                      # noqa: E731
        g = draw((3, 3, c, k))
    else:
        draw = lambda shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
        g = (rng.standard_normal((3, 3, c, k)) / np.sqrt(9 * c)).astype(np.float32)
    return draw((n, h, w, c)), g, draw((k,)), draw((n, ho, wo, k)), draw((n, h, w, c))


def reference(case, x, g, b, dz, mask):
    padding = case[5]
    f = np.float64
    y = T.conv2d_fwd(x.astype(f), g.astype(f), b.astype(f), 1, padding, relu=True)
    dx = T.conv2d_bwd_data(dz.astype(f), g.astype(f), x.shape, 1, padding) * (mask > 0)
    return y, dx


@pytest.mark.parametrize('prepared', [False, True], ids=['per call', 'prepared'])
@pytest.mark.parametrize('case', W.CASES, ids=lambda c: 'x'.join(map(str, c[:6])))
def test_forward_and_bwd_data_against_float64(case, prepared):
    c, k = case[3], case[4]
    for ternary in (False, True):
        ops_ = operands(case, ternary)
        y_ref, dx_ref = reference(case, *ops_)
        y, dx = run(case, *ops_, prepared)
        if ternary:
            np.testing.assert_array_equal(y[..., :k], y_ref)
            np.testing.assert_array_equal(dx[..., :c], dx_ref)
        else:
            ry, rdx = rel_l2(y[..., :k], y_ref), rel_l2(dx[..., :c], dx_ref)
            print(f'rel-L2 fwd {ry:.3e} bwd-data {rdx:.3e}')
            assert ry < RTOL_F32 and rdx < RTOL_F32
        assert (y[..., k:] == GUARD).all() and (dx[..., c:] == GUARD).all()      # columns beyond k / c are never written


@pytest.mark.parametrize('shape', [(2, 11, 9, 16, 24, 5, 5, 1, 'SAME'), (2, 13, 18, 32, 48, 3, 3, 2, 'VALID')], ids=['5x5', 'stride 2'])
def test_calls_the_route_does_not_take_run_as_fp32(shape):
    from ann3depth_amd import ops
    n, h, w, c, k = shape[:5]
    rng = np.random.default_rng(12)
    probe = ops.conv_desc(*shape)
    x = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal(shape[5:7] + (c, k)).astype(np.float32)).cuda()
    dz = torch.from_numpy(rng.standard_normal((n, probe.ho, probe.wo, k)).astype(np.float32)).cuda()
    outs = {}
    for prec in ('fp32', 'fp32w'):
        d = ops.conv_desc(*shape, precision=prec)
        y, dx, dw = torch.empty_like(dz), torch.empty_like(x), torch.empty_like(g)
        ops.conv2d_fwd(d, x, g, None, y, 'relu')
        ops.conv2d_bwd_data(d, dz, g, dx, relu_mask=x)
        ops.conv2d_bwd_filter(d, x, dz, dw)
        outs[prec] = [t.cpu().numpy() for t in (y, dx, dw)]
    for a, b in zip(outs['fp32'], outs['fp32w']):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bwd_filter_of_a_3x3_layer_runs_as_fp32():
    from ann3depth_amd import ops
    rng = np.random.default_rng(13)
    shape = (2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    x = torch.from_numpy(rng.standard_normal((2, 6, 8, 32)).astype(np.float32)).cuda()
    dz = torch.from_numpy(rng.standard_normal((2, 4, 6, 200)).astype(np.float32)).cuda()
    got = []
    for prec in ('fp32', 'fp32w'):
        dw, db = torch.empty((3, 3, 32, 200), device='cuda'), torch.empty(200, device='cuda')
        ops.conv2d_bwd_filter(ops.conv_desc(*shape, precision=prec), x, dz, dw, db)
        got.append((dw.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and np.array_equal(got[0][1], got[1][1])


def test_one_timing_record_around_the_sixteen_products():
    from ann3depth_amd import _lib
    lib = _lib.load()
    case = W.CASES[3]
    n, h, w, c, k = case[:5]
    ops_ = operands(case, True)
    lib.a3d_timing_select(None)
    lib.a3d_timing_enable(1)
    try:
        run(case, *ops_, False)
        torch.cuda.synchronize()
    finally:
        lib.a3d_timing_enable(0)
    arr = (_lib.TimingRecord * 8)()
    recs = [arr[i] for i in range(lib.a3d_timing_collect(arr, 8))]
    assert len(recs) == 2
    fwd, bwd = recs
    tiles_f, tiles_b = n * 2 * 3, n * 3 * 4                         # 4x6 outputs, 6x8 input gradients
    for r, mode, m, nn, kk in ((fwd, 0, 16 * tiles_f, k, c), (bwd, 1, 16 * tiles_b, c, k)):
        assert (r.mode, r.prec, r.lds_dma, r.splitk) == (mode, 0, 0, 1)
        assert (r.bm, r.bn, r.waves_m, r.nwaves, r.bk, r.avec, r.bvec) == (128, 128, 4, 8, 32, 4, 4)
        assert (r.m, r.n, r.k) == (m, nn, kk) and r.flops == 2.0 * m * nn * kk and r.ms > 0


def test_two_runs_give_the_same_bits():
    case = W.CASES[0]
    ops_ = operands(case, False)
    y0, dx0 = run(case, *ops_, True)
    y1, dx1 = run(case, *ops_, True)
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and np.array_equal(dx0.view(np.uint32), dx1.view(np.uint32))


def test_dense_layers_run_as_fp32():
    """No 3x3 window in a dense layer: the _ex forms with 'fp32w' give the bits of 'fp32', forward, bwd-data and the fused
    filter gradient + ApplyAdam (never the bf16 kernels a value other than 'fp32' selects)."""
    from ann3depth_amd import ops
    rng = np.random.default_rng(14)
    m, k, n = 24, 200, 136
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()      # noqa: E731
    x, w, b, dz, mask = t(m, k), t(k, n), t(n), t(m, n), t(m, k)
    got = {}
    for prec in ('fp32', 'fp32w'):
        y, dx = torch.empty((m, n), device='cuda'), torch.empty((m, k), device='cuda')
        ops.dense_fwd_ex(x, w, b, y, 'relu', precision=prec)
        ops.dense_bwd_data_ex(dz, w, dx, mask=mask, precision=prec)
        var, m_w, v_w = w.clone(), torch.zeros_like(w), torch.zeros_like(w)
        ops.dense_bwd_filter_adam_tf1(x, dz, var, m_w, v_w, None, None, None, 1e-3, 0.9, 1.0, 0.9, 1.0, precision=prec)
        got[prec] = [a.cpu().numpy() for a in (y, dx, m_w)]
    for a, b_ in zip(got['fp32'], got['fp32w']):
        assert np.array_equal(a.view(np.uint32), b_.view(np.uint32))
