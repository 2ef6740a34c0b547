"""The 1-D Winograd F(4,5) route (include/a3d_wino1d.h, csrc/wino1d.hip) on the GPU, on the cases of tests/wino1d_ref.py: dx, dw
and db against oracle.tf13_ops in float64 under the two bounds of tests/test_wino1d_cpu.py (rel-L2 below RTOL_F32, and element
by element RTOL_F32 times the same convolution of absolute values), with and without the ReLU mask, with a prepared and a
per-call filter (the same bits), with db wanted and not, at one split and at uneven ones; guard values beyond the channels of a
wider pixel stride and around dw and db; run-to-run bits; the timing records; the descriptors the route hands on; a short
workspace; and the coarse step of MSDNReplica with the routes forced on against the same step with them forced off.

Measured on an MI355X (rel-L2 / worst element as a multiple of its scale), largest over the cases: see DESIGN.md 3.1l."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import wino1d_ref as W1
from oracle import tf13_ops as T

pytestmark = pytest.mark.gpu

RTOL_F32 = 1e-5
GUARD = 7.0


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def within(what, got, ref, scale):
    r = rel_l2(got, ref)
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f'{what}: rel-L2 {r:.3e}, worst element {worst:.3e} of its scale')
    assert r < RTOL_F32 and (err <= RTOL_F32 * scale).all(), (what, r, worst)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def host(case):
    """operands of the case and its float64 references, computed once: dx and (dw, db) with their scales"""
    n, h, w, c, k, r, padding = case[:7]
    f = np.float64
    x, dz, wt, relu = W1.operands(case, 51)
    shape = (r, 5, c, k)
    dx = T.conv2d_bwd_data(dz.astype(f), wt.astype(f), (n, h, w, c), 1, padding)
    dx_scale = T.conv2d_bwd_data(np.abs(dz).astype(f), np.abs(wt).astype(f), (n, h, w, c), 1, padding)
    grads = T.conv2d_bwd_filter(x.astype(f), dz.astype(f), shape, 1, padding)
    scales = T.conv2d_bwd_filter(np.abs(x).astype(f), np.abs(dz).astype(f), shape, 1, padding)
    return dict(x=x, dz=dz, w=wt, relu=relu, dx=dx, dx_scale=dx_scale, grads=grads, scales=scales)


def padded(a, ld):
    """a [..., c] on the device as the first c channels of pixels `ld` apart; the other channels hold GUARD"""
    t = torch.full(a.shape[:-1] + (ld,), GUARD, device='cuda')
    t[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def guarded(shape, lead=64):
    n = int(np.prod(shape))
    big = torch.full((lead + n + 64,), GUARD, device='cuda')
    return big, big[lead:lead + n].view(shape)


def outside_is_untouched(big, n, lead=64):
    b = big.cpu().numpy()
    return (b[:lead] == GUARD).all() and (b[lead + n:] == GUARD).all()


def desc_of(case):
    from ann3depth_amd import ops
    n, h, w, c, k, r, padding, ldx, ldy = case
    return ops.conv_desc(n, h, w, c, k, r, 5, 1, padding, ldx=ldx or c, ldy=ldy or k)


def collect(lib, records):
    from ann3depth_amd import _lib
    lib.a3d_timing_enable(0)
    arr = (_lib.TimingRecord * 8)()
    records.extend(arr[i] for i in range(lib.a3d_timing_collect(arr, 8)))


def run_bwd_data(case, mask=False, prepared=False, records=None):
    """a3dl_conv2d_bwd_data of the case -> dx as numpy; asserts that the channels beyond c were not written"""
    from ann3depth_amd import _lib, ops
    n, h, w, c, k, r, padding, ldx, ldy = case
    hs = host(case)
    d = desc_of(case)
    dzd = padded(hs['dz'], d.ldy)
    wd = torch.from_numpy(hs['w']).cuda()
    md = padded(hs['relu'], d.ldx) if mask else None
    dx = torch.full((n, h, w, d.ldx), GUARD, device='cuda')
    if prepared:
        pf = ops.PreparedFilter(d, dzd.device, 'bwd_d_wino1d')
        assert pf.ok
        pf.refresh(wd)
        d, wd = pf.desc_prepared, pf.buf
    lib = _lib.load()
    if records is not None:
        lib.a3d_timing_select(None)
        lib.a3d_timing_enable(1)
    try:
        ops.conv2d_bwd_data_wino1d(d, dzd, wd, dx, relu_mask=md)
        torch.cuda.synchronize()
    finally:
        if records is not None:
            collect(lib, records)
    assert (dx[..., c:] == GUARD).all() and (dzd[..., k:] == GUARD).all()
    return dx[..., :c].cpu().numpy()


def run_bwd_filter(case, want_db=True, records=None):
    """a3dl_conv2d_bwd_filter of the case -> dw, db as numpy; asserts that nothing around them was written"""
    from ann3depth_amd import _lib, ops
    n, h, w, c, k, r, padding, ldx, ldy = case
    hs = host(case)
    d = desc_of(case)
    xd, dzd = padded(hs['x'], d.ldx), padded(hs['dz'], d.ldy)
    dw_big, dw = guarded((r, 5, c, k))
    db_big, db = guarded((k,))
    lib = _lib.load()
    if records is not None:
        lib.a3d_timing_select(None)
        lib.a3d_timing_enable(1)
    try:
        ops.conv2d_bwd_filter_wino1d(d, xd, dzd, dw, db if want_db else None)
        torch.cuda.synchronize()
    finally:
        if records is not None:
            collect(lib, records)
    assert outside_is_untouched(dw_big, r * 5 * c * k) and outside_is_untouched(db_big, k)
    assert (xd[..., c:] == GUARD).all() and (dzd[..., k:] == GUARD).all()
    if not want_db:
        assert (db == GUARD).all()
    return dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize('case', W1.CASES, ids=W1.case_id)
def test_bwd_data_against_float64(case):
    """Per-call filter without a mask, prepared filter with one: both bounds; the prepared filter and a second run give the
    per-call run's bits."""
    hs = host(case)
    recs = []
    dx = run_bwd_data(case, records=recs)
    within('dx', dx, hs['dx'], hs['dx_scale'])
    g = W1.bwd_data_geometry(*case[:7])
    assert len(recs) == 1 and (recs[0].mode, recs[0].prec, recs[0].lds_dma, recs[0].splitk) == (1, 0, 0, 1)
    assert (recs[0].bm, recs[0].bn, recs[0].nwaves) == (128, g['bn'], 4 if g['bn'] == 96 else 8)
    assert (recs[0].m, recs[0].n, recs[0].k) == (8 * g['pm'], case[3], case[5] * case[4]) and recs[0].ms > 0
    assert np.array_equal(bits(dx), bits(run_bwd_data(case, prepared=True)))
    assert np.array_equal(bits(dx), bits(run_bwd_data(case)))
    keep = hs['relu'] > 0
    dxm = run_bwd_data(case, mask=True, prepared=True)
    within('dx masked', dxm, hs['dx'] * keep, hs['dx_scale'] * keep)
    assert np.array_equal(bits(dxm), bits(np.where(keep, dx, np.float32(0))))


@pytest.mark.parametrize('case', W1.CASES, ids=W1.case_id)
def test_bwd_filter_against_float64(case):
    """dw and db under both bounds, at the rule's split count (one for most cases, 6 + 6 + 5 and 7 + 7 + 7 + 5 k-tiles for the two
    large ones); without db the same dw; a second run the same bits."""
    n, h, w, c, k, r, padding = case[:7]
    hs = host(case)
    recs = []
    dw, db = run_bwd_filter(case, records=recs)
    ho, wo, _, _ = W1.geometry(h, w, r, padding)
    pixels = n * ho * -(-wo // 4)
    assert len(recs) == 1 and recs[0].splitk == W1.grad_splits(r * W1.pad4(c), W1.pad4(k), pixels)
    assert (recs[0].mode, recs[0].prec, recs[0].lds_dma) == (2, 0, 0)
    assert (recs[0].bm, recs[0].bn, recs[0].waves_m, recs[0].nwaves, recs[0].bk, recs[0].avec, recs[0].bvec) == (128, 128, 4, 8, 32, 4, 4)
    assert (recs[0].m, recs[0].n, recs[0].k) == (r * c, k, 8 * pixels) and recs[0].flops == 2.0 * r * c * k * 8 * pixels
    within('dw', dw, hs['grads'][0], hs['scales'][0])
    within('db', db, hs['grads'][1], hs['scales'][1])
    dw2, _ = run_bwd_filter(case, want_db=False)
    assert np.array_equal(bits(dw), bits(dw2))
    dw3, db3 = run_bwd_filter(case)
    assert np.array_equal(bits(dw), bits(dw3)) and np.array_equal(bits(db), bits(db3))


@pytest.mark.parametrize('shape', [(2, 13, 18, 32, 48, 3, 3, 1, 'SAME'), (2, 11, 19, 16, 24, 5, 5, 2, 'SAME')], ids=['3x3', 'stride 2'])
def test_descriptors_the_route_does_not_take_run_the_direct_kernels(shape):
    from ann3depth_amd import ops
    n, h, w, c, k = shape[:5]
    rng = np.random.default_rng(52)
    d = ops.conv_desc(*shape)
    x = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)).cuda()
    dz = torch.from_numpy(rng.standard_normal((n, d.ho, d.wo, k)).astype(np.float32)).cuda()
    wt = torch.from_numpy(rng.standard_normal(shape[5:7] + (c, k)).astype(np.float32)).cuda()
    got = []
    for bwd_f, bwd_d in ((ops.conv2d_bwd_filter, ops.conv2d_bwd_data), (ops.conv2d_bwd_filter_wino1d, ops.conv2d_bwd_data_wino1d)):
        dw, db, dx = torch.empty_like(wt), torch.empty(k, device='cuda'), torch.empty_like(x)
        bwd_f(d, x, dz, dw, db)
        bwd_d(d, dz, wt, dx, relu_mask=x)
        got.append([t.cpu().numpy() for t in (dw, db, dx)])
    for a, b in zip(*got):
        assert np.array_equal(bits(a), bits(b))


def test_a_workspace_one_byte_short_is_refused_and_nothing_written():
    from ann3depth_amd import _lib
    lib = _lib.load()
    case = W1.CASES[3]
    n, h, w, c, k, r, padding = case[:7]
    hs = host(case)
    d = desc_of(case)
    x, dz, wt = (torch.from_numpy(hs[a]).cuda() for a in ('x', 'dz', 'w'))
    dw, db, dx = (torch.full(s, GUARD, device='cuda') for s in ((r, 5, c, k), (k,), (n, h, w, c)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    need = lib.a3dl_conv2d_bwd_filter_ws_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    assert lib.a3dl_conv2d_bwd_filter(ctypes.byref(d), p(x), p(dz), p(dw), p(db), p(ws), need - 1, None) == -2
    need = lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d))
    ws2 = torch.empty(need, dtype=torch.uint8, device='cuda')
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), p(dz), p(wt), p(dx), None, p(ws2), need - 1, None) == -2
    torch.cuda.synchronize()
    assert 'workspace' in _lib.last_error()
    assert all(bool((t == GUARD).all()) for t in (dw, db, dx))
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), p(dz), p(wt), p(dx), None, p(ws2), need, None) == 0      # the queried size is enough
    torch.cuda.synchronize()
    within('dx', dx.cpu().numpy(), hs['dx'], hs['dx_scale'])


def test_the_coarse_step_with_the_routes_against_the_direct_kernels():
    """B = 8: both losses, both maps and every gradient but conv2d_1's and conv2d_0's kernel and bias gradients are the direct
    step's bits; those four differ by rounding alone."""
    from ann3depth_amd import models
    from oracle import msdn as O
    B = 8
    rng = np.random.default_rng(53)
    img = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)).cuda()
    dep = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 1)) / 255).astype(np.float32)).cuda()
    keep = torch.from_numpy(rng.random((B, 4096)) >= 0.5).cuda()
    params = O.init_params(3000)

    class Routes(models.MSDNReplica):
        WINO1D_BWD_D_MIN_ROWS = WINO1D_BWD_F_MIN_ROWS = 1

    class Direct(models.MSDNReplica):
        WINO1D_BWD_D_MIN_ROWS = WINO1D_BWD_F_MIN_ROWS = 1 << 30

    nets = [Routes(B, device='cuda:0', params=params), Direct(B, device='cuda:0', params=params)]
    layers = set(models.MSDNReplica.WINO1D_LAYERS)
    assert nets[0].wino1d_bwd_d == nets[0].wino1d_bwd_f == layers and not nets[1].wino1d_bwd_d and not nets[1].wino1d_bwd_f
    outs = [net.step(img, dep, keep) for net in nets]
    torch.cuda.synchronize()
    tbits = lambda t: t.detach().cpu().numpy().view(np.uint32)      # noqa: E731
    for key in ('coarse_loss', 'fine_loss'):
        assert np.float32(float(outs[0][key])).view(np.uint32) == np.float32(float(outs[1][key])).view(np.uint32), key
    for key in ('coarse', 'fine'):
        assert np.array_equal(tbits(getattr(nets[0], key)), tbits(getattr(nets[1], key))), key
    moved = [layer + suffix for layer in ('coarse/conv/conv2d_1', 'coarse/conv/conv2d_0') for suffix in ('/kernel', '/bias')]
    for name in nets[0].shapes:
        if not name.startswith('coarse/'):
            continue
        a, b = nets[0].grad(name), nets[1].grad(name)
        if name in moved:
            r = rel_l2(a.cpu().numpy(), b.cpu().numpy())
            print(f'{name}: rel-L2 {r:.3e}')
            assert 0 < r < RTOL_F32, name
        else:
            assert np.array_equal(tbits(a), tbits(b)), name
