"""The Winograd filter-gradient route (include/a3d_wino_grad.h, csrc/wino.hip) on the GPU: dw and db against oracle.tf13_ops in
float64 — element for element on ternary operands (exact: the headroom bound is asserted in tests/test_wino_grad_cpu.py for
these very cases), rel-L2 below RTOL_F32 on normal ones — at one split and at five uneven ones; guard values around dw, db and
in the extra columns of x / dz; run-to-run bits; the timing record; the descriptors the route hands on; a short workspace; and
the coarse step of MSDNReplica with the route against the same step on the direct kernels."""
import ctypes

import numpy as np
import pytest
import torch

import wino_grad_ref as WG
import wino_ref as W
from oracle import tf13_ops as T

pytestmark = pytest.mark.gpu

RTOL_F32 = 1e-5
GUARD = 7.0
# W.CASES (n = 3 of the 13x18 layers: 189 tiles, one split, a partial last k-tile) and the 13x18 layers at n = 13, the smallest
# batch the rule splits unevenly: 819 tiles, 26 k-tiles dealt to five splits as 6 + 6 + 6 + 6 + 2
CASES = list(W.CASES) + [(13, 13, 18, 256, 384, 'SAME', None, None), (13, 13, 18, 384, 256, 'SAME', None, None)]


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def padded(a, ld):
    """a [..., c] on the device as the first c channels of pixels `ld` apart; the other channels hold GUARD"""
    t = torch.full(a.shape[:-1] + (ld,), GUARD, device='cuda')
    t[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def guarded(shape, lead):
    """a GUARD-filled allocation and the view of `shape` that starts `lead` floats into it"""
    n = int(np.prod(shape))
    big = torch.full((lead + n + 64,), GUARD, device='cuda')
    return big, big[lead:lead + n].view(shape)


def outside_is_untouched(big, lead, n):
    b = big.cpu().numpy()
    return (b[:lead] == GUARD).all() and (b[lead + n:] == GUARD).all()


def operands(case, ternary, seed=31):
    n, h, w, c, k, padding = case[:6]
    ho, wo, _, _ = W.geometry(h, w, padding)
    rng = np.random.default_rng(seed)
    if ternary:
        return W.ternary(rng, (n, h, w, c)), W.ternary(rng, (n, ho, wo, k))
    return rng.standard_normal((n, h, w, c)).astype(np.float32), rng.standard_normal((n, ho, wo, k)).astype(np.float32)


def run(case, x, dz, lead=64, want_db=True, records=None):
    """a3dwg_conv2d_bwd_filter of the case -> dw, db as numpy; asserts that nothing around them was written"""
    from ann3depth_amd import _lib, ops
    n, h, w, c, k, padding, ldx, ldy = case
    ldx, ldy = ldx or c, ldy or k
    d = ops.conv_desc(n, h, w, c, k, 3, 3, 1, padding, ldx=ldx, ldy=ldy)
    xd, dzd = padded(x, ldx), padded(dz, ldy)
    dw_big, dw = guarded((3, 3, c, k), lead)
    db_big, db = guarded((k,), lead)
    lib = _lib.load()
    if records is not None:
        lib.a3d_timing_select(None)
        lib.a3d_timing_enable(1)
    try:
        ops.conv2d_bwd_filter_wino(d, xd, dzd, dw, db if want_db else None)
        torch.cuda.synchronize()
    finally:
        if records is not None:
            lib.a3d_timing_enable(0)
            arr = (_lib.TimingRecord * 8)()
            records.extend(arr[i] for i in range(lib.a3d_timing_collect(arr, 8)))
    assert outside_is_untouched(dw_big, lead, 9 * c * k) and outside_is_untouched(db_big, lead, k)
    assert (xd[..., c:] == GUARD).all() and (dzd[..., k:] == GUARD).all()
    if not want_db:
        assert (db == GUARD).all()
    return dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:6])))
def test_dw_and_db_against_float64(case):
    n, h, w, c, k, padding = case[:6]
    tiles = n * -(-W.geometry(h, w, padding)[0] // 2) * -(-W.geometry(h, w, padding)[1] // 2)
    for ternary in (True, False):
        x, dz = operands(case, ternary)
        dw_ref, db_ref = T.conv2d_bwd_filter(x.astype(np.float64), dz.astype(np.float64), (3, 3, c, k), 1, padding)
        recs = []
        dw, db = run(case, x, dz, records=recs)
        assert len(recs) == 1 and recs[0].splitk == WG.splits(c, k, tiles)
        if (h, w) == (13, 18) and c >= 256:
            assert recs[0].splitk == (1 if n == 3 else 5)
        if ternary:
            np.testing.assert_array_equal(dw, dw_ref)
            np.testing.assert_array_equal(db, db_ref)
        else:
            rw, rb = rel_l2(dw, dw_ref), rel_l2(db, db_ref)
            print(f'rel-L2 dw {rw:.3e} db {rb:.3e}')
            assert rw < RTOL_F32 and rb < RTOL_F32


@pytest.mark.parametrize('case', [CASES[3], CASES[2]], ids=['vector', 'scalar'])
def test_off_the_16_byte_grid_and_without_db(case):
    """dw and db one float off the 16-byte grid, behind the vector and the scalar form of the transforms; a call that wants no db."""
    c, k, padding = case[3], case[4], case[5]
    x, dz = operands(case, True)
    dw_ref, db_ref = T.conv2d_bwd_filter(x.astype(np.float64), dz.astype(np.float64), (3, 3, c, k), 1, padding)
    dw, db = run(case, x, dz, lead=61)
    np.testing.assert_array_equal(dw, dw_ref)
    np.testing.assert_array_equal(db, db_ref)
    dw, _ = run(case, x, dz, want_db=False)
    np.testing.assert_array_equal(dw, dw_ref)


def test_two_runs_give_the_same_bits():
    case = CASES[-2]                                                 # five splits
    x, dz = operands(case, False)
    dw0, db0 = run(case, x, dz)
    dw1, db1 = run(case, x, dz)
    assert np.array_equal(dw0.view(np.uint32), dw1.view(np.uint32)) and np.array_equal(db0.view(np.uint32), db1.view(np.uint32))


def test_one_timing_record_around_the_sixteen_products():
    case = CASES[3]                                                  # (2, 6, 8, 32, 200, VALID): 4x6 outputs, 2x3 tiles an image
    n, c, k = case[0], case[3], case[4]
    recs = []
    run(case, *operands(case, True), records=recs)
    assert len(recs) == 1
    r = recs[0]
    tiles = n * 2 * 3
    assert (r.mode, r.prec, r.lds_dma, r.splitk) == (2, 0, 0, 1)
    assert (r.bm, r.bn, r.waves_m, r.nwaves, r.bk, r.avec, r.bvec) == (128, 128, 4, 8, 32, 4, 4)
    assert (r.m, r.n, r.k) == (c, k, 16 * tiles) and r.flops == 2.0 * c * k * 16 * tiles and r.ms > 0


@pytest.mark.parametrize('shape', [(2, 11, 9, 16, 24, 5, 5, 1, 'SAME'), (2, 13, 18, 32, 48, 3, 3, 2, 'VALID')], ids=['5x5', 'stride 2'])
def test_descriptors_the_route_does_not_take_run_the_direct_kernels(shape):
    from ann3depth_amd import ops
    n, h, w, c, k = shape[:5]
    rng = np.random.default_rng(32)
    d = ops.conv_desc(*shape)
    x = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)).cuda()
    dz = torch.from_numpy(rng.standard_normal((n, d.ho, d.wo, k)).astype(np.float32)).cuda()
    got = []
    for call in (ops.conv2d_bwd_filter, ops.conv2d_bwd_filter_wino):
        dw, db = torch.empty(shape[5:7] + (c, k), device='cuda'), torch.empty(k, device='cuda')
        call(d, x, dz, dw, db)
        got.append((dw.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


def test_a_workspace_one_byte_short_is_refused_and_dw_untouched():
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    case = CASES[3]
    n, h, w, c, k, padding = case[:6]
    d = ops.conv_desc(n, h, w, c, k, 3, 3, 1, padding)
    x, dz = (torch.from_numpy(a).cuda() for a in operands(case, True))
    dw, db = torch.full((3, 3, c, k), GUARD, device='cuda'), torch.full((k,), GUARD, device='cuda')
    need = lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = lib.a3dwg_conv2d_bwd_filter(ctypes.byref(d), p(x), p(dz), p(dw), p(db), p(ws), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and 'workspace' in _lib.last_error()
    assert bool((dw == GUARD).all()) and bool((db == GUARD).all())
    rc = lib.a3dwg_conv2d_bwd_filter(ctypes.byref(d), p(x), p(dz), p(dw), p(db), p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0                                   # the queried size itself is enough
    xh, dzh = operands(case, True)
    dw_ref, db_ref = T.conv2d_bwd_filter(xh.astype(np.float64), dzh.astype(np.float64), (3, 3, c, k), 1, padding)
    np.testing.assert_array_equal(dw.cpu().numpy(), dw_ref)
    np.testing.assert_array_equal(db.cpu().numpy(), db_ref)


def test_the_coarse_step_with_the_route_against_the_direct_kernels():
    """B = 8: both losses, both maps and every gradient but conv2d_2/3's are the direct step's bits; those two layers' kernel and
    bias gradients differ by rounding alone."""
    from ann3depth_amd import models
    from oracle import msdn as O
    B = 8
    rng = np.random.default_rng(33)
    img = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)).cuda()
    dep = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 1)) / 255).astype(np.float32)).cuda()
    keep = torch.from_numpy(rng.random((B, 4096)) >= 0.5).cuda()
    params = O.init_params(3000)

    class Direct(models.MSDNReplica):
        WINO_GRAD_MIN_TILES = 1 << 30

    nets = [models.MSDNReplica(B, device='cuda:0', params=params), Direct(B, device='cuda:0', params=params)]
    assert nets[0].wino_grad == set(models.MSDNReplica.WINO_GRAD_LAYERS) and not nets[1].wino_grad
    outs = [net.step(img, dep, keep) for net in nets]
    torch.cuda.synchronize()
    bits = lambda t: t.detach().cpu().numpy().view(np.uint32)      # noqa: E731
    for key in ('coarse_loss', 'fine_loss'):
        assert np.float32(float(outs[0][key])).view(np.uint32) == np.float32(float(outs[1][key])).view(np.uint32), key
    for key in ('coarse', 'fine'):
        assert np.array_equal(bits(getattr(nets[0], key)), bits(getattr(nets[1], key))), key
    moved = [layer + suffix for layer in models.MSDNReplica.WINO_GRAD_LAYERS for suffix in ('/kernel', '/bias')]
    for name in nets[0].shapes:
        if not name.startswith('coarse/'):
            continue
        a, b = nets[0].grad(name), nets[1].grad(name)
        if name in moved:
            r = rel_l2(a.cpu().numpy(), b.cpu().numpy())
            print(f'{name}: rel-L2 {r:.3e}')
            assert 0 < r < RTOL_F32, name
        else:
            assert np.array_equal(bits(a), bits(b)), name
