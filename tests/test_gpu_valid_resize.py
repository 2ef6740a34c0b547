"""a3dx_resize_bilinear_tf1_valid and a3dx_warp_bilinear_pair_valid on the GPU, held to tests/valid_ref.py over every element
of the depth map (NaN where the reference has NaN, the reference's bits elsewhere); the image of the same launch must keep
the bits of the plain entry point.  Outputs are windows of sentinel-filled allocations whose guards must keep their bits."""
import numpy as np
import pytest
import torch

import augment_ref as R
import valid_ref as V
from ann3depth_amd import augment as A

pytestmark = pytest.mark.gpu

SENT = 7.0
INF = float('inf')
SIZES = [(7, 5, 3, 4, 3, 4), (48, 64, 228, 304, 55, 74), (480, 640, 228, 304, 55, 74)]   # h, w, oh0, ow0, oh1, ow1
RANGES = [(0.0, INF), (0.0, 0.99), (-1.0, INF)]           # the last admits everything


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Guarded:
    """A float32 tensor inside a larger allocation filled with a sentinel (512 elements before and after)."""

    def __init__(self, *shape, guard=512):
        n = int(np.prod(shape))
        self.big = torch.full((n + 2 * guard,), SENT, device='cuda')
        self.t = self.big[guard:guard + n].view(*shape)
        self.guard = guard

    def host(self):
        a = self.big.cpu().numpy()
        g = self.guard
        assert (a[:g] == SENT).all() and (a[-g:] == SENT).all(), 'the kernel wrote outside its tensor'
        return a[g:-g].reshape(tuple(self.t.shape))


def punch(rng, n, h, w):
    """Boolean [n, h, w]: rectangular blobs covering 5-30 % of each image, plus single pixels on the last row and the last
    column, where the clamp x1 = min(x0 + 1, w - 1) bites."""
    hole = np.zeros((n, h, w), bool)
    for b in range(n):
        want = rng.uniform(0.05, 0.30) * h * w
        while hole[b].sum() < want:
            bh, bw = rng.integers(1, max(2, h // 3) + 1), rng.integers(1, max(2, w // 3) + 1)
            y, x = rng.integers(0, h - bh + 1), rng.integers(0, w - bw + 1)
            hole[b, y:y + bh, x:x + bw] = True
            if hole[b].sum() > 0.30 * h * w:
                hole[b, y:y + bh, x:x + bw] = False
                hole[b, y, x] = True
        hole[b, h - 1, rng.integers(0, w)] = True
        hole[b, rng.integers(0, h), w - 1] = True
        hole[b, h - 1, w - 1] = bool(b % 2)
    return hole


def sources(rng, n, h, w, kind):
    """A uint8 image and a depth map with holes (stored 0) and the range cap (k = 255, stored 1.0) present: uint8, or the
    float32 of the same records scaled so that some depths lie above 0.99."""
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dep = rng.integers(1, 256, (n, h, w, 1), dtype=np.uint8)
    dep[rng.random((n, h, w, 1)) < 0.02] = 255
    dep[punch(rng, n, h, w)[..., None]] = 0
    dep[:, 0, 0, 0] = 255                       # the cap on a pixel every resize reads as a counting tap
    if kind == 'f32':
        dep = R.as_float(dep) * np.float32(1.25)
    return img, dep


def tables(n, h, w, seed):
    flip = R.identity(n)
    flip[:, 0], flip[:, 2] = -1, w - 1
    return {'identity': R.identity(n), 'flip': flip, 'eigen': A.table(A.Eigen2014(), seed, 0, 3, n, h, w)}


def same_where_valid(got, want):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[keep], bits(want)[keep])


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w,oh0,ow0,oh1,ow1', SIZES)
def test_valid_resize_is_the_reference(ops, h, w, oh0, ow0, oh1, ow1, n, kind):
    rng = np.random.default_rng(h + n)
    img, dep = sources(rng, n, h, w, kind)
    z0, z1 = Guarded(n, oh0, ow0, 3), Guarded(n, oh1, ow1, 1)
    ops.resize_bilinear_tf1_pair(dev(img), z0.t, dev(dep), z1.t)
    plain0, plain1 = z0.host(), z1.host()
    seen = []
    for lo, hi in RANGES:
        y0, y1 = Guarded(n, oh0, ow0, 3), Guarded(n, oh1, ow1, 1)
        ops.resize_bilinear_tf1_pair_valid(dev(img), y0.t, dev(dep), y1.t, lo, hi)
        got0, got1 = y0.host(), y1.host()
        want = V.resize_valid(dep, R.identity(n), oh1, ow1, lo, hi)
        same_where_valid(got1, want)
        np.testing.assert_array_equal(bits(got0), bits(plain0))              # the image: the plain launch's bits
        seen.append(int(np.isnan(want).sum()))
    assert seen[2] == 0 and 0 < seen[0] < seen[1] < want.size                # holes, then holes and the cap, then nothing
    np.testing.assert_array_equal(bits(got1), bits(plain1))                  # (-1, inf): the plain depth map


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w,oh0,ow0,oh1,ow1', SIZES)
def test_valid_warp_is_the_reference(ops, h, w, oh0, ow0, oh1, ow1, n, kind):
    rng = np.random.default_rng(h * 3 + n)
    img, dep = sources(rng, n, h, w, kind)
    for name, table in tables(n, h, w, seed=h + n).items():
        z0, z1 = Guarded(n, oh0, ow0, 3), Guarded(n, oh1, ow1, 1)
        ops.warp_bilinear_pair(dev(img), z0.t, dev(dep), z1.t, dev(table))
        plain0, plain1 = z0.host(), z1.host()
        for lo, hi in RANGES:
            y0, y1 = Guarded(n, oh0, ow0, 3), Guarded(n, oh1, ow1, 1)
            ops.warp_bilinear_pair_valid(dev(img), y0.t, dev(dep), y1.t, dev(table), lo, hi)
            got0, got1 = y0.host(), y1.host()
            want = V.resize_valid(dep, table, oh1, ow1, lo, hi)
            same_where_valid(got1, want)
            np.testing.assert_array_equal(bits(got0), bits(plain0))
            assert np.isnan(want).any() == (lo == 0.0), (name, lo, hi)
        np.testing.assert_array_equal(bits(got1), bits(plain1))


def test_identity_table_gives_the_valid_resize(ops):
    rng = np.random.default_rng(11)
    img, dep = sources(rng, 3, 48, 64, 'u8')
    a0, a1, b0, b1 = Guarded(3, 228, 304, 3), Guarded(3, 55, 74, 1), Guarded(3, 228, 304, 3), Guarded(3, 55, 74, 1)
    ops.resize_bilinear_tf1_pair_valid(dev(img), a0.t, dev(dep), a1.t, 0, 0.99)
    ops.warp_bilinear_pair_valid(dev(img), b0.t, dev(dep), b1.t, dev(R.identity(3)), 0, 0.99)
    np.testing.assert_array_equal(bits(a0.host()), bits(b0.host()))
    same_where_valid(b1.host(), a1.host())


def test_taps_that_are_not_finite(ops):
    """A NaN and an infinite depth in a float32 map: every element with one of them among its four taps is NaN, counting
    or not (the plain arithmetic gives NaN there too); with thresholds that admit every number nothing else is."""
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    dep = (rng.random((2, 48, 64, 1), dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    dep[0, 10, 20, 0], dep[0, 47, 63, 0], dep[1, 30, 5, 0], dep[1, 0, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    for table in (None, A.table(A.Eigen2014(), 5, 0, 0, 2, 48, 64)):
        for oh, ow in ((55, 74), (24, 32)):                                  # 24 x 32: lx = ly = 0 everywhere for the resize
            for lo, hi in ((-INF, INF), (0.0, INF)):
                y0, y1 = Guarded(2, 228, 304, 3), Guarded(2, oh, ow, 1)
                if table is None:
                    ops.resize_bilinear_tf1_pair_valid(dev(img), y0.t, dev(dep), y1.t, lo, hi)
                else:
                    ops.warp_bilinear_pair_valid(dev(img), y0.t, dev(dep), y1.t, dev(table), lo, hi)
                want = V.resize_valid(dep, R.identity(2) if table is None else table, oh, ow, lo, hi)
                got = y1.host()
                same_where_valid(got, want)
                assert 0 < np.isnan(got).sum() < 200 and not np.isinf(got).any()


def test_depth_map_alone_at_its_own_stored_size(ops):
    """ops.resize_bilinear_tf1_valid: the form the step uses when the depth maps are stored smaller than the images."""
    rng = np.random.default_rng(13)
    _, dep = sources(rng, 3, 24, 32, 'u8')
    y = Guarded(3, 55, 74, 1)
    ops.resize_bilinear_tf1_valid(dev(dep), y.t, 0, 0.99)
    same_where_valid(y.host(), V.resize_valid(dep, R.identity(3), 55, 74, 0, 0.99))


def test_bad_arguments_are_refused_before_any_launch(ops):
    from ann3depth_amd import _lib
    lib = _lib.load()
    x0, x1 = torch.zeros((2, 48, 64, 3), device='cuda'), torch.ones((2, 48, 64, 1), device='cuda')
    y0, y1 = Guarded(2, 228, 304, 3), Guarded(2, 55, 74, 1)
    table = dev(R.identity(2))
    nan = float('nan')

    def resize(x1p, y1p, lo, hi):
        return lib.a3dx_resize_bilinear_tf1_valid(2, 48, 64, 3, x0.data_ptr(), 0, 228, 304, y0.t.data_ptr(), 1, x1p, 0, 55, 74,
                                                 y1p, lo, hi, None)

    def warp(x1p, y1p, lo, hi, tab=table.data_ptr()):
        return lib.a3dx_warp_bilinear_pair_valid(2, 48, 64, 3, x0.data_ptr(), 0, 228, 304, y0.t.data_ptr(), 1, x1p, 0, 55, 74,
                                                y1p, tab, lo, hi, None)
    for fn in (resize, warp):
        assert fn(None, y1.t.data_ptr(), 0.0, 1.0) == -1 and 'depth map' in _lib.last_error()
        assert fn(x1.data_ptr(), None, 0.0, 1.0) == -1
        assert fn(x1.data_ptr(), y1.t.data_ptr(), nan, 1.0) == -1 and 'thresholds' in _lib.last_error()
        assert fn(x1.data_ptr(), y1.t.data_ptr(), 0.0, nan) == -1
        assert fn(x1.data_ptr(), y1.t.data_ptr(), 1.0, 0.5) == -1 and 'thresholds' in _lib.last_error()
    assert warp(x1.data_ptr(), y1.t.data_ptr(), 0.0, 1.0, tab=None) == -1 and 'table' in _lib.last_error()
    with pytest.raises(ValueError, match='depth map'):
        ops.resize_bilinear_tf1_pair_valid(x0, y0.t, None, None, 0, 1)
    with pytest.raises(ValueError, match='min_depth'):
        ops.warp_bilinear_pair_valid(x0, y0.t, x1, y1.t, table, 1, 0)
    with pytest.raises(ValueError, match='min_depth'):
        ops.resize_bilinear_tf1_pair_valid(x0, y0.t, x1, y1.t, nan, 1)
    with pytest.raises(ValueError, match='second tensor'):
        ops.warp_bilinear_pair_valid(x0, y0.t, torch.zeros((2, 6, 8, 1), device='cuda'), y1.t, table)
    with pytest.raises(ValueError, match='no table'):
        ops.warp_bilinear_pair_valid(x0, y0.t, x1, y1.t, None)
    torch.cuda.synchronize()
    assert (y0.host() == SENT).all() and (y1.host() == SENT).all()
    assert resize(x1.data_ptr(), y1.t.data_ptr(), 0.5, 0.5) == 0             # min == max is a legal (empty) range
    torch.cuda.synchronize()
    assert np.isnan(y1.host()).all() and (y0.host() == 0).all()
