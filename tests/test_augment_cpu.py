"""Train-time augmentation without a GPU: the numpy restatement of a3d_warp_bilinear_pair's contract (tests/augment_ref.py)
against the oracle's resize, flips and slices; the parameter draws of ann3depth_amd/augment.py (fit inside the image,
ranges, reproducibility, a pinned table); the C ABI's argument checks; the driver's --augment flag."""
import ctypes
import os
import re

import numpy as np
import pytest

import augment_ref as R
from ann3depth_amd import augment as A
from oracle import tf13_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'augment_table.npy')
GOLDEN_ARGS = dict(seed=3000, rank=1, step=7, n=4, h=480, w=640)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('oh,ow', [(228, 304), (55, 74), (240, 320), (480, 640)])
def test_identity_table_is_the_oracles_resize_bit_for_bit(oh, ow):
    rng = np.random.default_rng(oh)
    img = rng.random((2, 480, 640, 3), dtype=np.float32)
    dep = rng.random((2, 480, 640, 1), dtype=np.float32)
    np.testing.assert_array_equal(bits(R.warp(img, R.identity(2), oh, ow)), bits(T.resize_bilinear_tf1(img, oh, ow)))
    np.testing.assert_array_equal(bits(R.warp(dep, R.identity(2), oh, ow, second=True)),
                                  bits(T.resize_bilinear_tf1(dep, oh, ow)))


def test_identity_table_upscaling_past_the_last_source_pixel():
    """48 x 64 -> 228 x 304: fl(303 * fl(64 / 304)) = 63.79 > w - 1, where the resize reads pixel 63 twice and the warp
    clamps the coordinate to 63: the same value from finite sources."""
    x = np.random.default_rng(0).random((1, 48, 64, 3), dtype=np.float32)
    np.testing.assert_array_equal(bits(R.warp(x, R.identity(1), 228, 304)), bits(T.resize_bilinear_tf1(x, 228, 304)))


def test_uint8_sources_read_the_loaders_float():
    k = np.random.default_rng(1).integers(0, 256, (2, 12, 16, 3), dtype=np.uint8)
    f = (k.astype(np.float32) / np.float32(255) - np.float32(0.5)) + np.float32(0.5)
    np.testing.assert_array_equal(R.as_float(k), f)
    t = A.table(A.Eigen2014(), 1, 0, 0, 2, 12, 16)
    np.testing.assert_array_equal(bits(R.warp(k, t, 7, 9)), bits(R.warp(f, t, 7, 9)))


def test_flip_and_integer_translations_are_flips_and_slices():
    rng = np.random.default_rng(2)
    h, w = 9, 13
    x = rng.random((3, h, w, 3), dtype=np.float32)
    t = R.identity(3)
    t[:, 0], t[:, 2] = -1, w - 1
    np.testing.assert_array_equal(bits(R.warp(x, t, h, w)), bits(x[:, :, ::-1]))
    np.testing.assert_array_equal(bits(R.warp(x, t, h, w)), bits(np.flip(x, axis=2)))
    t = R.identity(3)
    t[:, 4], t[:, 5] = -1, h - 1                                           # vertical flip
    np.testing.assert_array_equal(bits(R.warp(x, t, h, w)), bits(np.flip(x, axis=1)))
    for dx, dy in [(2, 0), (0, 3), (4, 1)]:
        t = R.identity(3)
        t[:, 2], t[:, 5] = dx, dy
        y = R.warp(x, t, h, w)                                             # past the edge the clamp repeats the last pixel
        np.testing.assert_array_equal(bits(y[:, :h - dy, :w - dx]), bits(x[:, dy:, dx:]))
        np.testing.assert_array_equal(bits(y[:, :, w - dx:]), bits(np.repeat(y[:, :, w - dx - 1:w - dx], dx, axis=2)))
    g = R.identity(3)
    g[:, 6:9] = [0.5, 2.0, 0.25]
    g[:, 10] = 0.125
    np.testing.assert_array_equal(R.warp(x, g, h, w), x * np.array([0.5, 2.0, 0.25], np.float32))
    np.testing.assert_array_equal(R.warp(x[..., :1], g, h, w, second=True), x[..., :1] * np.float32(0.125))


def test_wild_coefficients_are_decided_by_the_clamp():
    x = np.random.default_rng(3).random((4, 7, 5, 1), dtype=np.float32)
    t = R.identity(4)
    t[0, 2], t[0, 5] = 1e30, -1e30                                         # far right, far above: pixel (0, w - 1)
    t[1, 0] = np.nan                                                       # NaN coordinate lands on column 0
    t[2, 2] = np.inf
    y = R.warp(x, t, 7, 5, second=True)
    np.testing.assert_array_equal(y[0], np.broadcast_to(x[0, 0, 4], (7, 5, 1)))
    np.testing.assert_array_equal(y[1], np.broadcast_to(x[1, :, :1], (7, 5, 1)))
    np.testing.assert_array_equal(y[2], np.broadcast_to(x[2, :, 4:], (7, 5, 1)))
    np.testing.assert_array_equal(y[3], x[3])


# ---------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize('h,w', [(480, 640), (48, 64)])
def test_sampled_windows_stay_inside_the_image(h, w):
    """4096 draws: the corners of the window, recomputed in float64 from (r, s, t), and the same corners through the
    float32 table, lie within 1e-3 pixel of the image (the float32 rounding slack of a coordinate below 640)."""
    cfg = A.Eigen2014()
    for step in range(4):
        p = A.draw(cfg, 11, 0, step, 1024, h, w)
        c = R.window_corners(p, h, w)
        print(f'{h}x{w} step {step}: x in [{c[..., 0].min():.6f}, {c[..., 0].max():.6f}], '
              f'y in [{c[..., 1].min():.6f}, {c[..., 1].max():.6f}]')
        assert c[..., 0].min() >= -1e-3 and c[..., 0].max() <= w - 1 + 1e-3
        assert c[..., 1].min() >= -1e-3 and c[..., 1].max() <= h - 1 + 1e-3
        t = A.assemble(p, h, w).astype(np.float64)
        for px, py in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]:
            X = t[:, 0] * px + t[:, 1] * py + t[:, 2]
            Y = t[:, 3] * px + t[:, 4] * py + t[:, 5]
            assert X.min() >= -1e-3 and X.max() <= w - 1 + 1e-3 and Y.min() >= -1e-3 and Y.max() <= h - 1 + 1e-3


def test_every_draw_is_inside_its_range():
    cfg = A.Eigen2014()
    h, w = 480, 640
    p = A.draw(cfg, 5, 2, 9, 4096, h, w)
    assert np.abs(p['r']).max() <= np.deg2rad(5.0) and np.abs(p['r']).max() > np.deg2rad(4.9)
    fit = A.s_fit(p['r'], h, w)
    assert (p['s'] >= np.maximum(1.0, fit)).all() and (p['s'] <= 1.5).all()
    assert A.s_fit(np.deg2rad(5.0), h, w) == pytest.approx(1.1125, abs=1e-3) and A.s_fit(0.0, h, w) == 1.0
    assert (p['gains'] >= 0.8).all() and (p['gains'] <= 1.2).all() and p['gains'].std() > 0.1
    assert set(np.unique(p['flip'])) == {-1.0, 1.0} and 0.45 < (p['flip'] < 0).mean() < 0.55
    assert np.abs(p['tx']).max() > 1 and np.abs(p['ty']).max() > 1
    t = A.assemble(p, h, w)
    assert t.dtype == np.float32 and t.shape == (4096, A.STRIDE)
    # gd * s = 1 to float32 rounding: gd = fl(1 / s), relative error 2^-24
    np.testing.assert_allclose(t[:, 10].astype(np.float64) * p['s'], 1.0, rtol=0, atol=2.0 ** -24)
    np.testing.assert_array_equal(t[:, 9], 1)
    np.testing.assert_array_equal(t[:, 11], 0)
    np.testing.assert_array_equal(t[:, 6:9], p['gains'].astype(np.float32))
    # the rotation part is a scaled rotation, mirrored where flipped
    np.testing.assert_allclose(t[:, 0].astype(np.float64) * t[:, 4] - t[:, 1].astype(np.float64) * t[:, 3],
                               p['flip'] / p['s'] ** 2, rtol=1e-6)


def test_table_is_a_pure_function_of_seed_rank_step():
    cfg = A.Eigen2014()
    base = A.table(cfg, 3000, 0, 5, 32, 480, 640)
    np.testing.assert_array_equal(base, A.table(cfg, 3000, 0, 5, 32, 480, 640))
    A.table(cfg, 1, 1, 1, 32, 480, 640)                                    # another draw in between: no state is kept
    np.testing.assert_array_equal(base, A.table(cfg, 3000, 0, 5, 32, 480, 640))
    for other in (A.table(cfg, 3001, 0, 5, 32, 480, 640), A.table(cfg, 3000, 1, 5, 32, 480, 640),
                  A.table(cfg, 3000, 0, 6, 32, 480, 640)):
        assert not np.isin(other[:, :9], base[:, :9]).any()                # not even a shifted copy of the stream
    out = np.full((32, 12), 7, np.float32)
    assert A.table(cfg, 3000, 0, 5, 32, 480, 640, out=out) is out
    np.testing.assert_array_equal(out, base)
    with pytest.raises(ValueError):
        A.table(cfg, 3000, 0, -1, 32, 480, 640)


def test_degenerate_ranges_give_exactly_the_identity_table():
    off = A.Eigen2014(scale=(1.0, 1.0), rotate_deg=0.0, color=(1.0, 1.0), flip=0.0, translate=True)
    for h, w in [(480, 640), (48, 64), (7, 5)]:
        t = A.table(off, 3, 1, 4, 16, h, w)
        np.testing.assert_array_equal(bits(t), bits(R.identity(16)))       # bits: no negative zero either
        np.testing.assert_array_equal(bits(t), bits(A.identity(16)))
    # one transformation on, the others off: only its columns move
    t = A.table(A.Eigen2014(scale=(1.0, 1.0), rotate_deg=0.0, flip=0.0), 3, 1, 4, 16, 480, 640)
    np.testing.assert_array_equal(t[:, :6], R.identity(16)[:, :6])
    assert (t[:, 6:9] != 1).all()
    t = A.table(A.Eigen2014(scale=(1.0, 1.0), rotate_deg=0.0, color=(1.0, 1.0), flip=1.0), 3, 1, 4, 16, 480, 640)
    np.testing.assert_array_equal(t[:, :6], np.tile(np.float32([-1, 0, 639, 0, 1, 0]), (16, 1)))


def test_golden_table():
    """This build's own output, pinned against drift of the generator and of the draw order."""
    want = np.load(GOLDEN)
    assert want.dtype == np.float32 and want.shape == (4, 12)
    np.testing.assert_array_equal(bits(A.table(A.Eigen2014(), **GOLDEN_ARGS)), bits(want))


# ---------------------------------------------------------------------------------------------- C ABI
def test_warp_is_declared_bound_and_documented():
    from ann3depth_amd import _lib, ops
    assert 'a3d_warp_bilinear_pair' in _lib.SIGNATURES and callable(ops.warp_bilinear_pair)
    header = open(os.path.join(ROOT, 'include', 'a3d.h')).read()
    assert re.search(r'#define A3D_WARP_STRIDE 12\b', header) and ops.WARP_STRIDE == A.STRIDE == R.STRIDE == 12
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*#define A3D_WARP_STRIDE 12\s*int a3d_warp_bilinear_pair\(', header, flags=re.S)
    assert m and 'fmaxf' in m.group(1) and 'A3D_EINVAL' in m.group(1)
    assert len(_lib.SIGNATURES) == 77


def test_warp_rejects_bad_arguments_before_any_launch(lib):
    """A3D_EINVAL comes before any device work: these calls pass host pointers that a launch would fault on."""
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def call(n=2, h=4, w=4, c0=3, x0=p, u8_0=1, oh0=2, ow0=2, y0=p, c1=1, x1=p, u8_1=1, oh1=2, ow1=2, y1=p, table=p):
        return lib.a3d_warp_bilinear_pair(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1, table, None)
    for kw in ({'c0': 5}, {'c0': 0}, {'table': None}, {'n': 0}, {'h': 0}, {'w': 0}, {'oh0': 0}, {'ow0': 0}, {'x0': None},
               {'y0': None}, {'c1': 0}, {'oh1': 0}, {'ow1': 0}, {'y1': None}, {'n': -3}, {'h': 1 << 16, 'w': 1 << 16}):
        assert call(**kw) == -1, kw
        from ann3depth_amd import _lib
        assert 'warp_pair' in _lib.last_error(), kw
    assert bytes(buf.raw) == bytes(1 << 12)                                # nothing was written


def test_op_checks_its_arguments_on_the_host():
    import torch

    from ann3depth_amd import ops
    x = torch.zeros((2, 4, 4, 3))
    y = torch.zeros((2, 2, 2, 3))
    t = torch.zeros((2, 12))
    for bad in (dict(table=torch.zeros((2, 11))), dict(table=torch.zeros((3, 12))), dict(table=t.double()),
                dict(y0=torch.zeros((2, 2, 2, 1))), dict(x1=torch.zeros((2, 4, 5, 1)), y1=torch.zeros((2, 2, 2, 1))),
                dict(x1=torch.zeros((2, 4, 4, 1))), dict()):                # the last: right shapes, but not on a GPU
        kw = dict(x0=x, y0=y, x1=None, y1=None, table=t)
        kw.update(bad)
        with pytest.raises(ValueError, match='warp_bilinear_pair'):
            ops.warp_bilinear_pair(**kw)


# ---------------------------------------------------------------------------------------------- CLI
def test_cli_flag_and_the_dcnf_refusal(capsys):
    from ann3depth_amd import ann3depth, models
    assert ann3depth.parse_args(['nyu']).augment == 'none'
    assert ann3depth.parse_args(['--augment', 'eigen', 'nyu']).augment == 'eigen'
    with pytest.raises(SystemExit):
        ann3depth.parse_args(['--augment', 'sometimes', 'nyu'])
    assert models.msdn.augment is None
    assert ann3depth.main(['--augment', 'eigen', '--model', 'dcnf', 'nyu']) == 2          # before anything touches a GPU
    out = capsys.readouterr()
    assert 'msdn only' in out.out + out.err
    assert models.msdn.augment is None and not hasattr(models.dcnf, 'augment')


def test_make_train_passes_train_args():
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert re.search(r'^TRAIN_ARGS \?=\s*$', mk, flags=re.M)
    assert re.search(r'^train:.*\n\t\$\{SCRIPT\} \$\{SCRIPT_PARAMETERS\} \$\{TRAIN_ARGS\} \$\{DATASET\}$', mk, flags=re.M)
