"""Joint bilateral upsampling without a GPU: the references of tests/upsample_ref.py against each other, the host tables
of ops.UpsampleMap, the property the feature exists for (a depth edge that follows the image's edge, where the legacy
bilinear resize smears it), and every refusal of ops and of the two drivers that comes before any GPU work."""
import numpy as np
import pytest
import torch

import upsample_ref as U
from oracle import tf13_ops as T

K = 25                                      # cells of an R = 2 window


def random_case(seed, n, gh, gw, H, W, u8=False):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 8, (n, gh, gw)).astype(np.float32)
    guide = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8) if u8 else rng.random((n, H, W, 3)).astype(np.float32)
    return depth, guide


def step_edge_case():
    """Guide 12 x 16, columns < 8 black and the rest white; depth 3 x 4, columns < 2 at 1.5 and the rest at 3.25."""
    guide = np.zeros((1, 12, 16, 3), np.float32)
    guide[:, :, 8:] = 1
    depth = np.full((1, 3, 4), 3.25, np.float32)
    depth[:, :, :2] = 1.5
    side = np.where(np.arange(16) < 8, np.float32(1.5), np.float32(3.25))[None, None, :].repeat(12, 1)
    return depth, guide, side


def test_reference_is_the_literal_quotient_at_moderate_sigmas():
    """sigma_s = 1, sigma_r = 0.5: the largest exponent is 2 * 2.5^2 / 2 + 3 / 0.5 < 13, nothing underflows."""
    depth, guide = random_case(1, 2, 5, 7, 9, 11)
    tabs = U.tables_corner(5, 7, 9, 11)
    ss, sr = U.inv2(1.0), U.inv2(0.5)
    want = U.literal(depth, guide, *tabs, 2, ss, sr)
    got = U.upsample(depth, guide, *tabs, 2, ss, sr)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(U.upsample(depth, guide, *tabs, 2, ss, sr, shifted=False), want, rtol=1e-12, atol=0)
    # the uint8 guide is the float32 guide fl(k / 255)
    depth, k = random_case(2, 1, 3, 4, 7, 9, u8=True)
    tabs = U.tables_corner(3, 4, 7, 9)
    a = U.upsample(depth, k, *tabs, 1, ss, sr)
    b = U.upsample(depth, k.astype(np.float32) / np.float32(255), *tabs, 1, ss, sr)
    assert np.array_equal(a, b)
    np.testing.assert_allclose(a, U.literal(depth, k, *tabs, 1, ss, sr), rtol=1e-12, atol=0)


def test_pinned_tables():
    from ann3depth_amd import ops
    # block, H = 240 (sp = 40): the 240 grid itself
    m = ops.UpsampleMap(6, 8, 240, 320, 'block', 40, device='cpu')
    assert m.cy.dtype == m.cx.dtype == torch.float32 and m.ay.dtype == m.ax.dtype == torch.int32
    assert (m.cy.shape, m.cx.shape, m.ay.shape, m.ax.shape) == ((240,), (320,), (6,), (8,))
    assert m.cy[0].item() == np.float32(-0.4875) and m.cy[239].item() == np.float32(5.4875)
    assert m.cx[0].item() == np.float32(-0.4875) and m.cx[319].item() == np.float32(7.4875)
    assert m.ay.tolist() == [20, 60, 100, 140, 180, 220]
    assert m.ax.tolist() == [20 + 40 * c for c in range(8)]
    # block, H = 480
    m = ops.UpsampleMap(6, 8, 480, 640, 'block', 40, device='cpu')
    assert m.ay.tolist() == [40, 120, 200, 280, 360, 440]
    assert m.ax.tolist() == [40 + 80 * c for c in range(8)]
    assert m.cy[0].item() == np.float32(-0.4875) and m.cy[479].item() == np.float32(5.5)
    # corner: cell i at relative position i / gh
    m = ops.UpsampleMap(3, 4, 12, 16, 'corner', device='cpu')
    assert m.cy.tolist() == [y * 0.25 for y in range(12)] and m.cx.tolist() == [x * 0.25 for x in range(16)]
    assert m.ay.tolist() == [0, 4, 8] and m.ax.tolist() == [0, 4, 8, 12]
    m = ops.UpsampleMap(55, 74, 480, 640, 'corner', device='cpu')
    assert m.cy[479].item() == np.float32(479 * 55 / 480) and m.ay[54].item() == 471 and m.ax[73].item() == 631
    # ops builds what the reference's scalar loops build, at every size the tests use
    for gh, gw, H, W in ((3, 4, 7, 9), (3, 4, 12, 16), (5, 7, 37, 130), (55, 74, 480, 640), (7, 5, 3, 2)):
        m = ops.UpsampleMap(gh, gw, H, W, 'corner', device='cpu')
        for got, want in zip((m.cy, m.cx, m.ay, m.ax), U.tables_corner(gh, gw, H, W)):
            assert got.numpy().dtype == want.dtype and np.array_equal(got.numpy(), want)
    for sp, H, W in ((40, 48, 64), (20, 37, 130), (10, 240, 320), (10, 480, 640), (40, 7, 9)):
        m = ops.UpsampleMap(240 // sp, 320 // sp, H, W, 'block', sp, device='cpu')
        for got, want in zip((m.cy, m.cx, m.ay, m.ax), U.tables_block(sp, H, W)):
            assert got.numpy().dtype == want.dtype and np.array_equal(got.numpy(), want)
        assert 0 <= m.ay.min() and m.ay.max() < H and 0 <= m.ax.min() and m.ax.max() < W


def test_shift_invariance():
    """w = exp(-(e - e_min)): a constant added to every exponent changes nothing beyond rounding."""
    depth, guide = random_case(3, 2, 5, 7, 12, 17)
    tabs = U.tables_block(40, 12, 17)
    depth6 = np.random.default_rng(4).uniform(0.5, 8, (2, 6, 8)).astype(np.float32)
    for d, t in ((depth, U.tables_corner(5, 7, 12, 17)), (depth6, tabs)):
        base = U.upsample(d, guide, *t, 2, U.inv2(1.0), U.inv2(0.1))
        for c in (3.0, 100.0, -50.0):
            np.testing.assert_allclose(U.upsample(d, guide, *t, 2, U.inv2(1.0), U.inv2(0.1), e_add=c), base, rtol=1e-12, atol=0)
    # where the literal form has already lost the pixel (every weight underflows), the shifted one has not
    sharp = U.upsample(depth, guide, *U.tables_corner(5, 7, 12, 17), 2, U.inv2(1.0), U.inv2(0.1), e_add=800.0, shifted=False)
    assert np.isnan(sharp).all()


def test_a_step_edge_keeps_its_side():
    depth, guide, side = step_edge_case()
    tabs = U.tables_corner(3, 4, 12, 16)
    assert tabs[3].tolist() == [0, 4, 8, 12]                            # cells 0, 1 take a black colour, 2, 3 a white one
    bound = (2 * K + 2) * 2.0 ** -24 * np.abs(side.astype(np.float64))
    for dtype in (np.float64, np.float32):
        out = U.upsample(depth, guide, *tabs, 2, U.inv2(1.0), U.inv2(0.05), dtype=dtype)
        err = np.abs(out.astype(np.float64) - side)
        print(f'step edge, {np.dtype(dtype).name}: max error {err.max():.3g} ({(err / (2.0 ** -23 * side)).max():.2f} ulp)')
        assert (err <= bound).all()
    # in float32 the wrong side's weights are exp(-600) = 0 exactly
    assert np.exp(-np.float32(3) * U.inv2(0.05)) == 0
    # the legacy bilinear resize of the same grid smears the edge: the property the feature exists for
    smeared = T.resize_bilinear_tf1(depth[..., None], 12, 16)[..., 0]
    assert np.abs(smeared.astype(np.float64) - side).max() > 0.1


def test_skips_and_nan_pixels_in_the_reference():
    depth, guide = random_case(5, 1, 3, 4, 7, 9)
    cy, cx, ay, ax = U.tables_corner(3, 4, 7, 9)
    d = depth.copy()
    d[0, 0, 0], d[0, 1, 1], d[0, 2, 3] = np.nan, np.inf, -np.inf
    for dtype in (np.float64, np.float32):
        out = U.upsample(d, guide, cy, cx, ay, ax, 1, U.inv2(1.0), U.inv2(0.1), dtype=dtype)
        assert np.isfinite(out).all()                                   # every window still holds a finite cell
        none = U.upsample(np.full_like(d, np.nan), guide, cy, cx, ay, ax, 4, U.inv2(1.0), U.inv2(0.1), dtype=dtype)
        assert np.isnan(none).all()
        bad = cy.copy()
        bad[2] = np.nan
        out = U.upsample(depth, guide, bad, cx, ay, ax, 2, U.inv2(1.0), U.inv2(0.1), dtype=dtype)
        assert np.isnan(out[0, 2]).all() and np.isfinite(np.delete(out, 2, axis=1)).all()
        one = np.full_like(d, np.nan)
        one[0, 1, 2] = 2.75
        out = U.upsample(one, guide, cy, cx, ay, ax, 4, U.inv2(1.0), U.inv2(0.1), dtype=dtype)
        assert (out == 2.75).all()                                      # R = 4 covers the 3 x 4 grid from anywhere


def test_ops_refusals_that_need_no_gpu():
    from ann3depth_amd import ops
    for args in ((0, 4, 7, 9, 'corner'), (3, 4, 0, 9, 'corner'), (3, -1, 7, 9, 'corner'), (3, 4, 7, 9, 'middle'),
                 (3, 4, 7, 9, 'corner', 40), (6, 8, 48, 64, 'block'), (6, 8, 48, 64, 'block', 20), (12, 16, 48, 64, 'block', 40),
                 (6, 8, 48, 64, 'block', 0), (34, 45, 48, 64, 'block', 7)):
        with pytest.raises(ValueError):
            ops.UpsampleMap(*args, device='cpu')
    m = ops.UpsampleMap(3, 4, 7, 9, 'corner', device='cpu')
    depth, guide = torch.zeros((2, 3, 4)), torch.zeros((2, 7, 9, 3))
    for kw in ({'radius': 0}, {'radius': 5}, {'radius': 1.5}, {'sigma_space': 0.0}, {'sigma_space': -1.0},
               {'sigma_space': float('nan')}, {'sigma_range': 0.0}, {'sigma_range': float('nan')}, {'sigma_range': 1e-30},
               {'sigma_space': 1e-25}):
        with pytest.raises(ValueError, match='joint_bilateral_upsample'):
            ops.joint_bilateral_upsample(depth, guide, m, **kw)
    assert ops.upsample_params(2, 1.0, float('inf')) == (2, 0.5, 0.0)
    assert ops.upsample_params(4, float('inf'), 0.1)[1] == 0.0
    for d, g, o in ((torch.zeros((2, 3, 5)), guide, None), (depth, torch.zeros((2, 7, 9, 1)), None),
                    (depth, torch.zeros((1, 7, 9, 3)), None), (depth, torch.zeros((2, 7, 8, 3)), None),
                    (torch.zeros((2, 3, 4, 1)), guide, None), (depth, guide, torch.zeros((2, 7, 8))),
                    (torch.zeros((0, 3, 4)), torch.zeros((0, 7, 9, 3)), None),
                    (torch.zeros((2, 4, 3)).transpose(1, 2), guide, None)):
        with pytest.raises(ValueError):
            ops.joint_bilateral_upsample(d, g, m, out=o)
    for d, g, o in ((depth.double(), guide, None), (depth, guide.half(), None), (depth, guide.to(torch.int8), None),
                    (depth, guide, torch.zeros((2, 7, 9), dtype=torch.float64))):
        with pytest.raises(TypeError):
            ops.joint_bilateral_upsample(d, g, m, out=o)
    with pytest.raises(TypeError):
        ops.joint_bilateral_upsample(depth, guide, (m.cy, m.cx, m.ay, m.ax))
    with pytest.raises(ValueError, match='one GPU'):                    # host tensors never reach the launch
        ops.joint_bilateral_upsample(depth, guide, m)
    with pytest.raises(ValueError):
        ops.JointUpsampler('corner', radius=7)


def test_predict_parse_args_and_refusals(tmp_path, capsys, monkeypatch):
    from ann3depth_amd import predict
    a = predict.parse_args(['--out', 'o', 'a.png', 'b.png'])
    assert (a.model, a.upsample, a.radius, a.sigma_space, a.sigma_range, a.batchsize, a.superpixel) == \
        ('msdn', 'joint', 2, 1.0, 0.1, 32, 40)
    assert a.images == ['a.png', 'b.png'] and a.out == 'o' and a.checkpoint == '' and a.precision == 'fp32'
    a = predict.parse_args(['--model', 'dcnf', '--superpixel', '10', '--upsample', 'bilinear', '--radius', '4', '--sigma-space',
                            '2', '--sigma-range', 'inf', '-b', '3', '--checkpoint', 'c.pt', '--out', 'o', 'x.png'])
    assert (a.model, a.superpixel, a.upsample, a.radius, a.sigma_space, a.sigma_range, a.batchsize, a.checkpoint) == \
        ('dcnf', 10, 'bilinear', 4, 2.0, float('inf'), 3, 'c.pt')
    assert predict.parse_args(['--upsample', 'none', '--out', 'o']).images == []
    for bad in (['--upsample', 'cubic', '--out', 'o'], ['a.png'], ['--superpixel', '30', '--out', 'o']):
        with pytest.raises(SystemExit):
            predict.parse_args(bad)
    capsys.readouterr()
    from ann3depth_amd import png
    img = str(tmp_path / 'a.png')
    png.imsave(img, np.zeros((4, 5, 3), np.uint8))
    out, ck = str(tmp_path / 'out'), str(tmp_path / 'ckpt')
    base = ['--ckptdir', ck, '--out', out]
    assert predict.main(base + ['--model', 'msdn', img]) == 2
    assert 'no checkpoint' in capsys.readouterr().err
    assert predict.main(base + ['--model', 'resnet', img]) == 2
    assert 'unknown model' in capsys.readouterr().err
    open(tmp_path / 'w.pt', 'wb').close()                               # a file is there; it is not read before the images
    assert predict.main(base + ['--checkpoint', str(tmp_path / 'w.pt')]) == 2
    assert 'no images' in capsys.readouterr().err
    junk = str(tmp_path / 'junk.png')
    with open(junk, 'wb') as f:
        f.write(b'not a png')
    assert predict.main(base + ['--checkpoint', str(tmp_path / 'w.pt'), img, junk]) == 2
    assert 'cannot read' in capsys.readouterr().err
    assert predict.main(base + ['--checkpoint', str(tmp_path / 'w.pt'), '--radius', '9', img]) == 2
    assert 'radius' in capsys.readouterr().err
    assert predict.main(base + ['--superpixel', '20', '--checkpoint', str(tmp_path / 'w.pt'), img]) == 2
    assert 'no superpixels' in capsys.readouterr().err
    monkeypatch.setenv('WORLD_SIZE', '2')
    assert predict.main(base + ['--checkpoint', str(tmp_path / 'w.pt'), img]) == 2
    assert 'one process' in capsys.readouterr().err
    assert not (tmp_path / 'out').exists()


def test_predict_refuses_a_patch_checkpoint_on_a_fine_grid_before_any_gpu_work(tmp_path, capsys):
    """check_dcnf_superpixel's refusal needs the checkpoint's own form: it is read on the host."""
    from ann3depth_amd import png, predict
    from oracle import dcnf as OD
    sd = {k: torch.from_numpy(v) for k, v in {**OD.init_params(3000), **OD.pairwise_init()}.items()}
    sd['global_step'] = torch.tensor(3, dtype=torch.int64)
    torch.save(sd, str(tmp_path / 'patch.pt'))
    img = str(tmp_path / 'a.png')
    png.imsave(img, np.zeros((4, 5, 3), np.uint8))
    rc = predict.main(['--model', 'dcnf', '--superpixel', '20', '--checkpoint', str(tmp_path / 'patch.pt'), '--out',
                       str(tmp_path / 'out'), img])
    assert rc == 2 and 'needs --unary fcsp' in capsys.readouterr().err


def test_read_image_and_depth_png(tmp_path):
    from ann3depth_amd import imresize, png, predict
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    png.imsave(str(tmp_path / 'rgb.png'), rgb)
    png.imsave(str(tmp_path / 'grey.png'), rgb[..., 0])
    assert np.array_equal(predict.read_image(str(tmp_path / 'rgb.png')), rgb)
    grey = predict.read_image(str(tmp_path / 'grey.png'))
    assert grey.shape == (5, 7, 3) and all(np.array_equal(grey[..., c], rgb[..., 0]) for c in range(3))
    d = rng.uniform(0.5, 9, (5, 7)).astype(np.float32)
    assert np.array_equal(predict.depth_png(d), imresize.bytescale(d))
    holes = d.copy()
    holes[0, 0], holes[1, 2], holes[4, 6] = np.nan, np.inf, -np.inf
    img = predict.depth_png(holes)
    ok = np.isfinite(holes)
    assert img.dtype == np.uint8 and (img[~ok] == 0).all()
    lo, hi = holes[ok].min(), holes[ok].max()
    assert np.array_equal(img[ok], ((holes[ok] - lo) * (255.0 / (hi - lo)) + 0.5).astype(np.uint8))
    assert img[ok].min() == 0 and img[ok].max() == 255
    assert (predict.depth_png(np.full((2, 2), np.nan, np.float32)) == 0).all()
    assert (predict.depth_png(np.full((2, 2), 3, np.float32)) == 0).all()
    assert predict.batches([np.zeros((2, 3, 3))] * 3 + [np.zeros((4, 3, 3))] + [np.zeros((2, 3, 3))], 2) == [[0, 1], [2], [3], [4]]


def test_evaluate_parse_args_upsample():
    from ann3depth_amd import evaluate
    a = evaluate.parse_args(['--upsample', 'joint', 'nyu'])
    assert (a.upsample, a.radius, a.sigma_space, a.sigma_range, a.dataset) == ('joint', 2, 1.0, 0.1, 'nyu')
    a = evaluate.parse_args(['nyu'])
    assert a.upsample == 'none'
    with pytest.raises(SystemExit):
        evaluate.parse_args(['--upsample', 'bilinear', 'nyu'])
    a = evaluate.parse_args(['--upsample', 'joint', '--radius', '1', '--sigma-space', '0.5', '--sigma-range', 'inf', 'nyu'])
    assert (a.radius, a.sigma_space, a.sigma_range) == (1, 0.5, float('inf'))
