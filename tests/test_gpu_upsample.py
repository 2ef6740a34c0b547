"""a3du_joint_bilateral_upsample on the GPU against tests/upsample_ref.py.

Accuracy: the kernel is the float32 restatement of the definition with another expf, so it is held to the float64
definition within 8 x the largest error the numpy restatement makes on the same inputs (both evaluate the same rounded
exponents; what differs is the exponential's last bit and nothing accumulates beyond the <= 81 terms of a window),
floored at one ulp of the output.  Everything that is exact by the definition is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import upsample_ref as U
from test_upsample_cpu import K, step_edge_case

pytestmark = pytest.mark.gpu

# (kind, sp, gh, gw, H, W): 3 x 4 is smaller than an R = 4 window; 37 x 130 is 5 x 5 tiles of 8 x 32 with tails both ways;
# kind 'block' with sp = 80 is the 3 x 4 grid of 240 x 320
SHAPES = [('corner', None, 3, 4, 7, 9), ('corner', None, 3, 4, 12, 16), ('corner', None, 5, 7, 37, 130),
          ('block', 80, 3, 4, 7, 9), ('block', 80, 3, 4, 12, 16), ('block', 40, 6, 8, 37, 130)]
N = 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tables(kind, sp, gh, gw, H, W):
    return U.tables_corner(gh, gw, H, W) if kind == 'corner' else U.tables_block(sp, H, W)


def run(depth, guide, tabs, R, sigma_s=1.0, sigma_r=0.1, out=None):
    """The launch through ops with the four host tables `tabs` as they are (any values)."""
    from ann3depth_amd import ops
    gh, gw = depth.shape[1:]
    H, W = guide.shape[1:3]
    m = ops.UpsampleMap(gh, gw, H, W, 'corner')
    m.cy, m.cx, m.ay, m.ax = (dev(t) for t in tabs)
    got = ops.joint_bilateral_upsample(dev(depth), dev(guide), m, R, sigma_s, sigma_r, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(shape, u8):
    kind, sp, gh, gw, H, W = shape
    rng = np.random.default_rng([gh, gw, H, W, int(kind == 'block')])
    depth = rng.uniform(0.5, 8, (N, gh, gw)).astype(np.float32)
    k = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    return depth, (k if u8 else U.guide_values(k)), tables(*shape)


def hold(got, depth, guide, tabs, R, sigma_s, sigma_r, what):
    """got against the float64 definition within 8 x the float32 restatement's largest error, >= 1 ulp; same NaNs."""
    args = (depth, guide, *tabs, R, U.inv2(sigma_s), U.inv2(sigma_r))
    r64, r32 = U.upsample(*args), U.upsample(*args, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == r64.shape
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and np.array_equal(np.isnan(r32), np.isnan(r64))
    ok = ~np.isnan(r64)
    assert np.isfinite(got[ok]).all()
    if not ok.any():
        return
    e32 = np.abs(r32.astype(np.float64) - r64)[ok].max()
    err = np.abs(got.astype(np.float64) - r64)[ok]
    bound = np.maximum(8 * e32, np.spacing(np.abs(r64[ok]).astype(np.float32)).astype(np.float64))
    print(f'{what}: restatement error {e32:.3g} ({(np.abs(r32 - r64)[ok] / np.abs(r64[ok])).max():.3g} rel), kernel '
          f'{err.max():.3g} ({(err / np.abs(r64[ok])).max():.3g} rel), {int((got[ok] != r32[ok]).sum())} of {int(ok.sum())} '
          f'pixels differ from the restatement')
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize('u8', [False, True], ids=['f32', 'u8'])
@pytest.mark.parametrize('R', [1, 2, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}-{s[2]}x{s[3]}-{s[4]}x{s[5]}')
def test_against_the_float64_definition(shape, R, u8):
    depth, guide, tabs = case(shape, u8)
    got = run(depth, guide, tabs, R)
    hold(got, depth, guide, tabs, R, 1.0, 0.1, f'{shape} R={R} u8={u8}')
    lo, hi = U.window_range(depth, tabs[0], tabs[1], R)
    assert (got >= lo).all() and (got <= hi).all()                       # inside the range of the window's depths
    if u8:                                                              # uint8 k is the float32 guide fl(k / 255), bit for bit
        assert np.array_equal(got, run(depth, U.guide_values(guide), tabs, R))


@pytest.mark.parametrize('sigma_s,sigma_r', [(0.5, float('inf')), (3.0, 0.02), (float('inf'), 0.3)])
def test_other_sigmas(sigma_s, sigma_r):
    """The range term off, a sharp one (most weights underflow), the space term off."""
    depth, guide, tabs = case(SHAPES[2], False)
    hold(run(depth, guide, tabs, 2, sigma_s, sigma_r), depth, guide, tabs, 2, sigma_s, sigma_r, f'sigmas {sigma_s} {sigma_r}')


def test_skipped_cells_exactly():
    depth, guide, tabs = case(SHAPES[2], False)              # 5 x 7 -> 37 x 130
    cy, cx, ay, ax = tabs
    _, gh, gw = depth.shape
    H, W = guide.shape[1:3]
    # one finite cell in the whole grid: every window that holds it returns its bits, every other pixel is NaN
    one = np.full_like(depth, np.nan)
    one[0, 2, 3], one[1, 4, 6] = np.float32(2.7182817), np.float32(0.1)
    one[0, 0, 0], one[1, 0, 1], one[1, 1, 1] = np.inf, -np.inf, np.inf
    for R in (1, 4):
        got = run(one, guide, tabs, R)
        qy, qx = U.centre(cy, gh), U.centre(cx, gw)
        for b, (ci, cj) in enumerate(((2, 3), (4, 6))):
            holds = (np.abs(qy - ci) <= R)[:, None] & (np.abs(qx - cj) <= R)[None, :]
            assert holds.any() and (R == 4 or not holds.all())
            assert np.array_equal(got[b][holds].view(np.uint32), np.full(holds.sum(), one[b, ci, cj]).view(np.uint32))
            assert np.isnan(got[b][~holds]).all()
    # no finite cell at all
    assert np.isnan(run(np.full_like(depth, np.inf), guide, tabs, 4)).all()
    # NaN and infinite depths among finite ones are left out: the result is the reference's without them
    holes = depth.copy()
    holes[0, 1, 2], holes[0, 3, 3], holes[1, 0, 0], holes[1, 4, 5] = np.nan, np.inf, -np.inf, np.nan
    got = run(holes, guide, tabs, 2)
    hold(got, holes, guide, tabs, 2, 1.0, 0.1, 'holes')
    assert np.isfinite(got).all()
    # an anchor of -1 or H (W) takes its cells out, and is never used as an index
    bad_ay, bad_ax = ay.copy(), ax.copy()
    bad_ay[1], bad_ay[4], bad_ax[0], bad_ax[5] = -1, H, W, -1
    got = run(depth, guide, (cy, cx, bad_ay, bad_ax), 1)
    hold(got, depth, guide, (cy, cx, bad_ay, bad_ax), 1, 1.0, 0.1, 'anchors outside')
    gone = depth.copy()
    gone[:, [1, 4], :] = np.nan
    gone[:, :, [0, 5]] = np.nan
    assert np.array_equal(got, run(gone, guide, tabs, 1), equal_nan=True)      # the same as cells without a depth
    far = (cy, cx, np.full_like(ay, 2 ** 31 - 1), np.full_like(ax, -2 ** 31))
    assert np.isnan(run(depth, guide, far, 2)).all()
    # a NaN in cy, in cx, or at a guide pixel: NaN at exactly the pixels the definition says
    ncy, ncx, g = cy.copy(), cx.copy(), guide.copy()
    ncy[[0, 9, 36]], ncx[[31, 32, 129]] = np.nan, np.nan
    g[0, 5, 40, 1], g[1, 20, 100, 2] = np.nan, np.inf
    g[0, ay[2], ax[3], 0] = np.nan                            # the pixel itself, and cell (2, 3) of image 0 for everyone
    got = run(depth, g, (ncy, ncx, ay, ax), 2)
    hold(got, depth, g, (ncy, ncx, ay, ax), 2, 1.0, 0.1, 'NaN tables and guide')
    want = np.zeros((N, H, W), bool)
    want[:, [0, 9, 36], :] = True
    want[:, :, [31, 32, 129]] = True
    want[0, 5, 40] = want[1, 20, 100] = want[0, ay[2], ax[3]] = True
    assert np.array_equal(np.isnan(got), want)


def test_tables_of_any_shape_and_the_tiles_that_do_not_fit_lds():
    """Tables that jump over a 40 x 40 grid make every tile's cell range the whole grid (1600 cells, more than the
    kernel stages): those tiles read their cells from memory, with the same result.  Values far outside the grid, and
    infinite ones, clamp to its border."""
    rng = np.random.default_rng(11)
    gh = gw = 40
    H, W = 9, 33
    depth = rng.uniform(0.5, 8, (N, gh, gw)).astype(np.float32)
    guide = rng.random((N, H, W, 3)).astype(np.float32)
    cy, cx = rng.uniform(-3, 43, H).astype(np.float32), rng.uniform(-3, 43, W).astype(np.float32)
    cy[0], cy[7], cx[0], cx[31], cy[3], cx[20] = -3, 43, -3, 43, 38.6, 39.4      # tile (0, 0) spans the grid for certain
    ay, ax = rng.integers(0, H, gh).astype(np.int32), rng.integers(0, W, gw).astype(np.int32)
    for R in (1, 3):
        got = run(depth, guide, (cy, cx, ay, ax), R, 2.0, 0.2)
        hold(got, depth, guide, (cy, cx, ay, ax), R, 2.0, 0.2, f'jumping tables R={R}')
        assert np.isfinite(got).all()
    # a distance whose square overflows float32 makes the exponent infinite: the pixel has no cell left (the float64
    # reference would keep it, so only the float32 restatement is asked)
    cx[7], cx[8] = 1e30, -1e30
    got = run(depth, guide, (cy, cx, ay, ax), 2, 2.0, 0.2)
    assert np.isnan(got[:, :, [7, 8]]).all() and np.isfinite(np.delete(got, [7, 8], axis=2)).all()
    r32 = U.upsample(depth, guide, cy, cx, ay, ax, 2, U.inv2(2.0), U.inv2(0.2), dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(r32))
    cx[7], cx[8] = np.inf, -np.inf
    got = run(depth, guide, (cy, cx, ay, ax), 2, float('inf'), 0.2)      # the space term off: inf * 0 is still NaN
    assert np.isnan(got[:, :, [7, 8]]).all() and np.isfinite(np.delete(got, [7, 8], axis=2)).all()


def test_a_step_edge_keeps_its_side_on_the_gpu():
    depth, guide, side = step_edge_case()
    tabs = U.tables_corner(3, 4, 12, 16)
    for g in (guide, (guide * 255).astype(np.uint8)):
        got = run(depth, g, tabs, 2, 1.0, 0.05)
        err = np.abs(got.astype(np.float64) - side)
        print(f'step edge on the GPU: max error {(err / (2.0 ** -23 * side)).max():.2f} ulp')
        assert (err <= (2 * K + 2) * 2.0 ** -24 * np.abs(side.astype(np.float64))).all()


def test_guard_bands_and_repeatability():
    depth, guide, tabs = case(SHAPES[2], True)
    H, W = guide.shape[1:3]
    guard = np.float32(-7.25)
    big = torch.full((N + 2, H, W), float(guard), device='cuda')
    got = run(depth, guide, tabs, 2, out=big[1:1 + N])
    first = big.clone()
    again = run(depth, guide, tabs, 2, out=big[1:1 + N])
    assert torch.equal(first, big) and np.array_equal(got, again)       # the same bits on every run
    assert (big[0] == float(guard)).all() and (big[-1] == float(guard)).all()
    assert np.array_equal(big[1:1 + N].cpu().numpy(), got) and np.isfinite(got).all()
    fresh = run(depth, guide, tabs, 2)                                  # a tensor ops allocates itself: every element written
    assert np.array_equal(fresh, got)
