"""Scale-and-shift alignment on the GPU (include/a3d_align.h): a3da_depth_align, a3da_depth_metrics_aligned and
a3da_affine_apply against the host reference of tests/align_ref.py, at the smallest shapes at which each path can go wrong.

count and status are exact; 'median' coefficients are the reference's bits.  'scale' and 'affine' coefficients are within ONE
float32 step of the exactly computed value, which is derived, not measured: a float64 sum of m exact products errs by at most
m 2^-53 of the sum of its terms' magnitudes in any order, so the numerator of s is off by at most m 2^-53 cond of itself (cond =
sum |terms| / |numerator|) and the denominator by m 2^-53 kappa (kappa = S_pp / (S_pp - S_p^2 / m)).  Every drawn case is
asserted to have kappa <= 100 and cond <= 1000; with m <= 6912 the float64 value is then within 1e-9 of the exact one, far
inside the 6e-8 of half a float32 step, so its rounding is the exact value's rounding or a neighbour of it."""
import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu

# name: (prediction grid, target grid, uint8 target, target base offset by one element)
SHAPES = {
    'resampled': ((3, 4), (6, 8), False, False),           # the sampler; 48 pixels: whole groups of four
    'tail': ((5, 7), (5, 7), False, False),                # same grid; 35 pixels: the scalar tail
    'onepart': ((55, 74), (55, 74), False, False),         # 4070 pixels: one part
    'twoparts': ((36, 48), (72, 96), False, False),        # 6912 pixels: two parts of kPixelsPerPart = 4096
    'u8': ((3, 4), (6, 8), True, False),                   # the look-up table, 4-byte loads
    'u8tail': ((5, 7), (5, 7), True, False),
    'offset': ((6, 8), (6, 8), False, True),               # a float target 4 bytes off the 16-byte grid: no vector loads
}
N = 3
HOLES = {False: (0.1, 0.5, 0.9), True: (0.1, 0.3, 0.5)}     # a different mask per image; [fewer than 100 pixels]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def draw(shape, family, seed):
    """(pred [N, ph, pw], the target as stored, the target as float32, depth range).  The prediction carries NaN and +-inf."""
    (ph, pw), (th, tw), u8, _ = SHAPES[shape]
    rng = np.random.default_rng(seed)
    kw = dict(min_depth=0.0, max_depth=float('inf'))
    if family == 'uniform':
        p = rng.uniform(0.5, 1.5, (N, ph, pw)).astype(np.float32)
    elif family == 'quantised':                            # four values: heavy ties in one bin
        p = rng.choice(np.float32([0.5, 0.75, 1.0, 1.25]), (N, ph, pw))
    elif family == 'wide':                                 # both signs, many exponents, zeros of both signs
        p = (rng.choice([-1, 1], (N, ph, pw), p=[0.3, 0.7]) * rng.uniform(1, 2, (N, ph, pw)) *
             2.0 ** rng.integers(-60, 60, (N, ph, pw))).astype(np.float32)
        p.reshape(-1)[rng.permutation(p.size)[:4]] = np.float32([0.0, -0.0, 0.0, -0.0])
    else:                                                  # denormals, and a few values at the top of the range
        p = (rng.integers(1, 1 << 22, (N, ph, pw)).astype(np.uint32)).view(np.float32).copy()
        p.reshape(-1)[rng.permutation(p.size)[:3]] = np.float32([3e38, 1e-38, 2e-45])
    ps = R.sampled(p, th, tw)
    noise = rng.uniform(-0.1, 0.1, (N, th, tw))
    if family in ('uniform', 'quantised'):
        t = (1.5 * ps + 0.25 + noise).astype(np.float32)
    elif family == 'wide':
        t = (rng.choice([-1, 1], (N, th, tw), p=[0.3, 0.7]) * rng.uniform(1, 2, (N, th, tw)) *
             2.0 ** rng.integers(-60, 60, (N, th, tw))).astype(np.float32)
        t.reshape(-1)[rng.permutation(t.size)[:2]] = np.float32([0.0, -0.0])
        kw['min_depth'] = float('-inf')                    # negative targets count
    else:
        t = (rng.integers(1, 1 << 22, (N, th, tw)).astype(np.uint32)).view(np.float32).copy()
    for i, share in enumerate(HOLES[th * tw < 100]):                      # holes of every kind
        hole = rng.random((th, tw)) < share
        t[i][hole] = rng.choice(np.float32([np.nan, np.inf, -np.inf] + ([] if family == 'wide' else [0.0, -1.0])), int(hole.sum()))
    flat = p.reshape(N, -1)
    for i in range(N):                                     # NaN and +-inf predictions (on the same grid: at valid pixels too)
        bad = np.float32([np.nan, np.inf, -np.inf])[:3 if flat.shape[1] >= 35 else 1]
        flat[i, rng.permutation(flat.shape[1])[:len(bad)]] = bad
    if (ph, pw) == (th, tw):
        t[0, 0, 0], p[0, 0, 0] = (t[np.isfinite(t) & (t > 0)][0], np.nan)     # a valid pixel with a NaN prediction
    if u8:
        assert family in ('uniform', 'quantised')
        with np.errstate(invalid='ignore'):
            stored = np.where(np.isfinite(t) & (t > 0), np.clip(np.rint(t * 90), 1, 255), 0).astype(np.uint8)
        from ann3depth_amd import data
        return p, stored, data.expand_u8(stored), kw
    return p, t, t, kw


def target_tensor(shape, stored):
    if not SHAPES[shape][3]:
        return dev(stored)
    flat = torch.empty(stored.size + 1, dtype=torch.float32, device='cuda')
    flat[1:] = dev(stored).reshape(-1)
    tgt = flat[1:].view(stored.shape)
    assert tgt.data_ptr() % 16 == 4 and tgt.is_contiguous()
    return tgt


FAMILIES = ('uniform', 'quantised', 'wide', 'denormal')
# every mode on the depth-like families; the selection also on the inputs made for it (float targets: a uint8 record has
# neither signs nor denormals), where the one-ulp bound of the least-squares modes has no bounded kappa and cond to rest on
CASES = [(s, f, m) for s in SHAPES for f in FAMILIES[:2] for m in R.MODES] + \
        [(s, f, 'median') for s in SHAPES if not SHAPES[s][2] for f in FAMILIES[2:]]


@pytest.mark.parametrize('shape,family,mode', CASES)
def test_depth_align_against_the_exact_reference(shape, family, mode):
    from ann3depth_amd import ops
    p, stored, tf32, kw = draw(shape, family, sorted(SHAPES).index(shape) * 10 + FAMILIES.index(family))
    pred, tgt = dev(p), target_tensor(shape, stored)
    coef, count, status = ops.depth_align(pred, tgt, mode, **kw)
    again = ops.depth_align(pred, tgt, mode, **kw)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((coef, count, status), again))          # the same bits on every run
    ref = R.ref_align(p, tf32, mode, **kw)
    c = coef.cpu().numpy()
    print(f'{shape} {family} {mode}: count {ref["count"].tolist()} status {ref["status"].tolist()} coef {c.tolist()} '
          f'kappa {ref["kappa"].max():.3g} cond {ref["cond"].max():.3g}')
    np.testing.assert_array_equal(count.cpu().numpy(), ref['count'])
    np.testing.assert_array_equal(status.cpu().numpy(), ref['status'])
    assert ref['count'].min() >= 1
    if mode == 'median':
        assert c.tobytes() == ref['coef'].tobytes()
    else:
        assert (ref['status'] == 0).all()
        assert ref['kappa'].max() <= 100 and ref['cond'].max() <= 1000
        assert R.ulps(c, ref['coef']).max() <= 1, (c, ref['coef'])
    if family in ('wide', 'denormal'):
        assert (ref['status'] == 0).any()
        return                                             # (targets no float64 reference of the metrics is defined on)
    # the aligned rows, fed the kernel's own coefficients
    rows = ops.depth_metrics(pred, tgt, coef=coef, **kw)
    rows2 = ops.depth_metrics(pred, tgt, coef=coef, **kw).clone()
    one = dev(np.tile(np.float32([1, 0]), (N, 1)))
    ident = ops.depth_metrics(pred, tgt, coef=one, **kw).clone()
    plain = ops.depth_metrics(pred, tgt, **kw).clone()
    torch.cuda.synchronize()
    assert same_bits(rows, rows2)
    assert same_bits(ident, plain)                         # coef (1, 0), clamp_lo > 0: a3d_depth_metrics' rows bit for bit
    want = R.aligned_rows(p, tf32, c, **kw)
    R.check_rows(rows.cpu().numpy(), want, R.aligned_rows(p, tf32, c, magnitude=True, **kw))
    assert (want[:, 0] == ref['count']).all()              # nothing overflowed: the fitted pixels are the judged ones
    assert want[:, 10].sum() > 0                           # NaN / inf predictions on valid pixels: column 10 only


def small_counts():
    """Four images of 5 x 7 with m = 0, 1, 2, 3 fitted pixels."""
    rng = np.random.default_rng(77)
    p = rng.uniform(0.5, 1.5, (4, 5, 7)).astype(np.float32)
    t = np.full((4, 5, 7), np.nan, np.float32)
    for i in range(4):
        for j, v in zip(rng.permutation(35)[:i], np.float32([0.5, 1.5, 1.0])):     # spread: kappa stays small at m = 2, 3
            p[i].reshape(-1)[j] = v
            t[i].reshape(-1)[j] = np.float32(1.5) * v + np.float32(0.25)
    return p, t


@pytest.mark.parametrize('mode', R.MODES)
def test_counts_of_zero_one_two_and_three(mode):
    from ann3depth_amd import ops
    p, t = small_counts()
    coef, count, status = ops.depth_align(dev(p), dev(t), mode)
    ref = R.ref_align(p, t, mode)
    assert ref['count'].tolist() == [0, 1, 2, 3]
    assert ref['status'].tolist() == ([1, 1, 0, 0] if mode == 'affine' else [1, 0, 0, 0])
    assert count.cpu().tolist() == [0, 1, 2, 3] and status.cpu().tolist() == ref['status'].tolist()
    c = coef.cpu().numpy()
    assert c[ref['status'] == 1].tolist() == [[1.0, 0.0]] * int(ref['status'].sum())
    if mode == 'median':
        assert c.tobytes() == ref['coef'].tobytes()
    else:
        assert ref['kappa'].max() <= 100 and ref['cond'].max() <= 1000
        assert R.ulps(c, ref['coef']).max() <= 1


def test_degenerate_images_are_judged_as_they_are_and_touch_no_other_image():
    from ann3depth_amd import ops
    rng = np.random.default_rng(3)
    healthy = rng.uniform(0.5, 1.5, (2, 6, 8)).astype(np.float32)
    p = np.stack([healthy[0], np.full((6, 8), 0.75, np.float32), -healthy[1], healthy[1], healthy[0]])
    t = (np.float32(1.5) * np.abs(p) + np.float32(0.25)).astype(np.float32)
    t[1] = rng.uniform(1, 2, (6, 8)).astype(np.float32)    # image 1: a constant prediction
    t[4] = 0                                               # image 4: no valid pixel; image 2: med(p) < 0
    for mode in R.MODES:
        coef, count, status = ops.depth_align(dev(p), dev(t), mode)
        ref = R.ref_align(p, t, mode)
        want_status = {'median': [0, 0, 1, 0, 1], 'scale': [0, 0, 1, 0, 1], 'affine': [0, 1, 0, 0, 1]}[mode]
        assert ref['status'].tolist() == want_status and status.cpu().tolist() == want_status, mode
        assert count.cpu().tolist() == [48, 48, 48, 48, 0]
        c = coef.cpu().numpy()
        for i, s in enumerate(want_status):
            if s:
                assert c[i].tolist() == [1.0, 0.0], (mode, i)
        if mode == 'median':
            assert c.tobytes() == ref['coef'].tobytes()
        else:
            assert R.ulps(c, ref['coef']).max() <= 1
        # the healthy images alone: the same bits
        alone = ops.depth_align(dev(p[[0, 3]]), dev(t[[0, 3]]), mode)
        torch.cuda.synchronize()
        for got, want in zip((coef, count, status), alone):
            assert same_bits(got[[0, 3]], want), mode
        rows = ops.depth_metrics(dev(p), dev(t), coef=coef).cpu().numpy()
        plain = ops.depth_metrics(dev(p), dev(t)).cpu().numpy()
        for i, s in enumerate(want_status):
            if s:
                assert rows[i].tobytes() == plain[i].tobytes(), (mode, i)


@pytest.mark.parametrize('per_image,offset', [((5, 7), 0), ((6, 8), 0), ((6, 8), 1), ((72, 96), 0)])
def test_affine_apply_bit_for_bit_in_and_out_of_place(per_image, offset):
    from ann3depth_amd import ops
    rng = np.random.default_rng(per_image[0] + offset)
    n = 3
    x = (rng.standard_normal((n,) + per_image) * 2.0 ** rng.integers(-20, 20, (n,) + per_image)).astype(np.float32)
    x.reshape(-1)[:5] = np.float32([np.nan, np.inf, -np.inf, -0.0, 1e-42])
    coef = np.float32([[1.5, 0.25], [-3.0000002, 1e-3], [1, 0]])
    want = R.apply(x, coef)
    flat = torch.full((x.size + offset + 1,), -7.25, dtype=torch.float32, device='cuda')
    xd = flat[offset:offset + x.size].view(x.shape)
    xd.copy_(dev(x))
    out = ops.affine_apply(xd, dev(coef))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes() and xd.cpu().numpy().tobytes() == x.tobytes()
    assert not np.isfinite(out.cpu().numpy().reshape(-1)[:3]).any()
    assert ops.affine_apply(xd, dev(coef), out=xd) is xd   # in place
    torch.cuda.synchronize()
    assert xd.cpu().numpy().tobytes() == want.tobytes()
    assert float(flat[-1]) == -7.25 and (offset == 0 or float(flat[0]) == -7.25)
    with pytest.raises(ValueError):
        ops.affine_apply(xd, dev(coef[:2]))
    with pytest.raises(ValueError):
        ops.depth_align(xd, xd, 'log')
    with pytest.raises(ValueError):
        ops.depth_metrics(xd, xd, coef=dev(coef[:2]))
