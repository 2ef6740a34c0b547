"""a3d_warp_bilinear_pair on the GPU, held bit for bit to tests/augment_ref.py (pinned on the CPU by
tests/test_augment_cpu.py), every output a window of a sentinel-filled allocation whose guard elements must keep their
bits; then the training step and the driver with the augmentation on."""
import json
import os
import signal

import numpy as np
import pytest
import torch

import augment_ref as R
from ann3depth_amd import augment as A
from oracle import msdn as O

pytestmark = pytest.mark.gpu

SENT = 7.0
SIZES = [(480, 640, 228, 304, 55, 74), (48, 64, 228, 304, 55, 74), (7, 5, 3, 4, 3, 4)]   # h, w, oh0, ow0, oh1, ow1


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


def sources(rng, n, h, w, kind):
    """(image, depth) numpy sources: kind 'u8', 'f32', or 'mixed' (uint8 image beside a float32 depth map)."""
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dep = rng.integers(0, 256, (n, h, w, 1), dtype=np.uint8)
    if kind == 'f32':
        return rng.random((n, h, w, 3), dtype=np.float32), rng.random((n, h, w, 1), dtype=np.float32) * np.float32(10)
    if kind == 'mixed':
        return img, rng.random((n, h, w, 1), dtype=np.float32) * np.float32(10)
    return img, dep


def run_pair(ops, img, dep, table, oh0, ow0, oh1, ow1):
    n = img.shape[0]
    y0, y1 = Guarded(n, oh0, ow0, img.shape[3]), Guarded(n, oh1, ow1, dep.shape[3])
    ops.warp_bilinear_pair(dev(img), y0.t, dev(dep), y1.t, dev(table))
    torch.cuda.synchronize()
    return y0.host(), y1.host()


def check_pair(ops, img, dep, table, oh0, ow0, oh1, ow1):
    got0, got1 = run_pair(ops, img, dep, table, oh0, ow0, oh1, ow1)
    want0, want1 = R.warp(img, table, oh0, ow0), R.warp(dep, table, oh1, ow1, second=True)
    np.testing.assert_array_equal(bits(got0), bits(want0))
    np.testing.assert_array_equal(bits(got1), bits(want1))
    return got0, got1


def some_tables(n, h, w, seed):
    """Named tables of n rows: identity, flips, integer and fractional translations, random Eigen draws."""
    flip = R.identity(n)
    flip[:, 0], flip[:, 2] = -1, w - 1
    vflip = R.identity(n)
    vflip[:, 4], vflip[:, 5] = -1, h - 1
    shift = R.identity(n)
    shift[:, 2], shift[:, 5] = np.arange(n) % 3, (np.arange(n) + 1) % 2
    frac = R.identity(n)
    frac[:, 2], frac[:, 5] = np.float32(0.37) + np.arange(n, dtype=np.float32) / 8, np.float32(1.625)
    frac[:, 6:9], frac[:, 10] = np.float32([0.8, 1.2, 1.0625]), np.float32(0.75)
    return {'identity': R.identity(n), 'flip': flip, 'vflip': vflip, 'shift': shift, 'frac': frac,
            'eigen': A.table(A.Eigen2014(), seed, 0, 3, n, h, w)}


@pytest.mark.parametrize('kind', ['u8', 'f32', 'mixed'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w,oh0,ow0,oh1,ow1', SIZES)
def test_warp_pair_is_the_reference_bit_for_bit(ops, h, w, oh0, ow0, oh1, ow1, n, kind):
    rng = np.random.default_rng(h * 10 + n)
    img, dep = sources(rng, n, h, w, kind)
    for name, table in some_tables(n, h, w, seed=h + n).items():
        got0, got1 = check_pair(ops, img, dep, table, oh0, ow0, oh1, ow1)
        if name == 'identity':                       # also against the resize launch it replaces
            z0, z1 = Guarded(n, oh0, ow0, 3), Guarded(n, oh1, ow1, 1)
            ops.resize_bilinear_tf1_pair(dev(img), z0.t, dev(dep), z1.t)
            np.testing.assert_array_equal(bits(got0), bits(z0.host()))
            np.testing.assert_array_equal(bits(got1), bits(z1.host()))


@pytest.mark.parametrize('kind', ['u8', 'mixed'])
def test_warp_pair_at_the_training_batch(ops, kind):
    """n = 32 at the stored size of the flagship workload, random Eigen tables of several steps."""
    rng = np.random.default_rng(32)
    img, dep = sources(rng, 32, 480, 640, kind)
    for step in (0, 1):
        check_pair(ops, img, dep, A.table(A.Eigen2014(), 3000, 0, step, 32, 480, 640), 228, 304, 55, 74)


def test_same_size_flip_is_the_flipped_tensor(ops):
    rng = np.random.default_rng(4)
    img, dep = sources(rng, 3, 48, 64, 'f32')
    t = some_tables(3, 48, 64, 0)['flip']
    got0, got1 = check_pair(ops, img, dep, t, 48, 64, 48, 64)
    np.testing.assert_array_equal(bits(got0), bits(img[:, :, ::-1]))
    np.testing.assert_array_equal(bits(got1), bits(dep[:, :, ::-1]))


def test_single_tensor_form_and_four_channels(ops):
    rng = np.random.default_rng(5)
    x = rng.random((3, 48, 64, 4), dtype=np.float32)
    t = A.table(A.Eigen2014(), 9, 0, 0, 3, 48, 64)
    t[:, 9] = np.float32(1.5)
    for src in (x, rng.integers(0, 256, (3, 48, 64, 4), dtype=np.uint8)):
        y = Guarded(3, 31, 45, 4)
        ops.warp_bilinear_pair(dev(src), y.t, None, None, dev(t))
        np.testing.assert_array_equal(bits(y.host()), bits(R.warp(src, t, 31, 45)))


def test_tensors_of_different_stored_sizes_are_refused(ops):
    """48 x 64 images beside 6 x 8 depth maps: one map in source pixels cannot serve both.  The C ABI carries ONE stored
    h x w for the pair, so this refusal is the operator layer's (ValueError before the library is called); the library's
    own A3D_EINVAL is shown on a fifth channel."""
    from ann3depth_amd import _lib
    x0, x1 = torch.zeros((2, 48, 64, 3), device='cuda'), torch.zeros((2, 6, 8, 1), device='cuda')
    y0, y1 = Guarded(2, 228, 304, 3), Guarded(2, 55, 74, 1)
    with pytest.raises(ValueError, match='second tensor'):
        ops.warp_bilinear_pair(x0, y0.t, x1, y1.t, dev(R.identity(2)))
    five = torch.zeros((2, 48, 64, 5), device='cuda')
    y5 = Guarded(2, 4, 4, 5)
    with pytest.raises(_lib.A3dError, match='channel gains'):              # A3D_EINVAL from the library
        ops.warp_bilinear_pair(five, y5.t, None, None, dev(R.identity(2)))
    lib = _lib.load()
    rc = lib.a3d_warp_bilinear_pair(2, 48, 64, 5, five.data_ptr(), 0, 4, 4, y5.t.data_ptr(), 0, None, 0, 0, 0, None,
                                    dev(R.identity(2)).data_ptr(), None)
    assert rc == -1
    torch.cuda.synchronize()
    assert (y0.host() == SENT).all() and (y1.host() == SENT).all() and (y5.host() == SENT).all()


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_wild_and_nan_coefficients_are_decided_by_the_clamp(ops, kind):
    """Coordinates far outside the image, infinite and NaN: the clamp decides which pixel is read, nothing outside the
    image is, and the neighbouring images of the batch keep their bits."""
    rng = np.random.default_rng(6)
    n, h, w = 6, 48, 64
    img, dep = sources(rng, n, h, w, kind)
    t = A.table(A.Eigen2014(), 2, 0, 0, n, h, w)
    calm = t.copy()
    t[1, 2], t[1, 5] = 1e30, -1e30
    t[2, 0] = np.nan
    t[3, 2], t[3, 4] = np.inf, -1e38
    t[4, :6] = [3e38, 3e38, 3e38, -3e38, -3e38, -3e38]
    got0, got1 = check_pair(ops, img, dep, t, 228, 304, 55, 74)
    ref0, ref1 = R.warp(img, calm, 228, 304), R.warp(dep, calm, 55, 74, second=True)
    for b in (0, 5):
        np.testing.assert_array_equal(bits(got0[b]), bits(ref0[b]))
        np.testing.assert_array_equal(bits(got1[b]), bits(ref1[b]))
    f = R.as_float(dep)
    np.testing.assert_array_equal(got1[1], np.broadcast_to(f[1, 0, w - 1] * t[1, 10], (55, 74, 1)))


# ---------------------------------------------------------------------------------------------- the step
def test_step_with_a_table_is_the_step_on_the_reference_warped_tensors():
    """Two replicas, same weights and keep mask: one warps the stored batch inside its step, the other gets the reference's
    warped 228 x 304 / 55 x 74 tensors (a same-size resize is the identity bit for bit).  Outputs, both losses and every
    variable and Adam slot must be bit-identical."""
    from ann3depth_amd import models
    B = 4
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8)
    dep = rng.integers(1, 256, (B, 480, 640, 1), dtype=np.uint8)
    keep = dev((rng.random((B, 4096)) >= 0.5).astype(np.uint8))
    params = O.init_params(3000)
    nets = [models.MSDNReplica(B, params=params, beta2=0.999) for _ in range(2)]
    for step in range(2):
        T = A.table(A.Eigen2014(), 3000, 0, step, B, 480, 640)
        x_ref, t_ref = R.warp(img, T, 228, 304), R.warp(dep, T, 55, 74, second=True)
        a = nets[0].step(dev(img), dev(dep), keep, warp=dev(T))
        b = nets[1].step(dev(x_ref), dev(t_ref), keep)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(nets[0].x.cpu().numpy()), bits(x_ref))
        np.testing.assert_array_equal(bits(nets[0].t.cpu().numpy()), bits(t_ref))
        assert float(a['coarse_loss']) == float(b['coarse_loss']) and float(a['fine_loss']) == float(b['fine_loss'])
        assert np.isfinite(float(a['coarse_loss']))
        assert torch.equal(nets[0].coarse, nets[1].coarse) and torch.equal(nets[0].fine, nets[1].fine)
    for gname in nets[0].groups:
        ga, gb = nets[0].groups[gname], nets[1].groups[gname]
        for buf in ('var', 'm', 'v'):
            assert torch.equal(getattr(ga, buf), getattr(gb, buf)), f'{gname}.{buf}'
    assert float(nets[0].groups['CoarseDense'].m.abs().sum()) > 0
    # and the table matters: the plain step on the same batch gives another loss
    plain = models.MSDNReplica(B, params=params, beta2=0.999)
    c = plain.step(dev(img), dev(dep), keep)
    assert float(c['coarse_loss']) != float(a['coarse_loss'])


# ---------------------------------------------------------------------------------------------- the driver
def write_shard(root, n=24):
    """One record n times, image and depth map both 48 x 64: a resumed run starts its shuffle queue afresh (as the
    reference's does), so only a shard whose every batch is the same batch lets two runs be compared step by step.
    What differs from step to step is then the table, the keep mask and the Adam state."""
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    img = rng.integers(0, 256, (48, 64, 3)).astype(np.float32) / np.float32(255) - np.float32(.5)
    dep = rng.integers(1, 256, (48, 64, 1)).astype(np.float32) / np.float32(255) - np.float32(.5)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'train.tfrecords')) as w:
        for _ in range(n):
            w.write_example(img, dep)


def losses(ck, run):
    rows = [json.loads(l) for l in open(os.path.join(ck, run, 'summaries.jsonl'))]
    return {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss']) for r in rows}


def test_driver_with_augmentation_is_reproducible_and_resumable(tmp_path):
    from ann3depth_amd import ann3depth, models
    write_shard(str(tmp_path))
    ck = str(tmp_path / 'ckpt')
    base = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', str(tmp_path), '--sumfreq', '1',
            '--trace-every', '0']

    def run(run_id, steps, *flags):
        assert ann3depth.main(base + ['--id', run_id, '--steps', str(steps), *flags, 'nyu']) == 0
        return losses(ck, 'msdn_' + run_id)
    try:
        a = run('a', 6, '--augment', 'eigen')
        b = run('b', 6, '--augment', 'eigen')
        assert sorted(a) == [1, 2, 3, 4, 5, 6] and a == b                  # same seeds: the same loss sequence
        assert len({v for v in a.values()}) == 6                           # ... and a new table at every step
        first = run('c', 3, '--augment', 'eigen')
        assert ann3depth.latest_checkpoint(os.path.join(ck, 'msdn_c')).endswith('model.ckpt-3.pt')
        resumed = run('c', 6, '--augment', 'eigen')                        # continues from the step-3 checkpoint
        assert first == {k: a[k] for k in (1, 2, 3)}
        assert resumed == a                                                # steps 4..6 as the uninterrupted run logged them
        none = run('d', 6, '--augment', 'none')
        assert models.msdn.augment is None
        plain = run('e', 6)
        assert none == plain
        assert all(none[k] != a[k] for k in a)
    finally:
        models.msdn.augment = None
        for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
            signal.signal(s, signal.SIG_DFL)
