"""The prediction driver end to end (image files in, depth maps out) and `evaluate --upsample joint`, on checkpoints
these tests save from freshly seeded replicas: every file the driver writes is, bit for bit, the ops call applied to the
replica's predict() of the same pixels."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_eval_dcnf import _write

pytestmark = pytest.mark.gpu

B = 2
SIZES = [(48, 64), (48, 64), (30, 41)]                 # two of one size run as one batch, the third alone (zero-padded)
METRICS = {'abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'log10', 'rmse_si', 'delta1', 'delta2', 'delta3', 'pixels', 'images',
           'images_without_valid_pixels', 'nonfinite'}


def make_replica(model):
    from ann3depth_amd import models
    if model == 'msdn':
        return models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False)
    return models.DCNFReplica(B, device='cuda:0', unary='fcsp', superpixel=20)


def model_args(model):
    return ['--model', model] + (['--superpixel', '20'] if model == 'dcnf' else [])


@pytest.fixture(scope='module', params=['msdn', 'dcnf'])
def setup(request, tmp_path_factory):
    """(model, checkpoint path, replica holding its weights, image paths, their pixels)."""
    from ann3depth_amd import png
    model = request.param
    tmp = tmp_path_factory.mktemp(model)
    rep = make_replica(model)
    ckpt = str(tmp / 'weights.pt')
    torch.save({k: v.detach().cpu() for k, v in rep.state_dict().items()}, ckpt)
    rng = np.random.default_rng(12)
    paths, pixels = [], []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        img[:, w // 2:] //= 3                                            # an edge for the guide to find
        if i == 1:
            img = np.repeat(img[..., :1], 3, axis=2)
            png.imsave(str(tmp / f'img{i}.png'), img[..., 0])              # a grey file: read as three equal channels
        else:
            png.imsave(str(tmp / f'img{i}.png'), img)
        paths.append(str(tmp / f'img{i}.png')), pixels.append(img)
    return model, ckpt, rep, paths, pixels, tmp


def expected(model, rep, pixels, mode):
    """What the driver must write for images [pixels], through the same replica calls and ops."""
    from ann3depth_amd import ops
    out = []
    for idx in ([0, 1], [2]):
        x = torch.from_numpy(np.stack([pixels[i] for i in idx])).cuda()
        n = len(idx)
        pred = rep.predict(x, n)[1][:n]
        if mode == 'joint':
            up = ops.JointUpsampler('corner' if model == 'msdn' else 'block', None if model == 'msdn' else 20)
            full = up(pred, x)
        elif mode == 'bilinear':
            full = ops.resize_bilinear_tf1(pred.reshape(n, *pred.shape[1:], 1),
                                           torch.empty((n, *x.shape[1:3], 1), device='cuda'))[..., 0]
        else:
            full = pred
        torch.cuda.synchronize()
        out += list(full.cpu().numpy())
    return out


@pytest.mark.parametrize('mode', ['joint', 'bilinear', 'none'])
def test_predict_writes_what_ops_computes(setup, mode, capsys):
    from ann3depth_amd import imresize, png, predict
    model, ckpt, rep, paths, pixels, tmp = setup
    out = str(tmp / f'out-{mode}')
    flags = [] if mode == 'joint' else ['--upsample', mode]              # joint is the default
    capsys.readouterr()
    assert predict.main(model_args(model) + ['--checkpoint', ckpt, '--batchsize', str(B), '--out', out] + flags + paths) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res['model'] == model and res['upsample'] == mode and res['checkpoint'] == ckpt and len(res['files']) == 3
    assert res['output'] == ('fine' if model == 'msdn' else 'crf') and res['nonfinite'] == 0
    if model == 'dcnf':
        assert res['singular_systems'] == 0 and res['superpixel'] == 20
    if mode == 'joint':
        assert (res['radius'], res['sigma_space'], res['sigma_range']) == (2, 1.0, 0.1)
    want = expected(model, rep, pixels, mode)
    grid = (55, 74) if model == 'msdn' else (12, 16)
    for i, f in enumerate(res['files']):
        got = np.load(f['npy'])
        size = grid if mode == 'none' else SIZES[i]
        assert got.dtype == np.float32 and got.shape == size and f['size'] == list(size) and f['image_size'] == list(SIZES[i])
        assert f['image'] == paths[i] and os.path.basename(f['npy']) == f'img{i}-depth.npy' and f['nonfinite'] == 0
        assert np.array_equal(got.view(np.uint32), want[i].view(np.uint32)), (i, np.abs(got - want[i]).max())
        img = png.imread(f['png'])
        assert img.dtype == np.uint8 and img.shape == size
        assert np.array_equal(img, imresize.bytescale(got))               # min -> 0, max -> 255, + 0.5 and truncated
        assert got.max() == got.min() or (img.min() == 0 and img.max() == 255)
    if mode == 'joint':                                    # and the three modes are three different maps
        other = expected(model, rep, pixels, 'bilinear')
        assert not np.array_equal(want[0], other[0])


def test_evaluate_upsample_joint_adds_an_output_and_changes_nothing_else(setup, capsys):
    from ann3depth_amd import evaluate
    model, ckpt, rep, paths, pixels, tmp = setup
    root = str(tmp / 'data')
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    _write(os.path.join(root, 'nyu', 'test.tfrecords'), 5, 1)            # 48 x 64 images, 6 x 8 depth maps; batches 2, 2, 1
    base = model_args(model) + ['--batchsize', str(B), '--ckptdir', str(tmp / 'ck'), '--datadir', root, '--checkpoint', ckpt]
    capsys.readouterr()
    assert evaluate.main(base + ['nyu']) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert evaluate.main(base + ['--upsample', 'joint', '--radius', '1', '--sigma-range', '0.25', 'nyu']) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    name = 'fine_joint' if model == 'msdn' else 'crf_joint'
    assert set(got) - set(plain) == {name, 'upsample', 'radius', 'sigma_space', 'sigma_range'}
    assert (got['upsample'], got['radius'], got['sigma_space'], got['sigma_range']) == ('joint', 1, 1.0, 0.25)
    assert set(got[name]) == METRICS and got[name]['images'] == 5 and got[name]['pixels'] == plain[name[:-6]]['pixels']
    assert all(np.isfinite(got[name][k]) for k in METRICS)
    for k in plain:                                                      # every other key: the same values, NaN included
        assert json.dumps(got[k], sort_keys=True) == json.dumps(plain[k], sort_keys=True), k
    run = os.path.join(str(tmp / 'ck'), model)
    on_disk = json.load(open(os.path.join(run, f'eval-{got["global_step"]}.json')))
    assert on_disk[name] == got[name]
    blob = b''.join(open(os.path.join(run, f), 'rb').read() for f in os.listdir(run) if f.startswith('events.out.tfevents.'))
    assert f'eval/{name}/abs_rel'.encode() in blob
