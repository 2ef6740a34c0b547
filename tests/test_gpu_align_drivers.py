"""`evaluate --align` and `predict --align MODE --align-to DIR` end to end (include/a3d_align.h), for both models, on
checkpoints these tests save from freshly seeded replicas, a handful of 48 x 64 records and three image files."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_eval_dcnf import _write
from test_gpu_predict import B, METRICS, SIZES, make_replica, model_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', params=['msdn', 'dcnf'])
def setup(request, tmp_path_factory):
    """(model, checkpoint path, image paths, directory)."""
    from ann3depth_amd import png
    model = request.param
    tmp = tmp_path_factory.mktemp('align-' + model)
    rep = make_replica(model)
    ckpt = str(tmp / 'weights.pt')
    sd = {k: v.detach().cpu().clone() for k, v in rep.state_dict().items()}
    # a freshly seeded network predicts around or below zero (msdn -0.05 +- 0.05, dcnf -0.41 +- 0.002); depths are
    # positive, so the bias of the last layer is raised until every output is
    name, shift = {'msdn': ('fine/third/bias', 0.3), 'dcnf': ('unary/unary_layers/dense_2/bias', 0.42)}[model]
    sd[name] = sd[name] + shift
    torch.save(sd, ckpt)
    rng = np.random.default_rng(12)
    paths = []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        img[:, w // 2:] //= 3
        png.imsave(str(tmp / f'img{i}.png'), img)
        paths.append(str(tmp / f'img{i}.png'))
    return model, ckpt, paths, tmp


def run(capsys, main, argv):
    capsys.readouterr()
    rc = main(argv)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert rc == 0 and len(lines) == 1
    return json.loads(lines[0])


def predict_args(model, ckpt, out, upsample='none'):
    return model_args(model) + ['--checkpoint', ckpt, '--batchsize', str(B), '--upsample', upsample, '--out', out]


def test_evaluate_align_adds_a_twin_to_every_output_and_nothing_else(setup, capsys):
    from ann3depth_amd import evaluate
    model, ckpt, paths, tmp = setup
    root = str(tmp / 'data')
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    _write(os.path.join(root, 'nyu', 'test.tfrecords'), 5, 1)            # 48 x 64 images, 6 x 8 depth maps; batches 2, 2, 1
    base = model_args(model) + ['--batchsize', str(B), '--ckptdir', str(tmp / 'ck'), '--datadir', root, '--checkpoint', ckpt,
                                '--upsample', 'joint', '--clamp-lo=-1e30']
    plain = run(capsys, evaluate.main, base + ['nyu'])
    assert 'align' not in plain and not any(k.endswith('_aligned') for k in plain)      # the keys of today
    outputs = ('coarse', 'fine', 'fine_joint') if model == 'msdn' else ('unary', 'crf', 'crf_joint')
    assert all(o in plain for o in outputs)
    for resolution in ('grid', 'record'):
        ref = plain if resolution == 'grid' else run(capsys, evaluate.main, base + ['--resolution', 'record', 'nyu'])
        got = run(capsys, evaluate.main, base + ['--align', 'affine', '--resolution', resolution, 'nyu'])
        assert set(got) - set(ref) == {o + '_aligned' for o in outputs} | {'align'} and got['align'] == 'affine'
        for k in ref:                                                    # every other key: the same values, NaN included
            assert json.dumps(got[k], sort_keys=True) == json.dumps(ref[k], sort_keys=True), k
        for o in outputs:
            twin = got[o + '_aligned']
            assert set(twin) == METRICS | {'unaligned_images', 'mean_scale', 'mean_shift'}
            assert twin['images'] == 5 and twin['pixels'] + twin['nonfinite'] == ref[o]['pixels'] + ref[o]['nonfinite']
            assert 0 <= twin['unaligned_images'] <= 5
            print(f'{model} {resolution} {o}: rmse {ref[o]["rmse"]:.6g} -> {twin["rmse"]:.6g}, unaligned '
                  f'{twin["unaligned_images"]}, mean scale {twin["mean_scale"]:.6g} shift {twin["mean_shift"]:.6g}')
            # least squares minimises that sum over the same pixels; the margin covers three float32 roundings per term
            assert twin['rmse'] <= ref[o]['rmse'] * (1 + 1e-5), o
    for mode in ('median', 'scale'):
        got = run(capsys, evaluate.main, base + ['--align', mode, 'nyu'])
        assert got['align'] == mode and all(got[o + '_aligned']['images'] == 5 for o in outputs)
        ok = [o for o in outputs if got[o + '_aligned']['unaligned_images'] < 5]
        assert all(got[o + '_aligned']['mean_shift'] == 0 for o in ok)
    on_disk = json.load(open(os.path.join(str(tmp / 'ck'), model, f'eval-{got["global_step"]}.json')))
    assert on_disk['align'] == 'scale'
    if model == 'dcnf':                                                 # the two outputs of --condition have twins too
        got = run(capsys, evaluate.main, base + ['--align', 'affine', '--condition', '0.5', 'nyu'])
        for o in outputs + ('crf_cond', 'crf_hidden'):
            assert got[o + '_aligned']['images'] == 5 and got[o + '_aligned']['pixels'] == got[o]['pixels'], o
            assert got[o + '_aligned']['rmse'] <= got[o]['rmse'] * (1 + 1e-5), o


def holes(shape):
    band = np.zeros(shape, bool)
    band[shape[0] // 3:shape[0] // 3 + 2] = True                         # a band of rows nothing was measured in
    return band


def test_predict_align_to_measured_maps(setup, capsys):
    from ann3depth_amd import predict
    model, ckpt, paths, tmp = setup
    plain = run(capsys, predict.main, predict_args(model, ckpt, str(tmp / 'plain')) + paths)
    depth = [np.load(f['npy']) for f in plain['files']]
    assert all(np.isfinite(d).all() and (d > 0).all() for d in depth)
    # --- affine: DIR/<stem>.npy = 3 depth + 0.5 with holes
    to = tmp / 'to-affine'
    to.mkdir()
    for i, d in enumerate(depth):
        m = (np.float32(3) * d + np.float32(0.5)).astype(np.float32)
        m[holes(d.shape)] = np.nan
        np.save(str(to / f'img{i}.npy'), m)
    got = run(capsys, predict.main, predict_args(model, ckpt, str(tmp / 'affine')) +
              ['--align', 'affine', '--align-to', str(to)] + paths)
    assert set(got) - set(plain) == {'align', 'min_depth', 'max_depth'} and got['align'] == 'affine'
    assert (got['min_depth'], got['max_depth']) == (0.0, float('inf'))
    for i, (f, d) in enumerate(zip(got['files'], depth)):
        assert set(f) - set(plain['files'][i]) == {'scale', 'shift', 'measured', 'aligned'}
        with np.errstate(invalid='ignore'):
            measured = int((~holes(d.shape) & (np.float32(3) * d + np.float32(0.5) > 0)).sum())
        print(f'{model} img{i}: scale {f["scale"]!r} shift {f["shift"]!r} measured {f["measured"]} of {measured}')
        assert f['aligned'] is True and f['measured'] == measured
        assert f['scale'] == pytest.approx(3, rel=1e-4) and f['shift'] == pytest.approx(0.5, rel=1e-3, abs=1e-4)
        assert np.allclose(np.load(f['npy']), np.float32(3) * d + np.float32(0.5), rtol=1e-5)
    # --- median: DIR = 2 depth: the scale is 2 exactly wherever the median prediction is positive
    to = tmp / 'to-median'
    to.mkdir()
    for i, d in enumerate(depth):
        m = (np.float32(2) * d).astype(np.float32)
        m[holes(d.shape)] = np.nan
        np.save(str(to / f'img{i}.npy'), m)
    got = run(capsys, predict.main, predict_args(model, ckpt, str(tmp / 'median')) +
              ['--align', 'median', '--align-to', str(to)] + paths)
    for f, d in zip(got['files'], depth):
        assert (d > 0).all()
        assert f['measured'] == int((~holes(d.shape)).sum())
        assert f['aligned'] is True and f['scale'] == 2 and f['shift'] == 0      # med(2 p) = 2 med(p), exactly
        assert np.array_equal(np.load(f['npy']), np.float32(2) * d)


def test_predict_align_to_maps_of_another_size_and_without_a_measured_pixel(setup, capsys):
    from ann3depth_amd import predict
    model, ckpt, paths, tmp = setup
    plain = run(capsys, predict.main, predict_args(model, ckpt, str(tmp / 'plain-bilinear'), 'bilinear') + paths)
    to = tmp / 'to-sizes'
    to.mkdir()
    rng = np.random.default_rng(8)
    for i, shape in enumerate([(20, 30), (20, 30), (7, 9)]):
        m = rng.uniform(1, 5, shape).astype(np.float32)
        m[rng.random(shape) < 0.6] = np.nan                              # sparse
        if i == 1:
            m[:] = np.nan                                                # nothing measured
        np.save(str(to / f'img{i}.npy'), m)
    for mode in ('median', 'scale', 'affine'):
        got = run(capsys, predict.main, predict_args(model, ckpt, str(tmp / f'sizes-{mode}'), 'bilinear') +
                  ['--align', mode, '--align-to', str(to)] + paths)
        for i, (f, g) in enumerate(zip(got['files'], plain['files'])):
            d = np.load(f['npy'])
            assert d.shape == SIZES[i] and np.isfinite(d).all() and f['nonfinite'] == 0
            assert f['measured'] == int(np.isfinite(np.load(str(to / f'img{i}.npy'))).sum())
            if i == 1 or not f['aligned']:
                assert (f['scale'], f['shift']) == (1, 0)
                assert open(f['npy'], 'rb').read() == open(g['npy'], 'rb').read()      # written as it is
        assert got['files'][1]['aligned'] is False and got['files'][1]['measured'] == 0
