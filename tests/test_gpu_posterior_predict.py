"""`predict --uncertainty`, `predict --depths` and `evaluate --condition` end to end (include/a3d_posterior.h,
DCNFReplica.posterior), on checkpoints these tests save from replicas that took two train steps at batch 2: the fully
convolutional unary at --superpixel 20 and the patch form at 40."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
SIZES = [(48, 64), (48, 64), (30, 41)]                 # two of one size run as one batch, the third alone
FORMS = {'fcsp20': dict(unary='fcsp', superpixel=20), 'patch40': dict(unary='patch', superpixel=40)}
METRICS = {'abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'log10', 'rmse_si', 'delta1', 'delta2', 'delta3', 'pixels', 'images',
           'images_without_valid_pixels', 'nonfinite'}


@pytest.fixture(scope='module', params=list(FORMS))
def setup(request, tmp_path_factory):
    """(form, checkpoint path, replica holding its weights, image paths, their pixels, directory, superpixel args)."""
    from ann3depth_amd import models, png
    form = request.param
    tmp = tmp_path_factory.mktemp(form)
    rep = models.DCNFReplica(B, device='cuda:0', train_pairwise=True, **FORMS[form])
    rng = np.random.default_rng(31)
    for _ in range(2):
        img = torch.from_numpy(rng.random((B, 48, 64, 3)).astype(np.float32) - np.float32(.5)).cuda()
        dep = torch.from_numpy(rng.uniform(0.5, 1.5, (B, 6, 8, 1)).astype(np.float32)).cuda()
        rep.step(img, dep)
    torch.cuda.synchronize()
    ckpt = str(tmp / 'weights.pt')
    torch.save({k: v.detach().cpu() for k, v in rep.state_dict().items()}, ckpt)
    paths, pixels = [], []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        img[:, w // 2:] //= 3
        png.imsave(str(tmp / f'img{i}.png'), img)
        paths.append(str(tmp / f'img{i}.png')), pixels.append(img)
    return form, ckpt, rep, paths, pixels, tmp, ['--model', 'dcnf', '--superpixel', str(FORMS[form]['superpixel'])]


def block_means(d, sp, lo, hi):
    """float64 superpixel targets of a 240 x 320 map as the driver forms them: the validity-aware resize to the same size
    keeps a pixel iff it is measured (finite, lo < d <= hi) and its right, lower and lower-right neighbours (clamped at the
    border; they are taps of weight 0) are finite (include/a3d_valid.h); a superpixel is a target iff at least half of its
    pixels are kept, and its target is their mean.  NaN elsewhere."""
    H, W = d.shape
    fin = np.isfinite(d)
    r1, c1 = np.minimum(np.arange(H) + 1, H - 1), np.minimum(np.arange(W) + 1, W - 1)
    with np.errstate(invalid='ignore'):
        kept = fin & (d > lo) & (d <= hi) & fin[:, c1] & fin[r1, :] & fin[np.ix_(r1, c1)]
    rows, cols = H // sp, W // sp
    count = kept.reshape(rows, sp, cols, sp).sum(axis=(1, 3))
    total = np.where(kept, d, 0).astype(np.float64).reshape(rows, sp, cols, sp).sum(axis=(1, 3))
    return np.where(count >= 0.5 * sp * sp, total / np.maximum(count, 1), np.nan)


def run_predict(capsys, argv):
    from ann3depth_amd import predict
    capsys.readouterr()
    rc = predict.main(argv)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    return rc, (json.loads(lines[0]) if rc == 0 and len(lines) == 1 else None)


@pytest.mark.parametrize('mode', ['joint', 'none'])
def test_uncertainty_writes_sigma_beside_unchanged_depth_files(setup, mode, capsys):
    form, ckpt, rep, paths, pixels, tmp, sel = setup
    base = sel + ['--checkpoint', ckpt, '--batchsize', str(B), '--upsample', mode]
    plain_dir, out_dir = str(tmp / f'plain-{mode}'), str(tmp / f'sigma-{mode}')
    rc0, plain = run_predict(capsys, base + ['--out', plain_dir] + paths)
    rc1, res = run_predict(capsys, base + ['--uncertainty', '--out', out_dir] + paths)
    assert rc0 == 0 and rc1 == 0
    assert set(res) - set(plain) == {'uncertainty', 'conditioned', 'observed_fraction', 'rejected_systems'}
    assert res['uncertainty'] is True and res['conditioned'] is False and res['observed_fraction'] == 0
    assert not os.path.exists(os.path.join(plain_dir, 'img0-sigma.npy'))
    grid = (rep.rows, rep.cols)
    rejected = 0
    for i, (f, g) in enumerate(zip(res['files'], plain['files'])):
        for ext in ('npy', 'png'):                                       # the depth files: the same bytes
            assert open(f[ext], 'rb').read() == open(g[ext], 'rb').read(), (i, ext)
        sigma = np.load(f['sigma_npy'])
        assert os.path.basename(f['sigma_npy']) == f'img{i}-sigma.npy' and os.path.exists(f['sigma_png'])
        assert sigma.dtype == np.float32 and sigma.shape == (grid if mode == 'none' else SIZES[i])
        if np.isnan(sigma).all():                                        # a rejected system (possible at 40: r is not >= 0)
            rejected += 1
        else:
            assert np.isfinite(sigma).all() and (sigma > 0).all(), i
    assert res['rejected_systems'] == rejected
    if form == 'fcsp20':
        assert rejected == 0                                             # r >= 0 there: every A is positive definite
    print(f'predict --uncertainty {form} {mode}: rejected {rejected}, sigma of image 0 '
          f'{np.nanmin(np.load(res["files"][0]["sigma_npy"])):.4g} .. {np.nanmax(np.load(res["files"][0]["sigma_npy"])):.4g}')


def test_depths_conditions_the_field_on_the_measured_superpixels(setup, capsys):
    """A synthetic 240 x 320 map with a punched rectangle of whole superpixels: the measured superpixels come back as their
    block means, the holes are filled with finite values and carry a positive sigma."""
    form, ckpt, rep, paths, pixels, tmp, sel = setup
    sp, rows, cols = rep.sp, rep.rows, rep.cols
    ddir = str(tmp / 'measured')
    os.makedirs(ddir, exist_ok=True)
    rng = np.random.default_rng(5)
    maps, holes = [], []
    for i in range(len(paths)):
        d = rng.uniform(1.0, 3.0, (240, 320)).astype(np.float32)
        hole = np.zeros((rows, cols), bool)
        hole[rows // 3:rows // 3 + 2, cols // 4:cols // 4 + 3] = True
        fill = [np.nan, 0.0, 11.0][i]                                    # not finite, <= min, > max
        d[np.kron(hole, np.ones((sp, sp), bool))] = fill
        np.save(os.path.join(ddir, f'img{i}.npy'), d)
        maps.append(d), holes.append(hole)
    out_dir = str(tmp / 'completed')
    base = sel + ['--checkpoint', ckpt, '--batchsize', str(B), '--upsample', 'none', '--out', out_dir]
    rc, res = run_predict(capsys, base + ['--depths', ddir, '--min-depth', '0.5', '--max-depth', '10', '--uncertainty'] + paths)
    assert rc == 0
    assert res['conditioned'] is True and res['uncertainty'] is True and (res['min_depth'], res['max_depth']) == (0.5, 10.0)
    ok = 0
    for i, f in enumerate(res['files']):
        got, sigma = np.load(f['npy']), np.load(f['sigma_npy'])
        assert got.shape == (rows, cols) == sigma.shape
        if np.isnan(got).all():
            continue
        ok += 1
        means = block_means(maps[i], sp, 0.5, 10.0)
        assert (np.isfinite(means) == ~holes[i]).all()
        # a float32 sum of at most sp * sp positive values, in any order, and one division: (sp * sp) u relative
        np.testing.assert_allclose(got[~holes[i]], means[~holes[i]], rtol=sp * sp * 2.0 ** -24)
        assert (sigma[~holes[i]] == 0).all()
        assert np.isfinite(got[holes[i]]).all() and (sigma[holes[i]] > 0).all()
    assert ok == len(paths) - res['rejected_systems']
    assert res['observed_fraction'] == pytest.approx(1 - 6 / (rows * cols), abs=1e-12)
    if form == 'fcsp20':
        assert res['rejected_systems'] == 0
    rc, only = run_predict(capsys, base + ['--depths', ddir, '--min-depth', '0.5', '--max-depth', '10'] + paths)
    assert rc == 0 and only['uncertainty'] is False and 'sigma_npy' not in only['files'][0]


def test_refusals_exit_2(setup, capsys):
    from ann3depth_amd import predict
    form, ckpt, rep, paths, pixels, tmp, sel = setup
    base = sel + ['--checkpoint', ckpt, '--batchsize', str(B), '--out', str(tmp / 'never')]
    bad = str(tmp / 'bad')
    os.makedirs(bad, exist_ok=True)
    np.save(os.path.join(bad, 'img0.npy'), np.ones((24, 32), np.float32))
    np.save(os.path.join(bad, 'img1.npy'), np.ones((24, 32), np.float64))             # the wrong dtype
    capsys.readouterr()
    assert predict.main(base + ['--depths', bad] + paths[:2]) == 2
    assert 'img1.npy' in capsys.readouterr().err
    np.save(os.path.join(bad, 'img1.npy'), np.ones((24, 32, 1), np.float32))          # the wrong rank
    assert predict.main(base + ['--depths', bad] + paths[:2]) == 2
    assert 'img1.npy' in capsys.readouterr().err
    np.save(os.path.join(bad, 'img1.npy'), np.ones((24, 32), np.float32))
    assert predict.main(base + ['--depths', bad] + paths) == 2                         # img2.npy is missing
    assert 'img2.npy' in capsys.readouterr().err
    assert predict.main(base + ['--depths', bad, '--min-depth', '3', '--max-depth', '2'] + paths[:1]) == 2
    for flag in (['--uncertainty'], ['--depths', bad]):
        assert predict.main(['--model', 'msdn', '--checkpoint', ckpt, '--out', str(tmp / 'never')] + flag + paths[:1]) == 2
        assert 'dcnf' in capsys.readouterr().err
    assert not os.path.exists(str(tmp / 'never'))


def test_evaluate_condition(setup, capsys):
    from ann3depth_amd import evaluate, tfrecord
    form, ckpt, rep, paths, pixels, tmp, sel = setup
    root = str(tmp / 'data')
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    rng = np.random.default_rng(3)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'test.tfrecords')) as w:   # 5 records: batches 2, 2, 1
        for _ in range(5):
            w.write_example(rng.integers(0, 256, (48, 64, 3)).astype(np.float32) / np.float32(255) - np.float32(.5),
                            rng.uniform(0.5, 1.5, (6, 8, 1)).astype(np.float32))
    base = sel + ['--batchsize', str(B), '--ckptdir', str(tmp / 'ck'), '--datadir', root, '--checkpoint', ckpt]

    def run(extra):
        capsys.readouterr()
        assert evaluate.main(base + extra + ['nyu']) == 0
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    plain = run([])
    got = run(['--condition', '0.5', '--condition-seed', '7'])
    again = run(['--condition', '0.5', '--condition-seed', '7'])
    other = run(['--condition', '0.5', '--condition-seed', '8'])
    assert json.dumps(got, sort_keys=True) == json.dumps(again, sort_keys=True)
    assert set(got) - set(plain) == {'crf_cond', 'crf_hidden', 'condition_z2', 'hidden_fraction', 'rejected_systems',
                                     'condition', 'condition_seed'}
    for k in plain:                                                      # every other key: the same values, NaN included
        assert json.dumps(got[k], sort_keys=True) == json.dumps(plain[k], sort_keys=True), k
    assert set(got['crf_cond']) == set(got['crf_hidden']) == METRICS
    assert got['crf_cond']['pixels'] == got['crf_hidden']['pixels'] > 0
    accepted = 5 - got['rejected_systems']
    print(f'evaluate --condition {form}: hidden_fraction {got["hidden_fraction"]:.3f}, z2 {got["condition_z2"]:.4g}, rejected '
          f'{got["rejected_systems"]}, rmse cond {got["crf_cond"]["rmse"]:.4g} / hidden {got["crf_hidden"]["rmse"]:.4g}')
    if form == 'fcsp20':
        assert accepted == 5
    if accepted:
        # the share of `accepted * nsp` fair coins that came up hidden: within five standard deviations of one half
        assert abs(got['hidden_fraction'] - 0.5) <= 5 * 0.5 / np.sqrt(accepted * rep.nsp)
        assert np.isfinite(got['condition_z2']) and got['condition_z2'] > 0
        assert other['crf_cond']['pixels'] != got['crf_cond']['pixels'] or other['condition_z2'] != got['condition_z2']
    assert evaluate.main(base + ['--condition', '1.0', 'nyu']) == 2
    assert evaluate.main(base + ['--condition', '0.5', '--resolution', 'record', 'nyu']) == 2
    assert evaluate.main(['--model', 'msdn', '--condition', '0.5', 'nyu']) == 2
