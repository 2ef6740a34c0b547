"""`--segmentation slic` through the replica, the driver, checkpoints, evaluation and prediction (batch 2, --unary fcsp).
segmentation='grid' is held to a replica built without the argument bit for bit.  A slic step is held to the ops calls
composed by hand, bit for bit: the kernels themselves are held to float64 in tests/test_gpu_slic*.py, and everything after
them (the CRF, the unary backward, the descent) is the code tests/test_gpu_dcnf_superpixel.py holds."""
import json
import os

import numpy as np
import pytest
import torch

import fcsp_ref as F
import slic_ref as S
from oracle import dcnf as OD

pytestmark = pytest.mark.gpu
KERNEL, BIAS = OD.PAIR_PREFIX + 'kernel', OD.PAIR_PREFIX + 'bias'
# The rates of the descent test, both groups.  tests/test_gpu_dcnf_superpixel.py and tests/test_gpu_dcnf_valid_train.py
# measured that the reference's 0.1 overshoots from the first step on once the pairwise layer is live, and that 1e-3 descends
# at 6 x 8 and at 12 x 16 (S = 192).  The banded objective is a SUM over the S superpixels of an image, so its gradient wrt a
# shared weight grows with S; the rate that was stable at S = 192 is scaled by 192 / S beyond it: 1e-3 at 6 x 8, 2.5e-4 at
# 24 x 32.  The pairwise group takes the same rate: on the grid the reference's two similarities are essentially 0, so
# d loss / d kernel = sum over the pairs of dr * sims is next to nothing and only the bias moves; the paper's similarities
# lie in (0, 1], so here the kernel's gradient is a sum over all Q pairs (1320 at 24 x 32) and 0.1 moves the weights by O(10)
# a step.  Measured on this batch before the rates were scaled: pairwise at 0.1, unary at 1e-3: at 40 the loss fell at each
# of five steps (-4.64 ... -14.31, kernel 1 -> 2.25), at 10 it went -343.1, -958.1, -963.5, -850.8, 5291.2 while the kernel
# ran from 1 to 12.7; both at 1e-3: at 40 -4.640, -4.696, -4.751, -4.805, -4.860, at 10 -343.1, -369.5, -390.0, -290.6, 5838.7
# (kernel 1.43): the unary step itself overshoots at S = 768, and so does the GRID replica on the same batch at 1e-3 (-205.3,
# -241.2, -267.8, -152.7, 7060.0; at 2.5e-4 it falls at every step).  That the reference's rates are too large for finer grids
# and live similarities is a property of the rates, stated in DESIGN.md 3.5.3, not of the segmentation or its kernels.


def descent_lr(nsp):
    return 1e-3 * min(1.0, 192.0 / nsp)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def start_params(seed=3000):
    """The fcsp form's draw with a pairwise layer of ones: a live loss and a live dr."""
    params = F.init_params(seed)
    params.update(OD.pairwise_init(seed + 1))
    params[KERNEL], params[BIAS] = np.ones((2, 1), np.float32), np.ones((1,), np.float32)
    return params


def edge_images(B, seed):
    """[B, 480, 640, 3]: two flat regions of low contrast with a slanted border that ignores every grid, plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(480), np.arange(640), indexing='ij')
    out = np.empty((B, 480, 640, 3), np.float32)
    for b in range(B):
        side = (yy - 240) * rng.normal() + (xx - 320) * rng.normal() + rng.normal() * 50 > 0
        out[b] = np.where(side[..., None], 0.6, 0.4) + 0.1 * (rng.random((480, 640, 3)) - 0.5)
    return out


def batch(B, seed):
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(edge_images(B, seed)).cuda()
    dep = torch.from_numpy(rng.uniform(0.2, 1.0, (B, 55, 74, 1)).astype(np.float32)).cuda()
    return img, dep


@pytest.mark.parametrize('sp', [40, 20])
def test_grid_is_the_replica_without_the_argument_bit_for_bit(sp):
    from ann3depth_amd import models
    img, dep = batch(2, 23)
    kw = dict(unary='fcsp', train_pairwise=True, superpixel=sp, seed=4)
    a, b = models.DCNFReplica(2, segmentation='grid', slic_iters=9, slic_compactness=3.0, **kw), models.DCNFReplica(2, **kw)
    assert not a.slic and a.labels is None and a.unary.labels is None and not hasattr(a, 'centres')
    for _ in range(2):
        la, lb = a.step(img, dep)['mean_loss'], b.step(img, dep)['mean_loss']
        torch.cuda.synchronize()
        assert same_bits(la, lb) and same_bits(a.dz, b.dz) and same_bits(a.r, b.r) and same_bits(a.sims, b.sims)
        assert same_bits(a.unary.group.var, b.unary.group.var) and same_bits(a.pair_group.var, b.pair_group.var)
        assert same_bits(a.unary.group.grad, b.unary.group.grad) and same_bits(a.y, b.y)
    pa, pb = a.predict(img), b.predict(img)
    assert same_bits(pa[0], pb[0]) and same_bits(pa[1], pb[1])
    painted = a.depth_map(pa[1])                                               # the blocks, for a grid replica
    assert tuple(painted.shape) == (2, 240, 320)
    assert torch.equal(painted[:, ::sp, ::sp], pa[1]) and torch.equal(painted[:, sp - 1::sp, sp - 1::sp], pa[1])


@pytest.mark.parametrize('sp', [40, 10])
def test_a_slic_step_is_the_ops_composed_by_hand(sp):
    from ann3depth_amd import models, ops
    B = 2
    rep = models.DCNFReplica(B, params=start_params(), unary='fcsp', superpixel=sp, segmentation='slic', train_pairwise=True)
    assert rep.slic and rep.banded == (sp != 40) and (rep.slic_iters, rep.slic_compactness) == (5, 0.1)
    total = rep.nsp
    img, dep = batch(B, 40 + sp)
    kernel, bias = rep.pair_var('kernel').clone(), rep.pair_var('bias').clone()
    out = rep.step(img, dep)
    torch.cuda.synchronize()
    u = rep.unary
    labels, centres, count = ops.slic_segment(u.resized, sp, 5, 0.1)
    assert torch.equal(labels, rep.labels) and torch.equal(count, rep.label_count) and same_bits(centres, rep.centres)
    lab = labels.cpu().numpy()
    grid = S.grid_labels(B, 240, 320, sp)
    moved = (lab != grid).mean()
    print(f'slic step at {sp}: {100 * moved:.1f} % of the pixels left their block; counts {int(count.min())} .. {int(count.max())}')
    assert 0.01 < moved < 0.9 and S.counts_mask(lab, sp).all() and int(count.min()) > 0
    assert (count.sum(1) == 240 * 320).all()
    y, ycount = ops.label_mean(rep.depths240, sp, labels)
    assert same_bits(y, rep.y) and torch.equal(ycount, count)
    pooled = ops.label_pool_fwd(u.act['conv2d_4/pool'], u.map, labels, count)
    assert same_bits(pooled, u.act['pooled'].view(B, total, -1))
    assert not same_bits(pooled, ops.superpixel_pool_fwd(u.act['conv2d_4/pool'], u.map))
    mean3, _ = ops.label_mean(u.resized, sp, labels)
    hist = ops.label_hist(u.resized, sp, labels)
    sims, r = ops.label_pair_similarity(mean3, hist, count, rep.left, rep.right, kernel, bias, 1.0)
    assert same_bits(hist, rep.hist) and same_bits(sims, rep.sims) and same_bits(r, rep.r)
    assert float(sims.min()) > 0.05 and float(sims.max()) <= 1            # the paper's similarities are not "essentially 0"
    dflat = torch.full_like(u.dact['flat'], float('nan'))
    ops.label_pool_bwd(u.dact['pooled'].view(B, total, -1), u.map, labels, count, dflat)
    assert same_bits(dflat, u.dact['flat']) and torch.isfinite(dflat).all() and float(dflat.abs().max()) > 0
    assert rep.status.tolist() == [0, 0] and np.isfinite(float(out['mean_loss'])) and rep.global_step == 1
    assert float(rep.pair_group.var.min()) >= 0 and float(rep.pair_grad('kernel').abs().max()) > 0
    assert torch.isfinite(u.group.var).all() and float(u.group.grad.abs().max()) > 0
    # prediction: the grid-shaped outputs, painted by the labels of that forward
    unary, crf = rep.predict(img)
    assert tuple(unary.shape) == tuple(crf.shape) == (B, rep.rows, rep.cols) and torch.isfinite(crf).all()
    painted = rep.depth_map(crf)
    assert tuple(painted.shape) == (B, 240, 320)
    assert torch.equal(painted, torch.gather(crf.reshape(B, -1), 1, rep.labels.reshape(B, -1).long()).view(B, 240, 320))
    assert np.isfinite(float(rep.nll(dep, B)))
    with pytest.raises(ValueError, match='slic'):
        rep.posterior(img)
    with pytest.raises(ValueError, match='slic'):
        rep.nll(dep, B, valid_range=(0.0, 0.9))


@pytest.mark.parametrize('sp', [40, 10])
def test_the_loss_falls_on_a_fixed_batch(sp):
    from ann3depth_amd import models
    rep = models.DCNFReplica(2, params=start_params(), unary='fcsp', superpixel=sp, segmentation='slic', train_pairwise=True)
    rate = rep.unary.group.lr = rep.pair_group.lr = descent_lr(rep.nsp)
    img = torch.from_numpy(edge_images(2, 31)).cuda()
    z = rep.predict(img)[0].cpu().numpy()                                      # a target the step can approach: z plus noise
    y = (z + 0.05 * np.random.default_rng(32).standard_normal(z.shape)).astype(np.float32)
    dep = torch.from_numpy(np.ascontiguousarray(np.kron(y, np.ones((sp, sp), np.float32))[..., None])).cuda()
    losses = [float(rep.step(img, dep)['mean_loss']) for _ in range(5)]
    print(f'slic descent at {sp}, rate {rate}: losses {losses}, pairwise kernel '
          f'{rep.pair_var("kernel").reshape(-1).tolist()}, bias {float(rep.pair_var("bias"))}, status {rep.status.tolist()}')
    assert np.isfinite(losses).all() and (np.diff(losses) < 0).all() and not rep.status.any()
    assert float(rep.pair_group.var.min()) >= 0 and rep.global_step == 5


def test_checkpoints_cross_the_segmentations():
    from ann3depth_amd import models
    img, dep = batch(2, 60)
    for first, second in (('grid', 'slic'), ('slic', 'grid')):
        a = models.DCNFReplica(2, params=start_params(), unary='fcsp', superpixel=20, segmentation=first, train_pairwise=True)
        a.step(img, dep)
        b = models.DCNFReplica(2, seed=9, unary='fcsp', superpixel=20, segmentation=second)
        assert list(a.state_dict()) == list(b.state_dict())                    # names and order do not change
        assert all(v.shape == b.state_dict()[k].shape for k, v in a.state_dict().items())
        b.load_state_dict(a.state_dict())
        assert same_bits(a.unary.group.var, b.unary.group.var) and same_bits(a.pair_group.var, b.pair_group.var)
        assert b.global_step == 1
        unary, crf = b.predict(img)
        assert torch.isfinite(crf).all() and b.status.tolist() == [0, 0] and np.isfinite(float(b.nll(dep, 2)))


def test_refusals():
    from ann3depth_amd import ann3depth, models
    with pytest.raises(ValueError, match='--unary fcsp'):
        models.DCNFReplica(2, segmentation='slic')
    with pytest.raises(ValueError, match='--unary fcsp'):
        models.DCNFReplica(2, segmentation='slic', unary='patch')
    with pytest.raises(ValueError, match='--pairwise-texture'):
        models.DCNFReplica(2, segmentation='slic', unary='fcsp', pairwise_texture=True)
    with pytest.raises(ValueError, match='--min-depth / --max-depth'):
        models.DCNFReplica(2, segmentation='slic', unary='fcsp', valid_range=(0.0, 0.9))
    with pytest.raises(ValueError, match='--segmentation'):
        models.DCNFReplica(2, segmentation='watershed', unary='fcsp')
    with pytest.raises(ValueError, match='--slic-iters'):
        models.DCNFReplica(2, segmentation='slic', unary='fcsp', slic_iters=-1)
    with pytest.raises(ValueError, match='--slic-compactness'):
        models.DCNFReplica(2, segmentation='slic', unary='fcsp', slic_compactness=float('nan'))
    models.check_dcnf_segmentation('grid', 'patch', True, (0.0, 0.9))             # today's forms stay
    with pytest.raises(SystemExit):
        ann3depth.parse_args(['nyu', '--model', 'dcnf', '--segmentation', 'watershed'])


def _write_records(path, count, seed):
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(48), np.arange(64), indexing='ij')
    with tfrecord.TFRecordWriter(path) as w:
        for _ in range(count):
            side = (yy - 24) * rng.normal() + (xx - 32) * rng.normal() > 0
            img = np.where(side[..., None], 0.65, 0.35) + 0.1 * (rng.random((48, 64, 3)) - 0.5)
            w.write_example(img.astype(np.float32), rng.uniform(0.2, 1.0, (6, 8, 1)).astype(np.float32))


def test_driver_evaluate_and_predict(tmp_path, capsys):
    from ann3depth_amd import ann3depth, evaluate, models, png, predict
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'nyu'))
    _write_records(os.path.join(root, 'nyu', 'train.tfrecords'), 8, 1)
    _write_records(os.path.join(root, 'nyu', 'test.tfrecords'), 4, 2)
    ck = str(tmp_path / 'ckpt')
    common = ['nyu', '--steps', '2', '--batchsize', '2', '--datadir', root, '--ckptdir', ck, '--sumfreq', '1', '--ckptfreq', '0']
    slic = ['--model', 'dcnf', '--segmentation', 'slic']
    try:
        # refused before anything is set up: msdn, the patch form, texture, holes, a bad parameter
        assert ann3depth.main(common + ['--model', 'msdn', '--segmentation', 'slic']) == 2
        assert ann3depth.main(common + slic) == 2
        assert ann3depth.main(common + slic + ['--unary', 'fcsp', '--pairwise-texture']) == 2
        assert ann3depth.main(common + slic + ['--unary', 'fcsp', '--min-depth', '0.1', '--max-depth', '0.9']) == 2
        assert ann3depth.main(common + slic + ['--unary', 'fcsp', '--slic-iters', '-2']) == 2
        assert not os.path.exists(ck)
        assert ann3depth.main(common + slic + ['--unary', 'fcsp', '--superpixel', '20', '--id', 'slic']) == 0
        assert (models.dcnf.segmentation, models.dcnf.slic_iters, models.dcnf.slic_compactness) == ('slic', 5, 0.1)
        assert ann3depth.main(common + ['--model', 'dcnf', '--unary', 'fcsp', '--steps', '1', '--id', 'grid']) == 0
        assert models.dcnf.segmentation == 'grid'
        assert ann3depth.main(common + ['--model', 'dcnf', '--steps', '1', '--id', 'patch']) == 0
    finally:
        models.dcnf.unary, models.dcnf.superpixel, models.dcnf.train_pairwise = 'patch', 40, False
        models.dcnf.segmentation, models.dcnf.slic_iters, models.dcnf.slic_compactness = 'grid', 5, 0.1
    capsys.readouterr()
    recs = [json.loads(l) for l in open(os.path.join(ck, 'dcnf_slic', 'summaries.jsonl'))]
    assert [r['global_step'] for r in recs] == [1, 2] and all(np.isfinite(r['loss/mean_loss']) for r in recs)
    for run in ('slic', 'grid'):
        state, _ = ann3depth.read_checkpoint(ann3depth.latest_checkpoint(os.path.join(ck, 'dcnf_' + run)), 'cpu')
        worst = max(float(v.abs().max()) for k, v in state.items() if k != 'global_step')
        with capsys.disabled():
            print(f'{run} checkpoint: step {int(state["global_step"])}, largest weight {worst:.3g}; losses '
                  f'{[r["loss/mean_loss"] for r in recs] if run == "slic" else "-"}')
        assert np.isfinite(worst)
    base = ['--model', 'dcnf', '--batchsize', '2', '--ckptdir', ck, '--datadir', root]
    reports = {}
    for run in ('slic', 'grid'):
        for seg, sp in (('slic', 20), ('grid', 20), ('slic', 40)):
            flags = ['--segmentation', seg] if seg != 'grid' else []
            assert evaluate.main(base + flags + ['--id', run, '--superpixel', str(sp), 'nyu']) == 0
            got = reports[run, seg, sp] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
            with capsys.disabled():
                print(f'evaluate {run} checkpoint, {seg} at {sp}: crf_nll {got["crf_nll"]}, singular {got["singular_systems"]}, '
                      f'unary rmse {got["unary"]["rmse"]}, crf rmse {got["crf"]["rmse"]}')
            assert got['superpixel'] == sp and got['unary_form'] == 'fcsp' and got['records'] == 4
            assert got.get('segmentation', 'grid') == seg and ('slic_iters' in got) == (seg == 'slic')
            assert np.isfinite(got['crf_nll']) and got['singular_systems'] == 0
            for o in ('unary', 'crf'):
                assert got[o]['pixels'] == 4 * 240 * 320 and all(np.isfinite(v) for v in got[o].values())
    assert evaluate.main(base + ['--id', 'slic', '--superpixel', '20', '--segmentation', 'slic', '--slic-iters', '0', 'nyu']) == 0
    # no iteration: the grid's superpixels.  z is the grid's bits (the pooling), y the same means in another order of
    # summation, so the float32 likelihood agrees far inside 1e-3 of its size.  (The rmse figures are not compared: two
    # steps at the reference's rate on random targets can leave a network whose output is one constant, which every
    # segmentation paints alike.)
    zero, grid = json.loads(capsys.readouterr().out.strip().splitlines()[-1]), reports['slic', 'grid', 20]
    assert zero['slic_iters'] == 0 and abs(zero['crf_nll'] - grid['crf_nll']) <= 1e-3 * max(1.0, abs(grid['crf_nll']))
    # what evaluation refuses under slic, each with its flag in the message and before any GPU work
    for flags, word in ((['--upsample', 'joint'], '--upsample joint'), (['--observed-nll'], '--observed-nll'),
                        (['--condition', '0.5'], '--condition'), (['--slic-compactness', '-1'], '--slic-compactness')):
        assert evaluate.main(base + ['--id', 'slic', '--segmentation', 'slic'] + flags + ['nyu']) == 2
        assert word in capsys.readouterr().err
    assert evaluate.main(base + ['--id', 'patch', '--segmentation', 'slic', 'nyu']) == 2
    assert '--unary fcsp' in capsys.readouterr().err
    assert evaluate.main(['--model', 'msdn', '--segmentation', 'slic', '--ckptdir', ck, '--datadir', root, 'nyu']) == 2
    assert 'no superpixels' in capsys.readouterr().err
    # prediction: painted by the labels, then --upsample
    rng = np.random.default_rng(7)
    paths = []
    for k in range(2):
        side = np.add.outer(np.arange(60) * (k + 1), -np.arange(80)) > 0
        pix = np.where(side[..., None], 170, 80) + rng.integers(-12, 13, (60, 80, 3))
        paths.append(str(tmp_path / f'im{k}.png'))
        png.imsave(paths[-1], pix.astype(np.uint8))
    pbase = ['--model', 'dcnf', '--ckptdir', ck, '--id', 'slic', '--batchsize', '2', '--segmentation', 'slic']
    for sp, total in ((20, 192), (40, 48)):
        out = str(tmp_path / f'out{sp}')
        assert predict.main(pbase + ['--superpixel', str(sp), '--upsample', 'none', '--out', out] + paths) == 0
        got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert got['segmentation'] == 'slic' and got['superpixel'] == sp and got['nonfinite'] == 0
        for f in got['files']:
            d = np.load(f['npy'])
            assert d.shape == (240, 320) and f['size'] == [240, 320] and np.unique(d).size <= total
    out = str(tmp_path / 'out-bilinear')
    assert predict.main(pbase + ['--superpixel', '20', '--upsample', 'bilinear', '--out', out] + paths) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert all(np.load(f['npy']).shape == (60, 80) for f in got['files']) and got['nonfinite'] == 0
    for flags, word in (([], '--upsample joint'), (['--upsample', 'none', '--uncertainty'], '--uncertainty'),
                        (['--upsample', 'none', '--depths', str(tmp_path)], '--depths')):
        assert predict.main(pbase + flags + ['--out', str(tmp_path / 'refused')] + paths) == 2
        assert word in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / 'refused'))
    assert predict.main(['--model', 'msdn', '--segmentation', 'slic', '--ckptdir', ck, '--out', out] + paths) == 2
    assert 'no superpixels' in capsys.readouterr().err
