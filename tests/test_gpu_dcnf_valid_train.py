"""models.DCNFReplica(valid_range=...) and `--model dcnf --min-depth / --max-depth` on the GPU: one step on a batch with
holes against the float64 likelihood of the observed superpixels (tests/crf_observed_ref.py) evaluated on the z and r
read back from the replica; the pairwise layer learning on such a batch; valid_range=None leaving every bit where it
was; two ranks against one rank on the concatenated batch; the driver, a checkpoint and `evaluate --observed-nll`.
Batch 2.  The objective has no epsilon: an untrained network against a random target does not saturate it."""
import json
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_loss_ref as L
import crf_observed_ref as V
import dcnf_pair_ref as P
from oracle import dcnf as OD

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
KERNEL, BIAS = OD.PAIR_PREFIX + 'kernel', OD.PAIR_PREFIX + 'bias'
RANGE = (0.0, 0.99)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def start_params(w=(1.0, 1.0), b=1.0):
    params = OD.init_params(3000)
    params[KERNEL], params[BIAS] = np.array(w, F).reshape(2, 1), np.array([b], F)
    return params


def holed_batch(B, seed):
    """(images [B, 240, 320, 3], depths [B, 55, 74, 1]) float32 on the host: dcnf_pair_ref's images (similarities inside
    (0, 1) in the first two, so that the pairwise layer has a gradient); depths in [0.05, 0.95] with the range cap
    1.0 over the upper 22 rows (two rows of superpixels and 16 of the 40 pixel rows of the third, which the zeros then
    leave near one half measured) and 6 % zeros, another pattern in every image."""
    rng = np.random.default_rng(seed)
    img = P.image(240, 320, 40, B, seed=seed)
    dep = (0.05 + 0.9 * rng.random((B, 55, 74, 1))).astype(F)
    dep[:, :22] = F(1.0)
    dep[rng.random(dep.shape) < 0.06] = F(0.0)
    return img, dep


def near_batch(rep, B, seed):
    """As tests/test_gpu_dcnf_pairwise_train.py's batch_for: a target at 240 x 320 whose superpixel means are the replica's
    own z plus noise of 0.05, here with holes in it: 100.0, beyond the range (-10, 10) this batch goes with, over the upper
    96 pixel rows and in 40 blocks of 12 x 12 pixels."""
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(P.image(240, 320, 40, B, seed=seed)).cuda()
    rep.unary.forward(img)
    z = rep.unary.z.view(B, rep.rows, rep.cols).cpu().numpy()
    assert np.abs(z).max() < 9
    y = (z + 0.05 * rng.standard_normal(z.shape)).astype(F)
    dep = np.kron(y, np.ones((40, 40), F))[..., None].copy()
    dep[:, :96] = F(100.0)
    for b in range(B):
        for _ in range(40):
            r0, c0 = rng.integers(96, 228), rng.integers(0, 308)
            dep[b, r0:r0 + 12, c0:c0 + 12] = F(100.0)
    return img, torch.from_numpy(dep).cuda()


def cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def host_reference(rep):
    """nll64 and nll32 on what the replica holds: z, y (NaN = no target) and r, read back."""
    B = rep.B
    z, y, r = (t.cpu().numpy() for t in (rep.unary.z.view(B, 48), rep.y.view(B, 48), rep.r))
    pairs = L.pairs(6, 8)
    return z, y, r, V.nll64(z, y, r, *pairs), V.nll32(z, y, r, *pairs)


def test_one_step_on_a_batch_with_holes_matches_float64():
    from ann3depth_amd import models
    B = 2
    params = OD.init_params(3000)
    params.update(OD.pairwise_init(3001))
    rep = models.DCNFReplica(B, params=params, valid_range=RANGE)
    assert rep.min_count == 800
    img, dep = holed_batch(B, 21)
    before = {n: rep.unary.group.view(rep.unary.group.var, n).clone() for n in rep.unary.shapes}
    out = rep.step(*cuda(img, dep))
    torch.cuda.synchronize()
    assert rep.global_step == 1 and rep.dr is None
    # the targets: the mean of the finite pixels of the resized map, NaN below 800 of them
    d240 = rep.depths240.cpu().numpy()
    y64, c64 = V.superpixel_mean_valid64(d240, 40, 800)
    z, y, r, ref, res = host_reference(rep)
    count, nobs = rep.count.cpu().numpy(), rep.nobs.cpu().numpy()
    np.testing.assert_array_equal(count, c64)
    np.testing.assert_array_equal(np.isnan(y), np.isnan(y64))
    obs = ~np.isnan(y64)
    assert (np.abs(y[obs] - y64[obs]) <= 1601 * L.U * np.abs(y64[obs])).all()      # a float32 sum of <= 1600 positive terms
    print(f'dcnf holes step: observed {nobs} of 48, counts {np.unique(count)[:4]} .. {count.max()}')
    assert (nobs == obs.sum(axis=1)).all() and (nobs > 8).all() and (nobs < 40).all()
    assert ((count > 0) & (count < 800)).any() and ((count >= 800) & (count < 1600)).any()
    assert (count[:, :16] == 0).all()                                                # the band at the cap
    assert (rep.status_observed.cpu().numpy() == 0).all()
    # loss and dz: within 8 x the float32 restatement's error on these very inputs
    got = (rep.loss_per_image.cpu().numpy(), rep.dz.cpu().numpy(), None)
    e, e32 = V.errors(got, ref), V.errors((res['per'], res['dz'], None), ref)
    print(f'dcnf holes step: losses {got[0]} (float64 {ref["per"]}), loss {e[0].max():.3g} (restatement {e32[0].max():.3g}), '
          f'dz {e[1].max():.3g} (restatement {e32[1].max():.3g})')
    assert e[0].max() <= 8 * e32[0].max() and e[1].max() <= 8 * e32[1].max()
    assert abs(float(out['mean_loss']) - ref['mean']) <= 8 * e32[0].max() * ref['scale'].max() + 16 * L.U * abs(ref['mean'])
    assert np.abs(ref['dz'][~obs]).max() > 1e-4                  # an unobserved superpixel's z still moves: it is integrated out
    # the unary gradient: unary.backward of the reference's dz, at the tolerance of tests/test_gpu_dcnf.py's step test
    a_gpu = rep.unary.activations()
    a_gpu['flat'] = a_gpu['conv2d_4/pool'].reshape(48 * B, -1)
    g = OD.unary_backward(params, a_gpu, ref['dz'].astype(F).reshape(48 * B, 1))
    for n, gref in g.items():
        ggpu = rep.unary.group.view(rep.unary.group.grad, n)
        if np.linalg.norm(gref) > 0:
            assert rel(ggpu.cpu().numpy(), gref) < 1e-4, n
        np.testing.assert_array_equal(rep.unary.group.view(rep.unary.group.var, n).cpu().numpy(),
                                      (before[n] - np.float32(0.1) * ggpu).cpu().numpy())
    np.testing.assert_array_equal(rep.pair_var('kernel').cpu().numpy(), params[KERNEL])       # no gradient without the flag
    # summaries
    rec = rep.summary_scalars(out)
    assert rec['loss/observed_fraction'] == nobs.sum() / 96 and 0 < rec['loss/observed_fraction'] < 1
    target = dict((t, x) for t, x, _ in rep.summary_images())['summaries/Target'].cpu().numpy()
    assert target.shape == (1, 240, 320, 1) and np.isfinite(target).all()
    np.testing.assert_array_equal(target == 0, np.isnan(d240[:1]) | (d240[:1] == 0))
    # nll(): the same objective from the z and r that stand in the buffers
    again = rep.nll(cuda(dep)[0], B)
    assert bits(again.cpu().numpy()) == bits(out['mean_loss'].cpu().numpy())


def test_the_pairwise_layer_learns_on_a_batch_with_holes_and_stays_nonnegative():
    """Six steps of both groups on one batch (near_batch): the loss descends, the layer moves against float64's dr at the
    first step and never leaves kernel, bias >= 0.  The pairwise group steps at its rate 0.1; the unary group's rate is
    lowered to 1e-3 for this test.  The reference's 0.1 was chosen under a loss whose epsilons saturate it, so that next
    to no gradient reaches the network; this objective has none, its curvature in z alone is 2 lambda_max(A) / B (A_ii =
    1 + sum r up to 13 here), and at 0.1 the whole step overshoots from the first step on: measured on this batch
    -1.19, 16.6, 2.6e4, 1.2e6, ...; against the random target of holed_batch(2, 5) 10.4, 1.8e4, 6.8e7, ..."""
    from ann3depth_amd import models
    import crf_pair_grad_ref as G
    rep = models.DCNFReplica(2, params=start_params(), train_pairwise=True, valid_range=(-10.0, 10.0))
    rep.unary.group.lr = 1e-3
    img, dep = near_batch(rep, 2, 5)
    losses = []
    for it in range(6):
        out = rep.step(img, dep)
        losses.append(float(out['mean_loss']))
        if it == 0:
            z, y, r, ref, res = host_reference(rep)
            dr = rep.dr.cpu().numpy()
            e, e32 = V.errors((res['per'], res['dz'], dr), ref)[2], V.errors(res, ref)[2]
            dw64, db64 = G.dense_bwd64(rep.sims.cpu().numpy(), ref['dr'])
            gw, gb = rep.pair_grad('kernel').cpu().numpy().reshape(2), float(rep.pair_grad('bias'))
            scale_w = np.einsum('bq,bqk->k', np.abs(ref['dr']), rep.sims.cpu().numpy().astype(np.float64))
            nobs = rep.nobs.cpu().numpy()
            assert (nobs > 8).all() and (nobs < 40).all()
            print(f'dcnf holes pairwise: observed {nobs}, dr {e.max():.3g} (restatement {e32.max():.3g}), dw {gw} (float64 {dw64}), db {gb} ({db64})')
            assert e.max() <= 8 * e32.max()
            tol = 8 * e32.max() * np.abs(ref['dr']).max(axis=1).sum() * 48 + 97 * L.U * scale_w      # dr's bound, then the sum's
            assert (np.abs(gw - dw64) <= tol).all() and (np.abs(dw64) > 10 * tol).all()      # a gradient the bound can see
        var = rep.pair_group.var.cpu().numpy()
        assert (var >= 0).all() and np.isfinite(var).all()
    print(f'dcnf holes pairwise: losses {losses}, kernel {rep.pair_var("kernel").reshape(-1).tolist()}, bias {float(rep.pair_var("bias"))}')
    assert np.isfinite(losses).all() and (np.diff(losses) < 0).all()
    assert not np.array_equal(rep.pair_var('kernel').cpu().numpy(), start_params()[KERNEL])


def test_without_a_range_nothing_differs():
    """valid_range=None against a replica built without the argument, two steps: the same bits everywhere, no new buffer."""
    from ann3depth_amd import models
    params = start_params(w=(0.5, 0.25), b=0.125)
    a, b = models.DCNFReplica(2, params=params, valid_range=None, min_valid=0.9), models.DCNFReplica(2, params=params)
    img, dep = cuda(*holed_batch(2, 9))
    for _ in range(2):
        oa, ob = a.step(img, dep), b.step(img, dep)
    torch.cuda.synchronize()
    for x, y in ((oa['mean_loss'], ob['mean_loss']), (a.dz, b.dz), (a.r, b.r), (a.y, b.y), (a.depths240, b.depths240),
                 (a.unary.group.var, b.unary.group.var), (a.unary.group.grad, b.unary.group.grad), (a.pair_group.var, b.pair_group.var)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a.t_one is None and a.count is None and a.nobs is None and a.valid_range is None
    assert set(a.summary_scalars(oa)) == {'loss/mean_loss'}
    assert a.summary_images()[2][1] is a.depths240
    with pytest.raises(ValueError, match='min_depth <= max_depth'):
        models.DCNFReplica(2, params=params, valid_range=(1.0, 0.5))
    with pytest.raises(ValueError, match='min_valid'):
        models.DCNFReplica(2, params=params, valid_range=RANGE, min_valid=1.5)


def test_two_ranks_equal_one_rank_on_the_concatenated_batch(tmp_path):
    """tests/dcnf_valid_dp_worker.py: two ranks on the one GPU over gloo."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'dcnf_valid_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'


def test_the_driver_trains_dcnf_on_a_shard_with_holes_and_evaluate_reports_the_objective(tmp_path):
    """Eight tiny records (48 x 64 images, 6 x 8 depth maps: one stored depth per superpixel corner) whose upper two rows
    are at the cap and which hold one zero: two steps, a checkpoint, then the held-out objective from it."""
    from ann3depth_amd import ann3depth, evaluate, models, tfrecord
    rng = np.random.default_rng(1)
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'nyu'))
    for split in ('train', 'test'):
        with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', f'{split}.tfrecords')) as w:
            for i in range(8 if split == 'train' else 4):
                dep = (0.05 + 0.9 * rng.random((6, 8, 1))).astype(F)
                dep[:2] = F(1.0)
                dep[4, 2 + i % 4] = F(0.0)
                w.write_example(rng.random((48, 64, 3)).astype(F) - F(0.5), dep - F(0.5))      # the loader adds 0.5
    ck = str(tmp_path / 'ckpt')
    flags = ['--min-depth', '0', '--max-depth', '0.99']
    try:
        rc = ann3depth.main(['nyu', '--model', 'dcnf', '--steps', '2', '--batchsize', '2', '--datadir', root, '--ckptdir', ck,
                             '--sumfreq', '1', '--ckptfreq', '0', *flags])
        assert rc == 0 and models.dcnf.valid_range == RANGE
    finally:
        models.dcnf.valid_range = None
        for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
            signal.signal(s, signal.SIG_DFL)
    d = os.path.join(ck, 'dcnf')
    recs = [json.loads(l) for l in open(os.path.join(d, 'summaries.jsonl'))]
    print(f'driver: {recs}')
    assert [r['global_step'] for r in recs] == [1, 2] and all(np.isfinite(r['loss/mean_loss']) for r in recs)
    # rows 0 and 1 at the cap take superpixel rows 0 and 1; the zero takes the four superpixels around it: 28 of 48 stay
    assert all(r['loss/observed_fraction'] == 28 / 48 for r in recs)
    assert os.path.exists(os.path.join(d, 'model.ckpt-2.pt'))
    common = ['nyu', '--model', 'dcnf', '--batchsize', '2', '--datadir', root, '--ckptdir', ck, *flags]
    assert evaluate.main(common) == 0
    plain = json.load(open(os.path.join(d, 'eval-2.json')))
    assert evaluate.main(common + ['--observed-nll']) == 0
    res = json.load(open(os.path.join(d, 'eval-2.json')))
    print(f'evaluate --observed-nll: {res}')
    assert 'observed_nll' not in plain and 'observed_fraction' not in plain
    assert {k: v for k, v in res.items() if k not in ('observed_nll', 'observed_fraction')} == plain
    assert res['records'] == 4 and res['global_step'] == 2 and np.isfinite(res['observed_nll'])
    assert res['observed_fraction'] == 28 / 48
    assert evaluate.main(['nyu', '--model', 'msdn', '--datadir', root, '--ckptdir', ck, '--observed-nll']) == 2
