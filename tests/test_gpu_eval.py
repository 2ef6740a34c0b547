"""Evaluation on the GPU: a3d_depth_metrics against the float64 numpy reference of tests/test_eval_cpu.py (sampling of
the prediction at the target's resolution included), MSDNReplica.predict against forward() and the oracle, and the
evaluation driver end to end on a checkpoint `make train` wrote."""
import json
import os

import numpy as np
import pytest
import torch

import bf16s_tol
from oracle import msdn as O
from oracle import tf13_ops as T
from test_eval_cpu import COLS, ref_rows

pytestmark = pytest.mark.gpu

EXACT = [0, 7, 8, 9, 10]                    # counts: n, the three deltas, non-finite
CONT = [1, 2, 3, 4, 5, 6]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _pred(rng, n, h, w):
    """Depth-like predictions with every awkward value: negatives, zeros, NaN, +-inf, values under the clamp."""
    p = rng.uniform(0.05, 8, (n, h, w)).astype(np.float32)
    flat = p.reshape(-1)
    idx = rng.permutation(flat.size)
    k = max(1, flat.size // 40)
    flat[idx[:k]] = -rng.uniform(0, 3, k)
    flat[idx[k:2 * k]] = 0
    flat[idx[2 * k:2 * k + 3]] = np.nan
    flat[idx[2 * k + 3:2 * k + 5]] = np.inf
    flat[idx[2 * k + 5:2 * k + 7]] = -np.inf
    flat[idx[2 * k + 7:3 * k + 7]] = rng.uniform(0, 1e-3, k)
    return p


def _target(rng, n, h, w, u8):
    if u8:
        k = rng.integers(0, 256, (n, h, w)).astype(np.uint8)           # k = 0: target 0, not valid
        from ann3depth_amd import data
        return k, data.expand_u8(k)
    t = rng.uniform(0.1, 9, (n, h, w)).astype(np.float32)
    flat = t.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:flat.size // 30]] = 0
    flat[idx[flat.size // 30:flat.size // 30 + 4]] = np.nan
    flat[idx[flat.size // 30 + 4:flat.size // 30 + 6]] = np.inf
    return t, t


def _check_rows(got, want, scale):
    np.testing.assert_array_equal(got[:, EXACT], want[:, EXACT])
    err = np.abs(got[:, CONT] - want[:, CONT])
    assert (err <= 1e-5 * scale[:, CONT] + 1e-30).all(), (err / np.maximum(scale[:, CONT], 1e-30)).max()


@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('th,tw', [(55, 74), (55, 73), (6, 8), (480, 640)])
def test_depth_metrics_against_the_float64_reference(th, tw, u8):
    from ann3depth_amd import ops
    rng = np.random.default_rng(th * 1000 + tw + u8)
    n, alloc = 3, 5
    pred = _pred(rng, alloc, 55, 74)
    stored, tf32 = _target(rng, alloc, th, tw, u8)
    pred[0, 0, 0] = np.nan                                             # sampled as is at target pixel (0, 0) ...
    stored[0, 0, 0] = 128 if u8 else 2.0                               # ... which is valid
    if u8:
        from ann3depth_amd import data
        tf32 = data.expand_u8(stored)
    guard = np.float64(-7.25)
    big = torch.full((alloc + 2, len(COLS)), guard, dtype=torch.float64, device='cuda')
    rows = big[1:1 + alloc]                                            # one guard row on each side
    kw = dict(min_depth=0.0, max_depth=8.5)
    ops.depth_metrics(dev(pred[:n]), dev(stored[:n]), rows=rows, **kw)
    first = big.clone()
    ops.depth_metrics(dev(pred[:n]), dev(stored[:n]), rows=rows, **kw)
    torch.cuda.synchronize()
    assert torch.equal(first, big)                                     # the same bits on every run
    out = big.cpu().numpy()
    assert (out[0] == guard).all() and (out[1 + n:] == guard).all()    # rows past n and the guards untouched
    sampled = pred[:n] if (th, tw) == (55, 74) else T.resize_bilinear_tf1(pred[:n, :, :, None], th, tw)[..., 0]
    want = ref_rows(sampled, tf32[:n], **kw)
    _check_rows(out[1:1 + n], want, ref_rows(sampled, tf32[:n], magnitude=True, **kw))
    assert want[:, 10].sum() > 0 and want[:, 0].min() > 0              # the case exercises non-finite predictions


@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('th,tw', [(55, 73), (6, 8), (480, 640), (110, 148)])
def test_record_resolution_is_grid_mode_on_the_resized_prediction(th, tw, u8):
    """In-kernel sampling == a3d_resize_bilinear_tf1 at the target's size followed by a 1:1 comparison, bit for bit."""
    from ann3depth_amd import ops
    rng = np.random.default_rng(th + tw)
    pred = dev(_pred(rng, 4, 55, 74))
    stored, _ = _target(rng, 4, th, tw, u8)
    tgt = dev(stored)
    resized = torch.empty((4, th, tw, 1), device='cuda')
    ops.resize_bilinear_tf1(pred.view(4, 55, 74, 1), resized)
    a = ops.depth_metrics(pred, tgt)
    b = ops.depth_metrics(resized, tgt)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- predict
@pytest.fixture(scope='module')
def batch():
    rng = np.random.default_rng(1000)
    B = 2
    img = (rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)
    dep = (rng.integers(0, 256, (B, 480, 640, 1)) / 255).astype(np.float32)
    params = O.init_params(3000)
    a = O.forward(params, img, dep, None)
    return img, dep, params, a


def test_predict_is_the_phase3_forward_and_matches_the_oracle(batch):
    from ann3depth_amd import models
    img, dep, params, a = batch
    net = models.MSDNReplica(2, device='cuda:0', params=params)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    grads = [g.grad.clone() for g in net.groups.values()]
    coarse, fine = net.predict(dev(img))
    coarse, fine = coarse.clone(), fine.clone()
    assert coarse.shape == (2, 55, 74) and fine.shape == (2, 55, 74)
    net.forward(dev(img), dev(dep), None, phase=3)
    torch.cuda.synchronize()
    assert torch.equal(coarse, net.coarse.view(2, 55, 74)) and torch.equal(fine, net.fine.view(2, 55, 74))
    assert rel(coarse.cpu().numpy(), a['coarse'][..., 0]) < 1e-3
    assert rel(fine.cpu().numpy(), a['fine'][..., 0]) < 1e-3
    after = net.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(torch.equal(g0, g.grad) for g0, g in zip(grads, net.groups.values()))
    assert net.global_step == 0
    # a short batch runs zero-padded at the replica's B: its rows are those of the full batch
    c1, f1 = net.predict(dev(img[:1]), n=1)
    torch.cuda.synchronize()
    assert torch.equal(c1[:1], coarse[:1]) and torch.equal(f1[:1], fine[:1])
    c1, f1 = net.predict(dev(img), n=1)                                 # rows >= n of the input are not read
    torch.cuda.synchronize()
    assert torch.equal(f1[:1], fine[:1])


def test_predict_from_uint8_images_matches_float32():
    from ann3depth_amd import data, models
    rng = np.random.default_rng(4)
    k = rng.integers(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    net = models.MSDNReplica(2, device='cuda:0')
    c8, f8 = (t.clone() for t in net.predict(dev(k)))
    c32, f32 = net.predict(dev(data.expand_u8(k)))
    torch.cuda.synchronize()
    assert torch.equal(c8, c32) and torch.equal(f8, f32)


@pytest.mark.parametrize('precision', ['bf16x3', 'bf16', 'bf16s'])
def test_predict_in_every_training_precision(batch, precision):
    from ann3depth_amd import models
    img, dep, params, a = batch
    net = models.MSDNReplica(2, device='cuda:0', params=params, precision=precision)
    coarse, fine = net.predict(dev(img))
    torch.cuda.synchronize()
    tol = {'bf16x3': {'coarse': 1e-3, 'fine': 1e-3}}.get(precision, bf16s_tol.DEPTH)
    e_c, e_f = rel(coarse.cpu().numpy(), a['coarse'][..., 0]), rel(fine.cpu().numpy(), a['fine'][..., 0])
    print(f'{precision}: coarse {e_c:.2e} fine {e_f:.2e}')
    assert e_c < tol['coarse'] and e_f < tol['fine']


# ---------------------------------------------------------------------------------------------- driver end to end
def _write(path, n, seed):
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(seed)
    with tfrecord.TFRecordWriter(path) as w:
        for _ in range(n):
            img = rng.integers(0, 256, (48, 64, 3)).astype(np.float32) / np.float32(255) - np.float32(.5)
            dep = rng.integers(0, 256, (6, 8, 1)).astype(np.float32) / np.float32(255) - np.float32(.5)
            w.write_example(img, dep)


def _oracle_metrics(params, root, resolution='grid'):
    from ann3depth_amd import data, ops
    inputs, _ = data.inputs(root, 'nyu', 4, 'test', shuffle=False)
    rows = {'coarse': [], 'fine': []}
    loss = {'coarse': [], 'fine': []}
    fine = []
    while True:
        try:
            img, dep = inputs.pipeline.next_batch()
        except data.OutOfRangeError:
            break
        a = O.forward(params, img, dep, None)
        for k in rows:
            out = a[k][..., 0]
            if resolution == 'grid':
                rows[k].append(ref_rows(out, a['depths']))
            else:
                rows[k].append(ref_rows(T.resize_bilinear_tf1(a[k], 6, 8)[..., 0], dep))
            loss[k].append((float(T.silog_loss_fwd(a[k], a['depths'])), len(img)))
        fine.append(a['fine'][..., 0])
    res = {}
    for k in rows:
        res[k] = ops.summarize_depth_metrics(np.concatenate(rows[k]))
        res[k]['silog'] = sum(l * n for l, n in loss[k]) / sum(n for _, n in loss[k])
    return res, np.concatenate(fine)


def _oracle_targets(root):
    """The test split's depth maps in file order, as stored and resized to the model grid by the oracle."""
    from ann3depth_amd import data
    inputs, _ = data.inputs(root, 'nyu', 4, 'test', shuffle=False)
    deps = []
    while True:
        try:
            deps.append(inputs.pipeline.next_batch()[1])
        except data.OutOfRangeError:
            break
    dep = np.concatenate(deps)
    return dep, T.resize_bilinear_tf1(dep, 55, 74)


def _agree(got, want):
    for k in ('coarse', 'fine'):
        g, w = got[k], want[k]
        assert g['pixels'] == w['pixels'] and g['images'] == w['images'] and g['nonfinite'] == w['nonfinite']
        for m in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'log10', 'rmse_si'):
            assert g[m] == pytest.approx(w[m], rel=1e-4), (k, m, g[m], w[m])
        # the training objective takes log(o + 1e-8) of the UNclamped output: at the untrained weights' outputs near zero
        # a 1e-7 change of o moves a pixel's term by a lot (tests/test_gpu_msdn.py: ill-conditioned); its computation is
        # checked at 1e-4 on the GPU's own predictions in the test below
        assert g['silog'] == pytest.approx(w['silog'], rel=1e-2), (k, g['silog'], w['silog'])
        for m in ('delta1', 'delta2', 'delta3'):
            assert abs(g[m] - w[m]) * w['pixels'] <= 1 + 1e-9, (k, m, g[m], w[m])


def test_evaluate_a_trained_checkpoint_end_to_end(tmp_path, capsys):
    from ann3depth_amd import ann3depth, evaluate
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'nyu'))
    _write(os.path.join(root, 'nyu', 'train.tfrecords'), 40, 0)
    _write(os.path.join(root, 'nyu', 'test.tfrecords'), 13, 1)
    ck = str(tmp_path / 'ckpt')
    base = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', root, '--id', 'r1']
    assert ann3depth.main(base + ['--steps', '6', '--sumfreq', '100', '--tf-checkpoints', 'nyu']) == 0
    capsys.readouterr()
    run = os.path.join(ck, 'msdn_r1')
    pred_path = str(tmp_path / 'pred.npy')
    ev = base
    assert evaluate.main(ev + ['--predictions', pred_path, 'nyu']) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert got['records'] == 13 and got['global_step'] == 6 and got['checkpoint'].endswith('model.ckpt-6.pt')
    sd = torch.load(os.path.join(run, 'model.ckpt-6.pt'))
    params = {n: sd[n].numpy() for n in O.param_shapes()}
    want, fine = _oracle_metrics(params, root)
    _agree(got, want)
    pred = np.load(pred_path)
    assert pred.shape == (13, 55, 74) and pred.dtype == np.float32
    assert all(rel(pred[i], fine[i]) < 1e-3 for i in range(13))          # record order
    _, grid_t = _oracle_targets(root)
    objective = [(float(T.silog_loss_fwd(pred[a:a + 4, :, :, None], grid_t[a:a + 4])), len(pred[a:a + 4]))
                 for a in range(0, 13, 4)]
    assert got['fine']['silog'] == pytest.approx(sum(l * n for l, n in objective) / 13, rel=1e-4)
    assert json.load(open(os.path.join(run, 'eval-6.json')))['fine'] == got['fine']
    events = [f for f in os.listdir(run) if f.startswith('events.out.tfevents.')]
    assert any(b'eval/fine/abs_rel' in open(os.path.join(run, f), 'rb').read() for f in events)
    # the TensorFlow bundle of the same step gives the same numbers
    assert evaluate.main(ev + ['--checkpoint', os.path.join(run, 'model.ckpt-6'), 'nyu']) == 0
    got_tf = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got_tf['coarse'] == got['coarse'] and got_tf['fine'] == got['fine']
    # the depth maps as stored (6 x 8), the prediction sampled in the kernel
    assert evaluate.main(ev + ['--resolution', 'record', 'nyu']) == 0
    got_rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want_rec, _ = _oracle_metrics(params, root, 'record')
    assert got_rec['fine']['pixels'] == want_rec['fine']['pixels'] <= 13 * 48
    _agree(got_rec, {k: dict(want_rec[k], silog=want[k]['silog']) for k in ('coarse', 'fine')})
