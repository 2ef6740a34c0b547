"""The MSDN training step and the driver on depth maps with holes (MSDNReplica(valid_range=...), --min-depth / --max-depth):
without holes the step is the plain step bit for bit; with holes the target, both losses and the loss gradients are those of
tests/valid_ref.py."""
import json
import os
import signal
import struct

import numpy as np
import pytest
import torch

import augment_ref as R
import valid_ref as V
from ann3depth_amd import augment as A
from oracle import msdn as O
from oracle import tfrecord as OT

pytestmark = pytest.mark.gpu

INF = float('inf')
B = 2


@pytest.fixture(scope='module')
def params():
    return O.init_params(3000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stored_batch(seed, holes):
    """uint8 images and depth maps stored at 48 x 64; holes: two blobs of k = 0 per map, one touching the last row and column."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (B, 48, 64, 3), dtype=np.uint8)
    dep = rng.integers(1, 255, (B, 48, 64, 1), dtype=np.uint8)
    if holes:
        dep[:, 5:20, 10:30] = 0
        dep[:, 40:, 50:] = 0
        dep[0, 30, 3] = 255                     # the range cap
    return img, dep, (rng.random((B, 4096)) >= 0.5).astype(np.uint8)


def fine_start(models):
    return models.SAMPLES_COARSE // B          # the first global step of the fine phase


def test_without_holes_the_step_is_the_plain_step(params):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(1, holes=False)
    nets = [models.MSDNReplica(B, params=params, beta2=0.999, valid_range=vr) for vr in (None, (0, INF))]
    assert nets[0].valid_range is None and nets[1].valid_range == (0.0, INF)
    for start in (0, fine_start(models)):
        outs = []
        for net in nets:
            net.global_step = start
            outs.append(net.step(dev(img), dev(dep), dev(keep)))
        torch.cuda.synchronize()
        assert outs[0]['phase'] == outs[1]['phase'] == (1 if start == 0 else 2)
        for k in ('coarse_loss', 'fine_loss'):
            assert torch.equal(outs[0][k], outs[1][k]) and np.isfinite(float(outs[0][k])), k
        assert float(nets[1].loss_pair_c[1]) == 1.0 and float(nets[1].loss_pair_f[1]) == 1.0
        for name in ('x', 't', 'coarse', 'fine', 'dz1' if start == 0 else 'dfine'):
            assert torch.equal(getattr(nets[0], name), getattr(nets[1], name)), name
        for gname in nets[0].groups:
            ga, gb = nets[0].groups[gname], nets[1].groups[gname]
            for buf in ('grad', 'var', 'm', 'v'):
                assert torch.equal(getattr(ga, buf), getattr(gb, buf)), f'{gname}.{buf}'
    assert float(nets[0].groups['CoarseDense'].m.abs().sum()) > 0 and float(nets[0].groups['FineA'].m.abs().sum()) > 0


def check_step_with_holes(params, table, lo, hi, seed):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(seed, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(lo, hi))
    want_t = V.resize_valid(dep, R.identity(B) if table is None else table, 55, 74, lo, hi)
    hole = np.isnan(want_t)
    assert 0.02 < hole.mean() < 0.5
    for start in (0, fine_start(models)):
        net.global_step = start
        out = net.step(dev(img), dev(dep), dev(keep), warp=None if table is None else dev(table))
        torch.cuda.synchronize()
        t = net.t.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(t), hole)
        np.testing.assert_array_equal(t.view(np.uint32)[~hole], want_t.view(np.uint32)[~hole])
        t64 = t.reshape(B, -1).astype(np.float64)
        for which, pair in (('coarse', net.loss_pair_c), ('fine', net.loss_pair_f)):
            o64 = getattr(net, which).cpu().numpy().reshape(B, -1).astype(np.float64)
            ref, frac = V.masked_silog_fwd(o64, t64)
            got = float(out[which + '_loss'])
            print(f'{which} loss {got:.6g} reference {ref:.6g} rel err {abs(got - ref) / abs(ref):.2e} valid {frac:.4f}')
            assert np.isfinite(got) and abs(got - ref) < 2e-6 * abs(ref)
            assert float(pair[1]) == np.float32(frac) and 0 < frac < 1
        which, g = ('coarse', net.dz1) if start == 0 else ('fine', net.dfine)
        g = g.cpu().numpy().reshape(B, -1)
        o64 = getattr(net, which).cpu().numpy().reshape(B, -1).astype(np.float64)
        assert (g[hole.reshape(B, -1)] == 0).all() and np.isfinite(g).all() and (g != 0).any()
        assert V.rel_l2(g, V.masked_silog_bwd(o64, t64)) < 1e-5
    for gname in net.groups:
        assert bool(torch.isfinite(net.groups[gname].var).all()), gname
    # the summaries: a hole is shown as 0, the scalar is there
    tag, target, _ = net.summary_images()[3]
    assert tag == 'summaries/Target'
    np.testing.assert_array_equal(target.cpu().numpy(), np.where(hole, np.float32(0), t)[:3])
    assert net.summary_scalars(out)['valid_fraction'] == float(np.float32((~hole).sum() / hole.size))


def test_step_with_holes_is_the_reference(params):
    check_step_with_holes(params, None, 0.0, 0.99, seed=2)


def test_step_with_holes_and_a_warp_table_is_the_reference(params):
    check_step_with_holes(params, A.table(A.Eigen2014(), 3000, 0, 1, B, 48, 64), 0.0, INF, seed=3)


def test_depth_maps_stored_at_another_size_take_the_valid_resize_too(params):
    from ann3depth_amd import models
    img, _, keep = stored_batch(4, holes=False)
    dep = np.random.default_rng(4).integers(1, 255, (B, 24, 32, 1), dtype=np.uint8)
    dep[:, 3:9, 4:12] = 0
    net = models.MSDNReplica(B, params=params, valid_range=(0, INF))
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    want = V.resize_valid(dep, R.identity(B), 55, 74, 0, INF)
    t = net.t.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(t), np.isnan(want))
    np.testing.assert_array_equal(t.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.isfinite(float(out['coarse_loss'])) and 0 < float(net.loss_pair_c[1]) < 1


def test_bf16_storage_takes_the_masked_gradient_as_bf16_rows(params):
    """--precision bf16s: dense_1's backward reads dz1 as bf16 rows of 4072; the masked backward writes them too."""
    from ann3depth_amd import models
    img, dep, keep = stored_batch(5, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, precision='bf16s', valid_range=(0, INF))
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    hole = np.isnan(V.resize_valid(dep, R.identity(B), 55, 74, 0, INF)).reshape(B, -1)
    np.testing.assert_array_equal(np.isnan(net.t.cpu().numpy()).reshape(B, -1), hole)
    assert np.isfinite(float(out['coarse_loss'])) and np.isfinite(float(out['fine_loss']))
    dz1, dz16 = net.dz1.cpu(), net.dz1_16.float().cpu()
    assert torch.equal(dz16[:, :4070], dz1.to(torch.bfloat16).float()) and bool((dz16[:, 4070:] == 0).all())
    assert bool((dz1.numpy()[hole] == 0).all()) and bool((dz1 != 0).any())
    for gname in ('CoarseConv', 'CoarseDense'):
        assert bool(torch.isfinite(net.groups[gname].var).all()), gname


def test_a_bad_range_is_refused(params):
    from ann3depth_amd import models
    with pytest.raises(ValueError, match='valid_range'):
        models.MSDNReplica(B, params=params, valid_range=(1.0, 0.5))


# ---------------------------------------------------------------------------------------------- the driver
def write_shard(root, holes, n=24):
    """One record n times (see tests/test_gpu_augment.py::write_shard), 48 x 64, converter-style floats k / 255 - 0.5 the
    loader stages as uint8; holes: blobs of k = 0 in the depth map."""
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    k = rng.integers(1, 256, (48, 64, 1))
    if holes:
        k[8:20, 10:40] = 0
        k[44:, 60:] = 0
    img = rng.integers(0, 256, (48, 64, 3)).astype(np.float32) / np.float32(255) - np.float32(.5)
    dep = k.astype(np.float32) / np.float32(255) - np.float32(.5)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'train.tfrecords')) as w:
        for _ in range(n):
            w.write_example(img, dep)


def rows(ck, run):
    return [json.loads(l) for l in open(os.path.join(ck, run, 'summaries.jsonl'))]


def losses(ck, run):
    return {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss']) for r in rows(ck, run)}


def event_scalars(ck, run, tag):
    """Every simple_value logged under `tag` in the run's event files (Summary.Value: tag = field 1, simple_value = 2)."""
    key = bytes([0x0a, len(tag)]) + tag.encode() + b'\x15'
    found = []
    d = os.path.join(ck, run)
    for name in sorted(os.listdir(d)):
        if name.startswith('events.out.tfevents.'):
            for payload in OT.unframe(open(os.path.join(d, name), 'rb').read()):
                at = payload.find(key)
                if at >= 0:
                    found.append(struct.unpack('<f', payload[at + len(key):at + len(key) + 4])[0])
    return found


def test_driver_on_a_shard_with_holes_is_reproducible_and_resumable(tmp_path):
    from ann3depth_amd import ann3depth, models
    holed, whole = tmp_path / 'holed', tmp_path / 'whole'
    write_shard(str(holed), holes=True)
    write_shard(str(whole), holes=False)
    ck = str(tmp_path / 'ckpt')

    def run(run_id, steps, datadir, *flags):
        argv = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', str(datadir), '--sumfreq', '1',
                '--trace-every', '0', '--beta2', '0.999', '--augment', 'eigen', '--id', run_id, '--steps', str(steps),
                *flags, 'nyu']
        assert ann3depth.main(argv) == 0
        return losses(ck, 'msdn_' + run_id)
    try:
        a = run('a', 6, holed, '--min-depth', '0')
        assert models.msdn.valid_range == (0.0, INF)
        b = run('b', 6, holed, '--min-depth', '0')
        assert sorted(a) == [1, 2, 3, 4, 5, 6] and a == b                  # reproducible
        assert all(np.isfinite(v) for pair in a.values() for v in pair) and len(set(a.values())) == 6
        first = run('c', 3, holed, '--min-depth', '0')
        resumed = run('c', 6, holed, '--min-depth', '0')                   # continues from the step-3 checkpoint
        assert first == {k: a[k] for k in (1, 2, 3)} and resumed == a
        fractions = [r['valid_fraction'] for r in rows(ck, 'msdn_a')]
        logged = event_scalars(ck, 'msdn_a', 'valid_fraction')
        assert len(logged) == 6 and logged == [float(np.float32(f)) for f in fractions]
        assert all(0 < f < 1 for f in logged)
        # a shard without holes under thresholds that admit everything: the losses of the run without the flags
        with_flag = run('d', 3, whole, '--min-depth', '-1')
        assert models.msdn.valid_range == (-1.0, INF)
        without = run('e', 3, whole)
        assert models.msdn.valid_range is None
        assert with_flag == without
        assert all(r['valid_fraction'] == 1.0 for r in rows(ck, 'msdn_d'))
        assert not any('valid_fraction' in r for r in rows(ck, 'msdn_e'))
        assert event_scalars(ck, 'msdn_e', 'valid_fraction') == []
    finally:
        models.msdn.augment = None
        models.msdn.valid_range = None
        for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
            signal.signal(s, signal.SIG_DFL)


def test_dcnf_with_a_depth_range_is_refused(tmp_path):
    from ann3depth_amd import ann3depth
    try:
        for flags in (['--min-depth', '0'], ['--max-depth', '0.99']):
            assert ann3depth.main(['--model', 'dcnf', '--ckptdir', str(tmp_path), '--datadir', str(tmp_path), *flags, 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', '--ckptdir', str(tmp_path), '--datadir', str(tmp_path), '--min-depth', '2',
                               '--max-depth', '1', 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
    finally:
        for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
            signal.signal(s, signal.SIG_DFL)
