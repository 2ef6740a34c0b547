"""models.DCNFUnaryFCSP on the GPU against tests/fcsp_ref.py at a small image: B = 2, 80 x 120 gives a 4 x 9 last map and
2 x 3 superpixels of edge 40, with cells that straddle superpixel borders on both axes.  The tolerances are those
tests/test_gpu_dcnf.py and tests/test_gpu_train.py hold the patch form to: z within 1e-3 rel-L2, every activation and every
gradient within 1e-4.  As there, the backward is checked on the activations the GPU produced (a ReLU or a pool window that
a last-bit difference flips says nothing about the kernels under test).

precision='bf16' is not exercised: tests/bf16s_tol.py lists no DCNF tensor to hold it to."""
import numpy as np
import pytest
import torch

import fcsp_ref as F
from oracle import dcnf as OD
from oracle import tf13_ops as T

pytestmark = pytest.mark.gpu

B, HW, SP = 2, (80, 120), 40


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope='module')
def run():
    """One forward and backward of the fused form, its inputs and the reference forward: shared, read only."""
    from ann3depth_amd import models
    rng = np.random.default_rng(5)
    img = (rng.integers(0, 256, (B, 160, 240, 3)) / 255).astype(np.float32)
    params = F.init_params(3000)
    for n in params:                                            # biases away from zero: every ReLU has both sides
        if n.endswith('/bias'):
            params[n] = (0.05 * rng.standard_normal(params[n].shape)).astype(np.float32)
    net = models.DCNFUnaryFCSP(B, params=params, image_hw=HW, sp=SP)
    z = net.forward(torch.from_numpy(img).cuda())
    dz = rng.standard_normal((net.P, 1)).astype(np.float32)
    net.backward(torch.from_numpy(dz).cuda())
    torch.cuda.synchronize()
    resized = T.resize_bilinear_tf1(img, *HW)
    ref = F.unary_forward({k: v.astype(np.float64) for k, v in params.items()}, resized.astype(np.float64), SP)
    return dict(net=net, z=z.cpu().numpy(), dz=dz, params=params, img=img, resized=resized, ref=ref)


def test_shapes_and_the_resized_image(run):
    net = run['net']
    assert (net.rows, net.cols, net.S, net.P) == (2, 3, 6, 12) and net.map_hw == (4, 9)
    assert net.conv_hw['conv2d_1'] == (31, 51) and net.act['conv2d_1/pool'].shape == (B, 15, 25, 256)     # odd maps lose a row / column
    assert net.act['conv2d_4/pool'].shape == (B, 4, 9, 256) and net.act['pooled'].shape == (12, 256)
    assert net.fuse_pool and run['z'].shape == (B, 6, 1)
    np.testing.assert_array_equal(net.resized.cpu().numpy(), run['resized'])
    assert net.var('dense/kernel').shape == (256, 128)


def test_forward_matches_the_reference(run):
    net, ref = run['net'], run['ref']
    assert rel(run['z'].reshape(-1, 1), ref['z']) < 1e-3
    for n in ('conv2d/pool', 'conv2d_1/pool', 'conv2d_2', 'conv2d_3', 'conv2d_4/pool', 'pooled', 'dense', 'dense_1', 'dense_2'):
        e = rel(net.act[n].cpu().numpy(), ref[n])
        print(f'{n}: rel-L2 {e:.3g}')
        assert e < 1e-4, n
    assert float(np.abs(ref['z']).min()) > 0 and (ref['dense'] > 0).any() and (ref['dense'] == 0).any()


def backward_reference(net, params, dz):
    a = {k: v.astype(np.float64) for k, v in net.activations().items()}
    return F.unary_backward({k: v.astype(np.float64) for k, v in params.items()}, a, dz.astype(np.float64), SP)


def test_backward_matches_the_reference(run):
    net = run['net']
    g = backward_reference(net, run['params'], run['dz'])
    for key, name in (('pooled', 'd:pooled'), ('flat', 'd:conv2d_4/pool')):
        e = rel(net.dact[key].cpu().numpy().reshape(g[name].shape), g[name])
        print(f'{name}: rel-L2 {e:.3g}')
        assert np.linalg.norm(g[name]) > 0 and e < 1e-4, name
    for n in net.shapes:
        e = rel(net.group.view(net.group.grad, n).cpu().numpy(), g[n])
        print(f'{n}: rel-L2 {e:.3g}')
        assert np.linalg.norm(g[n]) > 0 and e < 1e-4, n


def test_unfused_pools_give_the_same_gradients(run):
    from ann3depth_amd import models
    net = run['net']
    plain = models.DCNFUnaryFCSP(B, params=run['params'], image_hw=HW, sp=SP, fuse_pool=False)
    assert not plain.fuse_pool and not plain.argmax and 'conv2d' in plain.act
    z = plain.forward(torch.from_numpy(run['img']).cuda())
    plain.backward(torch.from_numpy(run['dz']).cuda())
    torch.cuda.synchronize()
    assert rel(z.cpu().numpy(), run['z']) < 1e-4
    for n in net.shapes:
        assert rel(plain.group.view(plain.group.grad, n).cpu().numpy(), net.group.view(net.group.grad, n).cpu().numpy()) < 1e-4, n
    g = backward_reference(plain, run['params'], run['dz'])
    for n in net.shapes:
        assert rel(plain.group.view(plain.group.grad, n).cpu().numpy(), g[n]) < 1e-4, n


def test_equal_seed_gives_the_patch_forms_conv_kernels():
    from ann3depth_amd import models
    a = models.DCNFUnaryFCSP(1, seed=11, image_hw=HW, sp=SP)
    b = models.DCNFUnary(1, seed=11)
    for n in a.shapes:
        if '/conv2d' in n:
            assert torch.equal(a.group.view(a.group.var, n).view(torch.int32), b.group.view(b.group.var, n).view(torch.int32)), n
    assert a.var('dense/kernel').shape == (256, 128) and b.var('dense/kernel').shape == (12544, 128)
    assert list(a.shapes) == list(b.shapes)
    ref = F.init_params(11)
    for n in a.shapes:
        np.testing.assert_array_equal(a.group.view(a.group.var, n).cpu().numpy(), ref[n])


def test_prediction_path_leaves_the_pool_positions_alone(run):
    net = run['net']
    arg = {k: v.clone() for k, v in net.argmax.items()}
    z = net.forward_resized(record_argmax=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(z.cpu().numpy(), run['z'])
    assert all(torch.equal(arg[k], net.argmax[k]) for k in arg)
