"""BASELINE config 4: DCNF unary conv stack, batch 16 (768 patches of 100x100x3), one MI355X.
Times the forward (resize -> patches -> 5 conv / 3 pool / 3 dense), the unary backward from a synthetic dz, and the
whole `models.dcnf` train step (+ pairwise part, CRF loss, gradient descent).  --train-pairwise: the step that also
learns the pairwise dense layer (NON-REFERENCE); `crf_loss_ms` is the loss launch alone in the form the step uses.
--pairwise-texture: the pairwise part with the LBP texture similarity as a third feature (NON-REFERENCE).
--holes: the step on depth maps with holes (NON-REFERENCE, DCNFReplica(valid_range=(0, 0.99))): the synthetic depth gets a
band at the range cap over its upper third and scattered zeros, so that whole superpixels, and some in part, are not
targets; `crf_loss_ms` is then ops.crf_loss_observed.
--unary fcsp: the fully convolutional unary with superpixel pooling (NON-REFERENCE, DCNFReplica(unary='fcsp')): the convs
once over the 240x320 image; `forward_tflops` then counts that form's own multiply-adds (conv_macs below).
--superpixel N (with --unary fcsp; NON-REFERENCE, DCNFReplica(superpixel=N)): the step on the 12 x 16 (N = 20) or 24 x 32
(N = 10) grid, whose CRF is the banded one (include/a3d_crf_band.h); `crf_loss_ms` is then ops.crf_band_nll in the form the
step uses, and `band` holds the band launches alone (nll with dr, nll without, map), their dynamic LDS bytes, the
workgroups per CU that leaves room for, and the share of the step the step's own launch takes.  --superpixel 40 is the
run without the flag.
--segmentation slic (with --unary fcsp; NON-REFERENCE, DCNFReplica(segmentation='slic')): the step on SLIC superpixels
(include/a3d_slic.h); `slic` then holds each new launch alone: the segmentation (5 rounds), the label mean of the target and
of the image, the label histogram, the pair similarities, the label pooling forward and backward.  --segmentation grid is
the run without the flag.
    python tools/bench_dcnf.py [batch] [--train-pairwise] [--pairwise-texture] [--holes] [--unary fcsp] [--superpixel N]
                               [--segmentation slic] > dcnf.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import models, ops  # noqa: E402

PAIRWISE = '--train-pairwise' in sys.argv[1:]
TEXTURE = '--pairwise-texture' in sys.argv[1:]
HOLES = '--holes' in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a not in ('--train-pairwise', '--pairwise-texture', '--holes')]
UNARY = 'patch'
if '--unary' in argv:
    i = argv.index('--unary')
    UNARY = argv[i + 1]
    del argv[i:i + 2]
SUPERPIXEL = 40
if '--superpixel' in argv:
    i = argv.index('--superpixel')
    SUPERPIXEL = int(argv[i + 1])
    del argv[i:i + 2]
SLIC = False
if '--segmentation' in argv:
    i = argv.index('--segmentation')
    SLIC = argv[i + 1] == 'slic'
    del argv[i:i + 2]
B = int(argv[0]) if argv else 16
rng = np.random.default_rng(1000)
img = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)).cuda()
dep = rng.random((B, 55, 74, 1)).astype(np.float32)
if HOLES:
    dep = 0.05 + 0.9 * dep
    dep[:, :22] = 1.0                                         # the range cap: two rows of superpixels and part of a third
    dep[rng.random(dep.shape) < 0.08] = 0.0                   # no return
dep = torch.from_numpy(dep).cuda()


def conv_macs(h, w, rows):
    """Multiply-adds of the unary stack on one h x w input (VALID convs, 2x2 pools) with `rows` dense rows behind it."""
    total = 0
    for n, ci, co, k in models.DCNF_CONVS:
        h, w = h - k + 1, w - k + 1
        total += h * w * co * k * k * ci
        if n in models.DCNF_POOL_AFTER:
            h, w = h // 2, w // 2
    first = h * w * co if rows == 1 else co                     # the patch form flattens its 7 x 7 x 256 map
    return total + rows * (first * 128 + 128 * 16 + 16)


if SLIC:
    rep = models.DCNFReplica(B, train_pairwise=PAIRWISE, pairwise_texture=TEXTURE, valid_range=(0.0, 0.99) if HOLES else None,
                             unary=UNARY, superpixel=SUPERPIXEL, segmentation='slic')
elif SUPERPIXEL != 40:
    rep = models.DCNFReplica(B, train_pairwise=PAIRWISE, pairwise_texture=TEXTURE, valid_range=(0.0, 0.99) if HOLES else None,
                             unary=UNARY, superpixel=SUPERPIXEL)
elif UNARY != 'patch':
    rep = models.DCNFReplica(B, train_pairwise=PAIRWISE, pairwise_texture=TEXTURE, valid_range=(0.0, 0.99) if HOLES else None,
                             unary=UNARY)
elif HOLES:
    rep = models.DCNFReplica(B, train_pairwise=PAIRWISE, pairwise_texture=TEXTURE, valid_range=(0.0, 0.99))
elif TEXTURE:
    rep = models.DCNFReplica(B, train_pairwise=PAIRWISE, pairwise_texture=True)
else:
    rep = models.DCNFReplica(B, train_pairwise=True) if PAIRWISE else models.DCNFReplica(B)
net = rep.unary
dz = torch.randn((net.P, 1), device='cuda')
# the objective of the untouched network, before the timed steps move it (at the reference's rate 0.1 they move it far)
first_loss = float(rep.forward(img, dep)) if HOLES or SLIC else None      # slic: also leaves the labels the unary pools over


def timeit(fn, reps=10):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


t_fwd = timeit(lambda: net.forward(img))
t_bwd = timeit(lambda: net.backward(dz))
t_step = timeit(lambda: rep.step(img, dep))
t_crf = timeit(lambda: rep.forward_crf(dep))
loss_args = (net.z.view(B, rep.nsp), rep.y.view(B, rep.nsp), rep.r, rep.left, rep.right, models.DCNF_EPSILON)
band = None
if SUPERPIXEL != 40:
    bz, by = loss_args[0].clone(), loss_args[1].clone()
    t_loss = timeit(lambda: ops.crf_band_nll(bz, by, rep.r, rep.left, rep.right, rep.band, pair_grad=PAIRWISE), reps=50)
    t_dr = timeit(lambda: ops.crf_band_nll(bz, by, rep.r, rep.left, rep.right, rep.band, pair_grad=True), reps=50)
    t_nodr = timeit(lambda: ops.crf_band_nll(bz, by, rep.r, rep.left, rep.right, rep.band, pair_grad=False), reps=50)
    t_map = timeit(lambda: ops.crf_band_map(bz, rep.r, rep.left, rep.right, rep.band, rep.crf, rep.status), reps=50)
    lds = (rep.nsp * ((rep.band + 2) & ~1) + 2 * rep.nsp) * 4            # band_lds_bytes of csrc/crf_band.hip
    band = {'grid': [rep.rows, rep.cols], 'superpixels': rep.nsp, 'band': rep.band, 'pairs': int(rep.left.numel()),
            'nll_with_dr_ms': round(t_dr, 4), 'nll_without_dr_ms': round(t_nodr, 4), 'map_ms': round(t_map, 4),
            'lds_bytes_per_workgroup': lds, 'workgroups_per_cu_by_lds': min(160 * 1024 // lds, 32), 'workgroups': B,
            'threads_per_workgroup': 256, 'share_of_step': round(t_loss / t_step, 4)}
elif HOLES:
    t_loss = timeit(lambda: ops.crf_loss_observed(*loss_args[:5], pair_grad=PAIRWISE), reps=50)
else:
    t_loss = timeit(lambda: (ops.crf_loss_grad if PAIRWISE else ops.crf_loss)(*loss_args), reps=50)
gflop_patch = 2.672          # forward GFLOP per patch
fwd_tf = gflop_patch * net.P / t_fwd           # GFLOP / ms = TFLOP/s
workload = f'DCNF unary, batch {B} -> {net.P} patches 100x100x3'
extra = {}
if UNARY != 'patch':
    gflop_image = 2e-9 * conv_macs(models.DCNF_IMG_H, models.DCNF_IMG_W, rep.nsp)
    fwd_tf = gflop_image * B / t_fwd
    workload = f'DCNF unary ({UNARY}), batch {B} -> {B} images 240x320x3, {net.P} superpixel rows'
    extra = {'unary': UNARY, 'forward_gflop_per_image': round(gflop_image, 3),
             'patch_form_gflop_per_image': round(2e-9 * 48 * conv_macs(100, 100, 1), 3)}
if band is not None:
    extra = {**extra, 'superpixel': SUPERPIXEL, 'band': band}
if SLIC:
    x, sp, last = net.resized, rep.sp, net.act['conv2d_4/pool']
    pooled, dpooled = net.act['pooled'].view(B, rep.nsp, -1), torch.randn((B, rep.nsp, 256), device='cuda')
    dflat = torch.empty_like(last)
    slic = {'segment_ms': timeit(lambda: rep._segment(), reps=50),
            'label_mean_target_ms': timeit(lambda: ops.label_mean(rep.depths240, sp, rep.labels, rep.y, rep.count3), reps=50),
            'label_mean_image_ms': timeit(lambda: ops.label_mean(x, sp, rep.labels, rep.mean3, rep.count3), reps=50),
            'label_hist_ms': timeit(lambda: ops.label_hist(x, sp, rep.labels, rep.hist), reps=50),
            'pair_similarity_ms': timeit(lambda: ops.label_pair_similarity(rep.mean3, rep.hist, rep.label_count, rep.left,
                                                                          rep.right, rep.pair_var('kernel'),
                                                                          rep.pair_var('bias'), models.DCNF_GAMMA), reps=50),
            'label_pool_fwd_ms': timeit(lambda: ops.label_pool_fwd(last, net.map, rep.labels, rep.label_count, pooled), reps=50),
            'label_pool_bwd_ms': timeit(lambda: ops.label_pool_bwd(dpooled, net.map, rep.labels, rep.label_count, dflat), reps=50)}
    grid_labels = (torch.arange(240, device='cuda')[:, None] // sp * rep.cols + torch.arange(320, device='cuda')[None, :] // sp)
    extra = {**extra, 'superpixel': SUPERPIXEL, 'segmentation': 'slic', 'slic_iters': rep.slic_iters,
             'slic_compactness': rep.slic_compactness, 'slic': {k: round(v, 4) for k, v in slic.items()},
             'pixels_off_their_block': round(float((rep.labels != grid_labels.int()).float().mean()), 4)}
if HOLES:
    torch.cuda.synchronize()
    nobs = rep.nobs.cpu().numpy()
    extra = {**extra, 'holes': True, 'observed_fraction': round(float(nobs.sum()) / (B * rep.nsp), 4),
             'observed_superpixels_min_max': [int(nobs.min()), int(nobs.max())], 'loss_before_the_steps': round(first_loss, 4)}
print(json.dumps({'workload': workload, 'forward_ms': round(t_fwd, 3),
                  'forward_images_per_s': round(B / t_fwd * 1e3, 1), 'forward_tflops': round(fwd_tf, 1),
                  'backward_ms': round(t_bwd, 3), 'dtype': 'f32',
                  'train_step_ms': round(t_step, 3), 'train_step_images_per_s': round(B / t_step * 1e3, 1),
                  'pairwise_and_crf_loss_ms': round(t_crf, 3), 'crf_loss_ms': round(t_loss, 4), 'train_pairwise': PAIRWISE,
                  'pairwise_texture': TEXTURE,
                  'fwd_bwd_images_per_s': round(B / (t_fwd + t_bwd) * 1e3, 1), **extra}))
