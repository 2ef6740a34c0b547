"""What training on depth maps with holes (--min-depth / --max-depth) costs on one GPU, against the launches and the step
it replaces (never against itself):
  - a3dx_resize_bilinear_tf1_valid beside a3d_resize_bilinear_tf1_ex's pair launch, and a3dx_warp_bilinear_pair_valid beside
    a3d_warp_bilinear_pair with the same Eigen table: same uint8-staged 480 x 640 buffers (a sixth of every depth map
    punched out), same 228 x 304 x 3 + 55 x 74 x 1 outputs, thresholds (0, 0.99), B = 32 and 64;
  - the masked loss, forward + backward, beside the plain pair at (32, 4070), 30 % of the targets NaN;
  - the coarse-phase fp32 training step at B = 32 with valid_range = (0, 0.99) and without.
Method and output as tools/bench_augment.py: the two sides alternate launch by launch in one process, every launch between
its own device events, 5 warm-up and 30 timed launches per side and round.
    python tools/bench_valid.py [repeats] > profiles/bench_valid.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import augment, models, ops  # noqa: E402
from tools.bench_augment import TIMED, WARMUP, compare  # noqa: E402


def depth_maps(rng, B):
    dep = rng.integers(1, 256, (B, 480, 640, 1)).astype(np.uint8)
    dep[:, 100:300, 150:400] = 0          # a sixth of the map, as a Kinect shadow or a Make3D sky region
    dep[:, 400:, 600:] = 0
    return torch.from_numpy(dep).cuda()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    lo, hi = 0.0, 0.99
    for B in (32, 64):
        img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
        dep = depth_maps(rng, B)
        y0, y1 = torch.empty((B, 228, 304, 3), device='cuda'), torch.empty((B, 55, 74, 1), device='cuda')
        table = torch.from_numpy(augment.table(augment.Eigen2014(), 3000, 0, 0, B, 480, 640)).cuda()
        out[f'resize_b{B}'] = compare(lambda: ops.resize_bilinear_tf1_pair_valid(img, y0, dep, y1, lo, hi),
                                      lambda: ops.resize_bilinear_tf1_pair(img, y0, dep, y1), repeats)
        out[f'warp_b{B}_eigen_table'] = compare(lambda: ops.warp_bilinear_pair_valid(img, y0, dep, y1, table, lo, hi),
                                                lambda: ops.warp_bilinear_pair(img, y0, dep, y1, table), repeats)
        del img, dep
    B, npix = 32, 4070
    o = torch.from_numpy((rng.random((B, npix)) * 3 - 0.4).astype(np.float32)).cuda()
    t = (rng.random((B, npix)) * 10 + 0.05).astype(np.float32)
    t[rng.random((B, npix)) < 0.3] = np.nan
    t = torch.from_numpy(t).cuda()
    loss, g = torch.zeros(2, device='cuda'), torch.empty((B, npix), device='cuda')
    ws, wsm = ops.silog_ws(B, 'cuda'), ops.silog_masked_ws(B, 'cuda')

    def masked():
        ops.silog_masked_loss_fwd(o, t, loss, wsm)
        ops.silog_masked_loss_bwd(o, t, wsm, g)

    def plain():
        ops.silog_loss_fwd(o, t, loss, ws)
        ops.silog_loss_bwd(o, t, ws, g)
    out[f'loss_fwd_bwd_b{B}'] = compare(masked, plain, repeats)
    nets = [models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, valid_range=vr) for vr in ((lo, hi), None)]
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    dep = depth_maps(rng, B)
    keep = torch.from_numpy((rng.random((B, 4096)) >= 0.5).astype(np.uint8)).cuda()
    assert models.phase_of(nets[0].global_step + repeats * (WARMUP + TIMED), B) == 1
    out[f'step_coarse_fp32_b{B}'] = compare(lambda: nets[0].step(img, dep, keep), lambda: nets[1].step(img, dep, keep), repeats)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
