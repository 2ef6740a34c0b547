"""What --augment eigen costs on one GPU, against the launch and the step it replaces (never against itself):
  - a3d_warp_bilinear_pair with an Eigen table beside a3d_resize_bilinear_tf1_ex's pair launch, same uint8-staged
    480 x 640 buffers, same 228 x 304 x 3 + 55 x 74 x 1 outputs, B = 32 and 64;
  - the coarse-phase fp32 training step at B = 32 with and without a table.
The two sides of each pair alternate launch by launch in one process; every launch sits between its own device events.
Per side: median, minimum and the 10th / 90th percentile of the timed launches, for each of `repeats` rounds (the spread
of the round medians is the noise the ratio has to be read against).
    python tools/bench_augment.py [repeats] > profiles/bench_augment.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import augment, models, ops  # noqa: E402

WARMUP, TIMED = 5, 30


def alternate(fns, warmup=WARMUP, timed=TIMED):
    """ms of every timed call of each function, the functions taking turns: a b a b ..."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    evs = [[] for _ in fns]
    for _ in range(timed):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return [np.array([a.elapsed_time(b) for a, b in e]) for e in evs]


def stats(ms):
    return {'median_us': round(float(np.median(ms)) * 1e3, 2), 'min_us': round(float(ms.min()) * 1e3, 2),
            'p10_us': round(float(np.percentile(ms, 10)) * 1e3, 2), 'p90_us': round(float(np.percentile(ms, 90)) * 1e3, 2)}


def compare(new, old, repeats):
    rounds = []
    for _ in range(repeats):
        t_new, t_old = alternate([new, old])
        rounds.append({'new': stats(t_new), 'parent': stats(t_old),
                       'ratio_of_medians': round(float(np.median(t_new) / np.median(t_old)), 4)})
    ratios = [r['ratio_of_medians'] for r in rounds]
    parents = [r['parent']['median_us'] for r in rounds]
    return {'rounds': rounds, 'ratio_median': round(float(np.median(ratios)), 4), 'ratio_min': min(ratios),
            'ratio_max': max(ratios),
            'parent_median_spread': round((max(parents) - min(parents)) / float(np.median(parents)), 4)}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    cfg = augment.Eigen2014()
    for B in (32, 64):
        img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
        dep = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 1)).astype(np.uint8)).cuda()
        y0, y1 = torch.empty((B, 228, 304, 3), device='cuda'), torch.empty((B, 55, 74, 1), device='cuda')
        table = torch.from_numpy(augment.table(cfg, 3000, 0, 0, B, 480, 640)).cuda()
        ident = torch.from_numpy(augment.identity(B)).cuda()
        out[f'launch_b{B}_eigen_table'] = compare(lambda: ops.warp_bilinear_pair(img, y0, dep, y1, table),
                                                  lambda: ops.resize_bilinear_tf1_pair(img, y0, dep, y1), repeats)
        out[f'launch_b{B}_identity_table'] = compare(lambda: ops.warp_bilinear_pair(img, y0, dep, y1, ident),
                                                     lambda: ops.resize_bilinear_tf1_pair(img, y0, dep, y1), repeats)
        del img, dep
    B = 32
    net = models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False)
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    dep = torch.from_numpy(rng.integers(1, 256, (B, 480, 640, 1)).astype(np.uint8)).cuda()
    keep = torch.from_numpy((rng.random((B, 4096)) >= 0.5).astype(np.uint8)).cuda()
    table = torch.from_numpy(augment.table(cfg, 3000, 0, 0, B, 480, 640)).cuda()
    assert models.phase_of(net.global_step + 2 * repeats * (WARMUP + TIMED), B) == 1
    out[f'step_coarse_fp32_b{B}'] = compare(lambda: net.step(img, dep, keep, warp=table), lambda: net.step(img, dep, keep),
                                           repeats)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
