"""What the gradient-matching term (--loss-gradient, include/a3d_gradloss.h) costs on one GPU, against the launches and the
step it replaces (never against itself), at b = 32 on the 55 x 74 grid:
  launches   a3dg_silog_grad_loss_fwd beside a3d_silog_loss_fwd and a3dg_silog_grad_loss_bwd_ex beside a3d_silog_loss_bwd_ex
             (weight 0.5), then the same pairs masked beside a3dx_silog_masked_loss_fwd / _bwd_ex with 30 % holes;
  step_off   the coarse-phase fp32 training step built with grad_weight=0.0 beside the step built without the argument (the
             same launches in one checkout: what a pair of replicas resolves);
  parent DIR the flag-off step against the parent commit: `python bench.py --gpus 1` (which builds the replica without the
             argument) in this checkout and in DIR, a built checkout of the commit before, alternately, a process each;
  step_on    the step with grad_weight=0.5 beside the step without, plain and with valid_range = (0, 0.99).
Method and output as tools/bench_valid.py: the two sides alternate launch by launch in one process, every launch between its
own device events, 5 warm-up and 30 timed launches per side and round.  One part per process, one JSON line each:
    for part in launches step_off step_on "parent ../parent"; do python tools/bench_gradloss.py $part; done \
        > profiles/bench_gradloss.json"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import models, ops  # noqa: E402
from tools.bench_augment import TIMED, WARMUP, compare  # noqa: E402
from tools.bench_valid import depth_maps  # noqa: E402

B, H, W, WEIGHT = 32, 55, 74, 0.5


def launches(rng, repeats):
    out = {}
    npix = H * W
    o = torch.from_numpy((rng.random((B, npix)) * 3 - 0.4).astype(np.float32)).cuda()
    t = (rng.random((B, npix)) * 10 + 0.05).astype(np.float32)
    holed = t.copy()
    holed[rng.random((B, npix)) < 0.3] = np.nan
    loss, g = torch.zeros(4, device='cuda'), torch.empty((B, npix), device='cuda')
    wsg = ops.silog_grad_ws(B, 'cuda')
    for masked, tgt in ((0, torch.from_numpy(t).cuda()), (1, torch.from_numpy(holed).cuda())):
        ws = ops.silog_masked_ws(B, 'cuda') if masked else ops.silog_ws(B, 'cuda')
        old_fwd = ops.silog_masked_loss_fwd if masked else ops.silog_loss_fwd
        old_bwd = ops.silog_masked_loss_bwd if masked else ops.silog_loss_bwd
        key = 'masked' if masked else 'plain'
        out[f'fwd_{key}_b{B}'] = compare(lambda: ops.silog_grad_loss_fwd(o, tgt, H, W, masked, WEIGHT, loss, wsg),
                                         lambda: old_fwd(o, tgt, loss[:2], ws), repeats)
        out[f'bwd_{key}_b{B}'] = compare(lambda: ops.silog_grad_loss_bwd(o, tgt, H, W, masked, WEIGHT, wsg, g),
                                         lambda: old_bwd(o, tgt, ws, g), repeats)
    return out


def steps(rng, repeats, variants):
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    dep = depth_maps(rng, B)
    keep = torch.from_numpy((rng.random((B, 4096)) >= 0.5).astype(np.uint8)).cuda()
    out = {}
    for key, new_kw, old_kw in variants:
        nets = [models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, **kw) for kw in (new_kw, old_kw)]
        assert models.phase_of(nets[0].global_step + repeats * (WARMUP + TIMED), B) == 1
        out[key] = compare(lambda: nets[0].step(img, dep, keep), lambda: nets[1].step(img, dep, keep), repeats)
        del nets
    return out


BENCH_ARGS = ['--gpus', '1', '--steps', '300', '--warmup', '30', '--no-cpu-baseline', '--no-fine', '--no-dp-rank',
              '--no-dp-rank-standin']


def against_parent(parent_dir, runs):
    """bench.py's result line from this checkout and from parent_dir in turns; this process never touches the GPU."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sides = {'new': here, 'parent': os.path.abspath(parent_dir)}
    lines = {k: [] for k in sides}
    for _ in range(runs):
        for k, d in sides.items():
            done = subprocess.run([sys.executable, 'bench.py', *BENCH_ARGS], cwd=d, capture_output=True, text=True, timeout=300,
                                  check=True)
            lines[k].append(json.loads(done.stdout.strip().splitlines()[-1]))
    out = {'part': 'parent', 'bench_args': ' '.join(BENCH_ARGS), 'runs': runs}
    for k, ls in lines.items():
        out[k] = {'images_per_sec': [l['value'] for l in ls], 'ms_per_step': [l['ms_per_step'] for l in ls]}
    med = {k: float(np.median(out[k]['ms_per_step'])) for k in sides}
    out['ratio_of_median_ms'] = round(med['new'] / med['parent'], 4)
    out['parent_ms_spread'] = round((max(out['parent']['ms_per_step']) - min(out['parent']['ms_per_step'])) / med['parent'], 4)
    return out


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else 'launches'
    if part == 'parent':
        print(json.dumps(against_parent(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)))
        return
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rng = np.random.default_rng(0)
    out = {'part': part, 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    holes = {'valid_range': (0.0, 0.99)}
    if part == 'launches':
        out.update(launches(rng, repeats))
    elif part == 'step_off':
        out.update(steps(rng, repeats, [(f'step_coarse_fp32_b{B}_weight0', {'grad_weight': 0.0}, {})]))
    elif part == 'step_on':
        out.update(steps(rng, repeats, [(f'step_coarse_fp32_b{B}_weight{WEIGHT}', {'grad_weight': WEIGHT}, {}),
                                        (f'step_coarse_fp32_b{B}_weight{WEIGHT}_holes', {'grad_weight': WEIGHT, **holes}, holes)]))
    else:
        raise SystemExit(f'{part!r}: launches, step_off, step_on or parent DIR')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
