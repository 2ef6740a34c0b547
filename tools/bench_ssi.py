"""What the scale-and-shift-invariant objective (--loss ssi, include/a3d_ssi.h) costs on one GPU at b = 32 and npix = 4070,
against the launches and the step of the scale-invariant log loss and of the reverse Huber loss:
  launches    a3di_ssi_loss_fwd (two launches) beside a3d_silog_loss_fwd and beside a3dh_berhu_loss_fwd (two launches, the same
              bytes), a3di_ssi_loss_bwd_ex beside a3d_silog_loss_bwd_ex and a3dh_berhu_loss_bwd_ex, then the same pairs masked
              (a3dx_silog_masked_loss_fwd / _bwd_ex) with 30 % holes; `berhu_vs_silog_*` is berHu's own forward against silog's in
              the same process, whose round-to-round spread is the yardstick for ssi against berHu;
  step        the coarse-phase fp32 training step built with objective='ssi' beside the step built without the argument (the
              parent commit's launches, which this change leaves as they are), plain and with valid_range = (0, 0.99);
  parent DIR  the DEFAULT step of this checkout against the PARENT COMMIT's own build: `one_step` below run as a process of its
              own, in turns, on DIR (a built checkout of the commit before) and on this checkout (silog, then ssi), three
              rounds;
  one_step ROOT OBJECTIVE   what `parent` starts: ms per step of the coarse-phase fp32 step of the package under ROOT.
Method and output of launches / step as tools/bench_berhu.py: the two sides alternate launch by launch in one process, every
launch between its own device events, 5 warm-up and 30 timed launches per side and round.  One part per process, one JSON
line each:
    for part in launches step "parent ../parent"; do python tools/bench_ssi.py $part; done > profiles/bench_ssi.json"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NPIX, FRACTION = 32, 4070, 0.2
STEPS, WARM = 300, 30                 # of one_step


def launches(rng, repeats):
    import torch
    from ann3depth_amd import ops
    from tools.bench_augment import compare
    out = {}
    t = (rng.random((B, NPIX)) * 10 + 0.05).astype(np.float32)
    o = torch.from_numpy((t + rng.standard_normal((B, NPIX)) * 3).astype(np.float32)).cuda()
    holed = t.copy()
    holed[rng.random((B, NPIX)) < 0.3] = np.nan
    loss, g = torch.zeros(4, device='cuda'), torch.empty((B, NPIX), device='cuda')
    wsi, wsh = ops.ssi_ws(B, 'cuda'), ops.berhu_ws(B, 'cuda')
    for masked, tgt in ((0, torch.from_numpy(t).cuda()), (1, torch.from_numpy(holed).cuda())):
        ws = ops.silog_masked_ws(B, 'cuda') if masked else ops.silog_ws(B, 'cuda')
        silog_fwd = ops.silog_masked_loss_fwd if masked else ops.silog_loss_fwd
        silog_bwd = ops.silog_masked_loss_bwd if masked else ops.silog_loss_bwd
        key = 'masked' if masked else 'plain'
        sides = {'silog': (lambda: silog_fwd(o, tgt, loss[:2], ws), lambda: silog_bwd(o, tgt, ws, g)),
                 'berhu': (lambda: ops.berhu_loss_fwd(o, tgt, masked, FRACTION, loss, wsh),
                           lambda: ops.berhu_loss_bwd(o, tgt, masked, FRACTION, wsh, g))}
        for name, (fwd, bwd) in sides.items():
            out[f'fwd_{key}_b{B}_vs_{name}'] = compare(lambda: ops.ssi_loss_fwd(o, tgt, masked, loss, wsi), fwd, repeats)
            out[f'bwd_{key}_b{B}_vs_{name}'] = compare(lambda: ops.ssi_loss_bwd(o, tgt, masked, wsi, g), bwd, repeats)
        out[f'berhu_vs_silog_fwd_{key}_b{B}'] = compare(sides['berhu'][0], sides['silog'][0], repeats)
    return out


def step_inputs(rng):
    import torch
    from tools.bench_valid import depth_maps
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    keep = torch.from_numpy((rng.random((B, 4096)) >= 0.5).astype(np.uint8)).cuda()
    return img, depth_maps(rng, B), keep


def steps(rng, repeats):
    from ann3depth_amd import models
    from tools.bench_augment import TIMED, WARMUP, compare
    img, dep, keep = step_inputs(rng)
    out = {}
    for key, kw in ((f'step_coarse_fp32_b{B}_ssi', {}), (f'step_coarse_fp32_b{B}_ssi_holes', {'valid_range': (0.0, 0.99)})):
        nets = [models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, **more, **kw) for more in ({'objective': 'ssi'}, {})]
        assert models.phase_of(nets[0].global_step + repeats * (WARMUP + TIMED), B) == 1
        out[key] = compare(lambda: nets[0].step(img, dep, keep), lambda: nets[1].step(img, dep, keep), repeats)
        del nets
    return out


def one_step(root, objective):
    """ms per step over STEPS coarse-phase fp32 steps of the package under `root`, after WARM; the parent's package has no
    'ssi', and 'silog' passes no argument."""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from ann3depth_amd import models
    assert os.path.abspath(models.__file__).startswith(os.path.abspath(root) + os.sep), models.__file__
    sys.path.insert(1, HERE)
    img, dep, keep = step_inputs(np.random.default_rng(0))
    net = models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, **({'objective': 'ssi'} if objective == 'ssi' else {}))
    assert models.phase_of(net.global_step + WARM + STEPS, B) == 1
    for _ in range(WARM):
        net.step(img, dep, keep)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        net.step(img, dep, keep)
    b.record()
    torch.cuda.synchronize()
    return {'ms_per_step': round(a.elapsed_time(b) / STEPS, 4)}


def against_parent(parent_dir, rounds):
    """one_step as a process of its own on the parent's checkout and on this one, in turns; this process never touches the GPU."""
    sides = (('parent_silog', os.path.abspath(parent_dir), 'silog'), ('new_silog', HERE, 'silog'), ('new_ssi', HERE, 'ssi'))
    ms = {k: [] for k, _, _ in sides}
    for _ in range(rounds):
        for k, root, objective in sides:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), 'one_step', root, objective], cwd=root,
                                  capture_output=True, text=True, timeout=300, check=True)
            ms[k].append(json.loads(done.stdout.strip().splitlines()[-1])['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {'part': 'parent', 'rounds': rounds, 'steps': STEPS, 'warmup': WARM, 'ms_per_step': ms,
            'ssi_minus_parent_us': round((med['new_ssi'] - med['parent_silog']) * 1e3, 2),
            'silog_minus_parent_us': round((med['new_silog'] - med['parent_silog']) * 1e3, 2),
            'parent_spread_us': round((max(ms['parent_silog']) - min(ms['parent_silog'])) * 1e3, 2)}


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else 'launches'
    if part == 'one_step':
        print(json.dumps(one_step(sys.argv[2], sys.argv[3])))
        return
    if part == 'parent':
        print(json.dumps(against_parent(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)))
        return
    sys.path.insert(0, HERE)
    import torch
    from tools.bench_augment import TIMED, WARMUP
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rng = np.random.default_rng(0)
    out = {'part': part, 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    if part == 'launches':
        out.update(launches(rng, repeats))
    elif part == 'step':
        out.update(steps(rng, repeats))
    else:
        raise SystemExit(f'{part!r}: launches, step, parent DIR or one_step ROOT OBJECTIVE')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
