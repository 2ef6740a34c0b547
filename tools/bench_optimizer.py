"""What SGD with momentum (--optimizer momentum, include/a3d_optim.h) costs on one GPU against what it replaces, by the method of
tools/bench_objective.py: the two sides alternate launch by launch in one process, every launch between its own device events,
5 warm-up and 30 timed launches per side and round.
  launches    a3do_momentum_apply beside a3d_adam_apply_tf1 at beta2 = 0.999 on the dense group's 67 M elements (3 streams
              read and 2 written against 4 and 3), and a3do_dense_bwd_filter_momentum beside a3d_dense_bwd_filter +
              a3do_momentum_apply on dense_0 [12288, 4096] and dense_1 [4096, 4070] at 32 and 64 batch rows ('new' is the fused
              launch, 'parent' the two calls);
  step        the coarse-phase fp32 step at batch 32 under optimizer='momentum' with keep_dense_grads=False (the fused launch,
              'new') beside keep_dense_grads=True (the two calls, 'parent'), in one process;
  parent DIR  whole steps against the PARENT COMMIT's own build, DIR being a built checkout of the commit before: `one_step`
              below as a process of its own, in turns, on DIR (the default step, and the step at beta2 = 0.999: the only moving
              weights the parent has) and on this checkout (the default step, momentum fused, momentum unfused), three rounds;
              then `python bench.py --gpus 1` in both checkouts in turns.  This process never touches the GPU;
  one_step ROOT SIDE   what `parent` starts: ms per step of the coarse-phase fp32 step of the package under ROOT; SIDE is default,
              adam999, momentum or momentum_unfused.
The weights of a step timed here move by the paper's rates on random records and leave every sensible range within a few steps;
the launches and their bytes do not depend on the values.  One part per process, one JSON line each, as profiles/bench_optimizer.json
holds them:
    for part in launches step "parent ../parent"; do python tools/bench_optimizer.py $part; done > profiles/bench_optimizer.json"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B = 32
DENSE_GROUP = 67010560                # elements of MSDNReplica's CoarseDense flat buffer
LAYERS = {'dense_0': (12288, 4096), 'dense_1': (4096, 4070)}
STEPS, WARM = 300, 30                 # of one_step
SIDES = {'default': {}, 'adam999': {'beta2': 0.999}, 'momentum': {'optimizer': 'momentum'},
         'momentum_unfused': {'optimizer': 'momentum', 'keep_dense_grads': True}}


def launches(rng, repeats):
    import torch
    from ann3depth_amd import ops
    from tools.bench_augment import compare
    out = {}
    var, m, v, g = (torch.from_numpy(rng.standard_normal(DENSE_GROUP).astype(np.float32)).cuda() for _ in range(4))
    v.abs_()
    out[f'apply_{DENSE_GROUP}_momentum_vs_adam999'] = compare(
        lambda: ops.momentum_apply(var, m, g, 1e-6, 0.9),
        lambda: ops.adam_apply_tf1(var, m, v, g, 1e-6, 0.9, 0.999, 1e-8, 0.9, 0.999), repeats)
    del v
    for name, (k, n) in LAYERS.items():
        var_w, acc_w, dw = (t[:k * n].view(k, n) for t in (var, m, g))
        var_b, acc_b, db = (torch.zeros(n, device='cuda') for _ in range(3))
        for rows in (32, 64):
            x = torch.from_numpy(rng.standard_normal((rows, k)).astype(np.float32)).cuda()
            dz = torch.from_numpy((rng.standard_normal((rows, n)) * 1e-3).astype(np.float32)).cuda()

            def two_calls():
                ops.dense_bwd_filter(x, dz, dw, db)
                ops.momentum_apply(var_w, acc_w, dw, 1e-6, 0.9)
                ops.momentum_apply(var_b, acc_b, db, 1e-6, 0.9)
            out[f'{name}_m{rows}_fused_vs_two_calls'] = compare(
                lambda: ops.dense_bwd_filter_momentum(x, dz, var_w, acc_w, var_b, acc_b, 1e-6, 0.9), two_calls, repeats)
    return out


def steps(rng, repeats):
    from ann3depth_amd import models
    from tools.bench_augment import TIMED, WARMUP, compare
    from tools.bench_objective import step_inputs
    img, dep, keep = step_inputs(rng)
    nets = [models.MSDNReplica(B, device='cuda:0', **{'keep_dense_grads': False, **SIDES[side]})
            for side in ('momentum', 'momentum_unfused')]
    assert nets[0]._fused_dense_momentum() and not nets[1]._fused_dense_momentum()
    assert models.phase_of(nets[0].global_step + repeats * (WARMUP + TIMED), B) == 1
    return {f'step_coarse_fp32_b{B}_momentum_fused_vs_unfused': compare(lambda: nets[0].step(img, dep, keep),
                                                                        lambda: nets[1].step(img, dep, keep), repeats)}


def one_step(root, side):
    """ms per step over STEPS coarse-phase fp32 steps of the package under `root`, after WARM."""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from ann3depth_amd import models
    assert os.path.abspath(models.__file__).startswith(os.path.abspath(root) + os.sep), models.__file__
    from tools.bench_objective import step_inputs
    img, dep, keep = step_inputs(np.random.default_rng(0))
    net = models.MSDNReplica(B, device='cuda:0', **{'keep_dense_grads': False, **SIDES[side]})
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
    """one_step as a process of its own on the parent's checkout and on this one, in turns; then bench.py in both."""
    from tools.bench_objective import bench_against_parent
    parent = os.path.abspath(parent_dir)
    sides = (('parent_default', parent, 'default'), ('new_default', HERE, 'default'), ('parent_adam999', parent, 'adam999'),
             ('new_adam999', HERE, 'adam999'), ('new_momentum', HERE, 'momentum'), ('new_momentum_unfused', HERE, 'momentum_unfused'))
    ms = {k: [] for k, _, _ in sides}
    for _ in range(rounds):
        for k, root, side in sides:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), 'one_step', root, side], cwd=root,
                                  capture_output=True, text=True, timeout=300, check=True)
            ms[k].append(json.loads(done.stdout.strip().splitlines()[-1])['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) * 1e3, 2) for k, v in ms.items()}
    us = lambda a, b: round((med[a] - med[b]) * 1e3, 2)          # noqa: E731
    return {'part': 'parent', 'rounds': rounds, 'steps': STEPS, 'warmup': WARM, 'ms_per_step': ms, 'spread_us': spread,
            'default_minus_parent_us': us('new_default', 'parent_default'),
            'adam999_minus_parent_us': us('new_adam999', 'parent_adam999'),
            'momentum_minus_parent_adam999_us': us('new_momentum', 'parent_adam999'),
            'momentum_unfused_minus_parent_adam999_us': us('new_momentum_unfused', 'parent_adam999'),
            'momentum_fused_minus_unfused_us': us('new_momentum', 'new_momentum_unfused'),
            'bench': bench_against_parent(parent, rounds)}


def main():
    usage = 'launches, step, parent DIR or one_step ROOT SIDE'
    part, more = sys.argv[1] if len(sys.argv) > 1 else 'launches', sys.argv[2:]
    if part == 'one_step':
        print(json.dumps(one_step(*more)))
        return
    if part == 'parent':
        print(json.dumps(against_parent(more[0], int(more[1]) if len(more) > 1 else 3)))
        return
    if part not in ('launches', 'step'):
        raise SystemExit(f'{part!r}: {usage}')
    import torch
    from tools.bench_augment import TIMED, WARMUP
    repeats = int(more[0]) if more else 3
    out = {'part': part, 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    out.update((launches if part == 'launches' else steps)(np.random.default_rng(0), repeats))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
