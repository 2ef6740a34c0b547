"""What an MSDN objective beside the scale-invariant log loss costs on one GPU at b = 32 on the 55 x 74 grid (npix = 4070), against
the launches and the step it replaces (never against itself).  OBJECTIVE is gradloss (--loss-gradient 0.5,
include/a3d_gradloss.h), berhu (--loss berhu, fraction 0.2, include/a3d_berhu.h) or ssi (--loss ssi, include/a3d_ssi.h):
  launches    the objective's forward and backward launches beside a3d_silog_loss_fwd / _bwd_ex, then the same pairs masked beside
              a3dx_silog_masked_loss_fwd / _bwd_ex with 30 % holes; ssi also beside berhu's (the same bytes, two launches too), with
              `berhu_vs_silog_*`, berhu's own forward against silog's in the same process, whose round-to-round spread is the
              yardstick for ssi against berhu;
  step        the coarse-phase fp32 training step built with the objective beside the step built without the argument, plain and
              with valid_range = (0, 0.99); gradloss first also with grad_weight=0.0, the same launches in one checkout;
  parent DIR  the DEFAULT step of this checkout against the PARENT COMMIT's own build, DIR being a built checkout of the commit
              before.  berhu and ssi: `one_step` below as a process of its own, in turns, on DIR and on this checkout (silog, then
              the objective), three rounds.  gradloss: `python bench.py --gpus 1`, which builds the replica without the argument,
              in this checkout and in DIR in turns.  This process never touches the GPU;
  one_step ROOT SIDE   what `parent` starts: ms per step of the coarse-phase fp32 step of the package under ROOT, SIDE being
              silog or the objective.
Method as tools/bench_valid.py: the two sides alternate launch by launch in one process, every launch between its own device
events, 5 warm-up and 30 timed launches per side and round.  One part per process, one JSON line each, with the keys
profiles/bench_{gradloss,berhu,ssi}.json hold:
    for part in launches step "parent ../parent"; do python tools/bench_objective.py ssi $part; done > profiles/bench_ssi.json"""
import collections
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 32, 55, 74
NPIX = H * W
WEIGHT, FRACTION = 0.5, 0.2
HOLES = {'valid_range': (0.0, 0.99)}
STEPS, WARM = 300, 30                 # of one_step
BENCH_ARGS = ['--gpus', '1', '--steps', '300', '--warmup', '30', '--no-cpu-baseline', '--no-fine', '--no-dp-rank',
              '--no-dp-rank-standin']

# What differs between the objectives: the replica's keyword arguments, the word its step keys carry, a flag-off step timed
# first as (word, keyword arguments), the objectives besides silog its launches are timed against, whether the outputs are drawn
# around the targets (linear depth) or on their own, and ops' workspace, fwd(ops, o, t, masked, loss, ws) and
# bwd(ops, o, t, masked, ws, g).
Objective = collections.namedtuple('Objective', 'kw word off beside around ws fwd bwd')
OBJECTIVES = {
    'gradloss': Objective({'grad_weight': WEIGHT}, f'weight{WEIGHT}', ('weight0', {'grad_weight': 0.0}), (), False, 'silog_grad_ws',
                          lambda ops, o, t, m, loss, ws: ops.silog_grad_loss_fwd(o, t, H, W, m, WEIGHT, loss, ws),
                          lambda ops, o, t, m, ws, g: ops.silog_grad_loss_bwd(o, t, H, W, m, WEIGHT, ws, g)),
    'berhu': Objective({'objective': 'berhu', 'berhu_fraction': FRACTION}, 'berhu', None, (), True, 'berhu_ws',
                       lambda ops, o, t, m, loss, ws: ops.berhu_loss_fwd(o, t, m, FRACTION, loss, ws),
                       lambda ops, o, t, m, ws, g: ops.berhu_loss_bwd(o, t, m, FRACTION, ws, g)),
    'ssi': Objective({'objective': 'ssi'}, 'ssi', None, ('berhu',), True, 'ssi_ws',
                     lambda ops, o, t, m, loss, ws: ops.ssi_loss_fwd(o, t, m, loss, ws),
                     lambda ops, o, t, m, ws, g: ops.ssi_loss_bwd(o, t, m, ws, g)),
}


def launches(objective, rng, repeats):
    import torch
    from ann3depth_amd import ops
    from tools.bench_augment import compare
    spec, out = OBJECTIVES[objective], {}
    if not spec.around:
        o = (rng.random((B, NPIX)) * 3 - 0.4).astype(np.float32)
    t = (rng.random((B, NPIX)) * 10 + 0.05).astype(np.float32)
    if spec.around:
        o = (t + rng.standard_normal((B, NPIX)) * 3).astype(np.float32)
    o = torch.from_numpy(o).cuda()
    holed = t.copy()
    holed[rng.random((B, NPIX)) < 0.3] = np.nan
    loss, g = torch.zeros(4, device='cuda'), torch.empty((B, NPIX), device='cuda')
    own = {name: getattr(ops, OBJECTIVES[name].ws)(B, 'cuda') for name in (objective, *spec.beside)}

    def side(name, masked, tgt):
        if name == 'silog':
            ws = ops.silog_masked_ws(B, 'cuda') if masked else ops.silog_ws(B, 'cuda')
            fwd = ops.silog_masked_loss_fwd if masked else ops.silog_loss_fwd
            bwd = ops.silog_masked_loss_bwd if masked else ops.silog_loss_bwd
            return lambda: fwd(o, tgt, loss[:2], ws), lambda: bwd(o, tgt, ws, g)
        other = OBJECTIVES[name]
        return (lambda: other.fwd(ops, o, tgt, masked, loss, own[name]), lambda: other.bwd(ops, o, tgt, masked, own[name], g))

    for masked, tgt in ((0, torch.from_numpy(t).cuda()), (1, torch.from_numpy(holed).cuda())):
        key = 'masked' if masked else 'plain'
        sides = {name: side(name, masked, tgt) for name in (objective, 'silog', *spec.beside)}
        for name in ('silog', *spec.beside):
            vs = f'_vs_{name}' if spec.beside else ''
            out[f'fwd_{key}_b{B}{vs}'] = compare(sides[objective][0], sides[name][0], repeats)
            out[f'bwd_{key}_b{B}{vs}'] = compare(sides[objective][1], sides[name][1], repeats)
        for name in spec.beside:
            out[f'{name}_vs_silog_fwd_{key}_b{B}'] = compare(sides[name][0], sides['silog'][0], repeats)
    return out


def step_inputs(rng):
    import torch
    from tools.bench_valid import depth_maps
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    dep = depth_maps(rng, B)
    keep = torch.from_numpy((rng.random((B, 4096)) >= 0.5).astype(np.uint8)).cuda()
    return img, dep, keep


def steps(objective, rng, repeats):
    from ann3depth_amd import models
    from tools.bench_augment import TIMED, WARMUP, compare
    spec, out = OBJECTIVES[objective], {}
    img, dep, keep = step_inputs(rng)
    variants = [(spec.word, spec.kw, {}), (spec.word + '_holes', {**spec.kw, **HOLES}, HOLES)]
    for word, new_kw, old_kw in ([(*spec.off, {})] if spec.off else []) + variants:
        nets = [models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, **kw) for kw in (new_kw, old_kw)]
        assert models.phase_of(nets[0].global_step + repeats * (WARMUP + TIMED), B) == 1
        out[f'step_coarse_fp32_b{B}_{word}'] = compare(lambda: nets[0].step(img, dep, keep), lambda: nets[1].step(img, dep, keep),
                                                      repeats)
        del nets
    return out


def one_step(root, side):
    """ms per step over STEPS coarse-phase fp32 steps of the package under `root`, after WARM; 'silog' passes no argument."""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from ann3depth_amd import models
    assert os.path.abspath(models.__file__).startswith(os.path.abspath(root) + os.sep), models.__file__
    sys.path.insert(1, HERE)
    img, dep, keep = step_inputs(np.random.default_rng(0))
    net = models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False, **({} if side == 'silog' else OBJECTIVES[side].kw))
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


def against_parent(objective, parent_dir, rounds):
    """one_step as a process of its own on the parent's checkout and on this one, in turns."""
    sides = (('parent_silog', os.path.abspath(parent_dir), 'silog'), ('new_silog', HERE, 'silog'),
             (f'new_{objective}', HERE, objective))
    ms = {k: [] for k, _, _ in sides}
    for _ in range(rounds):
        for k, root, side in sides:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), objective, 'one_step', root, side], cwd=root,
                                  capture_output=True, text=True, timeout=300, check=True)
            ms[k].append(json.loads(done.stdout.strip().splitlines()[-1])['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {'part': 'parent', 'rounds': rounds, 'steps': STEPS, 'warmup': WARM, 'ms_per_step': ms,
            f'{objective}_minus_parent_us': round((med[f'new_{objective}'] - med['parent_silog']) * 1e3, 2),
            'silog_minus_parent_us': round((med['new_silog'] - med['parent_silog']) * 1e3, 2),
            'parent_spread_us': round((max(ms['parent_silog']) - min(ms['parent_silog'])) * 1e3, 2)}


def bench_against_parent(parent_dir, runs):
    """bench.py's result line from this checkout and from parent_dir, in turns."""
    sides = {'new': HERE, 'parent': os.path.abspath(parent_dir)}
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
    usage = f'{"|".join(OBJECTIVES)} then launches, step, parent DIR or one_step ROOT SIDE'
    if len(sys.argv) < 2 or sys.argv[1] not in OBJECTIVES:
        raise SystemExit(usage)
    objective, part, more = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else 'launches', sys.argv[3:]
    if part == 'one_step':
        print(json.dumps(one_step(*more)))
        return
    if part == 'parent':
        rounds = int(more[1]) if len(more) > 1 else 3
        print(json.dumps(bench_against_parent(more[0], rounds) if objective == 'gradloss' else
                         against_parent(objective, more[0], rounds)))
        return
    if part not in ('launches', 'step'):
        raise SystemExit(f'{part!r}: {usage}')
    sys.path.insert(0, HERE)
    import torch
    from tools.bench_augment import TIMED, WARMUP
    repeats = int(more[0]) if more else 3
    out = {'part': part, 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed_launches': TIMED, 'repeats': repeats}
    out.update((launches if part == 'launches' else steps)(objective, np.random.default_rng(0), repeats))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
