"""What gradient clipping by global norm (--clip-norm, include/a3d_clip.h) costs on one GPU, by the method of
tools/bench_optimizer.py: the two sides alternate launch by launch in one process, every launch between its own device events,
5 warm-up and 30 timed launches per side and round.
  launches    a3dn_grad_norm_scale beside a3do_momentum_apply on the dense group's 67 010 560 elements and on the conv group's
              ('new' is the norm, one stream read; 'parent' the apply, three read and two written), with the bytes per second of
              both; and the pair the step runs on the conv group, norm then a3dn_momentum_apply_ctl, beside the plain apply;
  step        the coarse-phase fp32 step at batch 32 under optimizer='momentum': clip_norm=inf ('new') beside the unfused
              unclipped step and beside the fused one ('parent'), in one process, step by step;
  parent DIR  `python bench.py --gpus 1` in this checkout and in DIR, a built checkout of the commit before, in turns, three rounds.
              This process never touches the GPU;
  divergence  the eight first steps of the training driver on the random records of tests/test_gpu_valid_train.py::write_shard
              at batch 4 under --optimizer momentum at the paper's rates, at clip_norm inf, 100, 10 and 1: the losses, and the
              norms and scales the summaries hold.
One part per process, one JSON line each, as profiles/bench_clip.json holds them:
    for part in launches step "parent ../parent" divergence; do python tools/bench_clip.py $part; done > profiles/bench_clip.json"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B = 32
DENSE_GROUP = 67010560                # elements of MSDNReplica's CoarseDense flat buffer
CLIPS = ('inf', '100', '10', '1')


def launches(rng, repeats):
    import torch
    from ann3depth_amd import models, ops
    from tools.bench_augment import compare
    probe = models.MSDNReplica(1, device='cuda:0')
    counts = {'dense': probe.groups['CoarseDense'].count, 'conv': probe.groups['CoarseConv'].count}
    assert counts['dense'] == DENSE_GROUP
    del probe
    out = {'counts': counts}
    var, m, g = (torch.from_numpy(rng.standard_normal(DENSE_GROUP).astype(np.float32)).cuda() for _ in range(3))
    for name, count in counts.items():
        v, a, gr = var[:count], m[:count], g[:count]
        ctl, ws = ops.clip_ctl('cuda'), ops.grad_norm_ws(count, 'cuda')
        res = compare(lambda: ops.grad_norm_scale(gr, 1.0, 1e30, ctl, ws), lambda: ops.momentum_apply(v, a, gr, 1e-6, 0.9), repeats)
        for r in res['rounds']:                                                # the norm reads 4 bytes per element, the apply moves 20
            r['new']['TB_per_s'] = round(4 * count / r['new']['median_us'] / 1e6, 3)
            r['parent']['TB_per_s'] = round(20 * count / r['parent']['median_us'] / 1e6, 3)
        out[f'norm_vs_momentum_apply_{name}_{count}'] = res

        def pair():
            ops.grad_norm_scale(gr, 1.0, 1e30, ctl, ws)
            ops.momentum_apply_ctl(v, a, gr, 1e-6, 0.9, ctl)
        out[f'norm_then_apply_ctl_vs_apply_{name}_{count}'] = compare(pair, lambda: ops.momentum_apply(v, a, gr, 1e-6, 0.9), repeats)
    return out


def steps(rng, repeats):
    from ann3depth_amd import models
    from tools.bench_augment import TIMED, WARMUP, compare
    from tools.bench_objective import step_inputs
    img, dep, keep = step_inputs(rng)
    kw = dict(device='cuda:0', optimizer='momentum')
    clipped = models.MSDNReplica(B, keep_dense_grads=False, clip_norm=float('inf'), **kw)
    unfused = models.MSDNReplica(B, keep_dense_grads=True, **kw)
    fused = models.MSDNReplica(B, keep_dense_grads=False, **kw)
    assert clipped.keep_dense_grads and fused._fused_dense_momentum() and not unfused._fused_dense_momentum()
    assert models.phase_of(clipped.global_step + 2 * repeats * (WARMUP + TIMED), B) == 1
    return {f'step_coarse_fp32_b{B}_momentum_clip_inf_vs_unfused': compare(lambda: clipped.step(img, dep, keep),
                                                                           lambda: unfused.step(img, dep, keep), repeats),
            f'step_coarse_fp32_b{B}_momentum_clip_inf_vs_fused': compare(lambda: clipped.step(img, dep, keep),
                                                                         lambda: fused.step(img, dep, keep), repeats)}


def divergence():
    """{clip_norm: [{step, coarse_loss, fine_loss, norms, scales, skipped}]} of eight steps of the driver."""
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    from ann3depth_amd import ann3depth
    from test_gpu_valid_train import rows, write_shard
    out = {}
    with tempfile.TemporaryDirectory() as root:
        data, ck = os.path.join(root, 'data'), os.path.join(root, 'ckpt')
        write_shard(data, holes=False)
        for c in CLIPS:
            argv = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--sumfreq', '1', '--trace-every', '0',
                    '--optimizer', 'momentum', '--clip-norm', c, '--id', 'clip' + c, '--steps', '8', 'nyu']
            assert ann3depth.main(argv) == 0
            out[c] = [{'step': r['global_step'], 'coarse_loss': r['loss/coarse_loss'], 'fine_loss': r['loss/fine_loss'],
                       **{k.split('optimizers/')[1]: v for k, v in r.items() if k.startswith('optimizers/') and '/' in k[11:]}}
                      for r in rows(ck, 'msdn_clip' + c)]
    return {'part': 'divergence', 'batch': 4, 'optimizer': 'momentum', 'clip_norm': out}


def main():
    usage = 'launches, step, parent DIR or divergence'
    part, more = sys.argv[1] if len(sys.argv) > 1 else 'launches', sys.argv[2:]
    if part == 'parent':
        from tools.bench_objective import bench_against_parent
        print(json.dumps(bench_against_parent(more[0], int(more[1]) if len(more) > 1 else 3)))
        return
    if part == 'divergence':
        print(json.dumps(divergence()))
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
