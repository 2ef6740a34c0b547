"""Rank body of tests/test_gpu_clip_train.py::test_two_ranks_clip_the_reduced_gradients_to_the_same_bits: two ranks share cuda:0
and reduce over gloo (the tests/momentum_dp_worker.py pattern).  Rank k steps an MSDNReplica(optimizer='momentum', clip_norm=C)
under a reducer on records 2k, 2k + 1 and one without a reducer or a bound on the same two.  C is half the smaller group norm of
the all-reduced gradient at grad_scale 1 / 2, so both groups clip.  After the step, the dense bucket applied in settle() included,
every variable and accumulator is tests/momentum_ref.py on the all-reduced gradient at the scale read back from the group's
control block, that scale within one float32 ulp of tests/clip_ref.py's with gs = 1 / 2, and the replicas and their control
blocks are bit-identical across the ranks.

    clip_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import clip_ref as CR          # noqa: E402
import momentum_ref as MR          # noqa: E402
from ann3depth_amd import dp, models, ops          # noqa: E402
from oracle import msdn as O          # noqa: E402

B = 2
MU = 0.9
COARSE = ('CoarseConv', 'CoarseDense')


def same(a, b):
    a, b = (np.ascontiguousarray(x, np.float32) for x in (a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def within_one_ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return bool(np.nextafter(want, np.float32(-np.inf)) <= got <= np.nextafter(want, np.float32(np.inf)))


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    rng = np.random.default_rng(41)
    img = rng.integers(0, 256, (2 * B, 48, 64, 3), dtype=np.uint8)
    dep = rng.integers(1, 255, (2 * B, 48, 64, 1), dtype=np.uint8)
    keep = (rng.random((2 * B, 4096)) >= 0.5).astype(np.uint8)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    sl = slice(rank * B, (rank + 1) * B)
    kw = dict(params=O.init_params(3000), optimizer='momentum', momentum=MU)
    solo = models.MSDNReplica(B, **kw)
    solo.step(cu(img[sl]), cu(dep[sl]), cu(keep[sl]))
    totals = {}
    for gn in COARSE:
        g = solo.groups[gn].grad
        q = world * models.ParamGroup.ALIGN if gn == 'CoarseDense' else 1     # the dense group is padded for `world` equal slices
        totals[gn] = torch.nn.functional.pad(g.clone(), (0, -(-g.numel() // q) * q - g.numel()))
        dist.all_reduce(totals[gn])
    C = 0.5 * min(0.5 * float(np.sqrt(CR.sumsq(t.cpu().numpy()))) for t in totals.values())
    net = models.MSDNReplica(B, reducer=dp.GradReducer(), clip_norm=C, **kw)
    checks = {'all-reduce, nothing sharded': net.dense_exchange == 'all_reduce' and net.keep_dense_grads}
    before = {gn: (g.var.cpu().numpy(), g.m.cpu().numpy()) for gn, g in net.groups.items()}
    net.step(cu(img[sl]), cu(dep[sl]), cu(keep[sl]))
    checks['the dense bucket is deferred'] = net._deferred is not None
    net.settle()
    torch.cuda.synchronize()
    checks['not sharded'] = not net._m_sharded
    for gn in COARSE:
        g, total = net.groups[gn], totals[gn]
        assert g.count == total.numel(), gn
        checks[gn + ' all-reduce'] = bool(torch.equal(g.grad, total)) and float(total.abs().sum()) > 0
        st, want = ops.clip_read(g.ctl), CR.clip(total.cpu().numpy(), 0.5, C)
        checks[gn + ' scale'] = st.skip == 0 and 0 < st.scale < 0.5 and within_one_ulp(st.scale, want.scale) and \
            within_one_ulp(st.norm, want.norm)
        var, accum = MR.step(before[gn][0], before[gn][1], total.cpu().numpy(), g.lr, MU, st.scale)
        checks[gn + ' accum'] = same(g.m.cpu().numpy(), accum) and bool(np.any(accum != 0))
        checks[gn + ' var'] = same(g.var.cpu().numpy(), var) and not same(var, before[gn][0])
    for gn in ('FineA', 'FineB'):                                            # the coarse phase leaves them alone
        g = net.groups[gn]
        checks[gn + ' untouched'] = same(g.var.cpu().numpy(), before[gn][0]) and not bool(g.m.any())
    print(f'clip dp rank {rank}: C {C:.6g} {checks}', flush=True)
    ok = all(checks.values())
    for grp in net.groups.values():                                        # replicas stay bit-identical, control blocks included
        for buf in (grp.var, grp.m, grp.ctl):
            theirs = buf.clone()
            dist.broadcast(theirs, 0)
            ok &= bool(torch.equal(theirs.view(torch.int32), buf.view(torch.int32)))
    flag = torch.tensor([int(ok)])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        open(out_path, 'w').write(str(int(flag.item())))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
