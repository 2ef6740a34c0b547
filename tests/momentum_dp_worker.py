"""Rank body of tests/test_gpu_momentum_train.py::test_two_ranks_apply_the_rule_to_the_reduced_gradients: two ranks share cuda:0
and reduce over gloo (the tests/ssi_dp_worker.py pattern).  Rank k steps an MSDNReplica(optimizer='momentum') under a reducer on
records 2k, 2k + 1 and one without a reducer on the same two.  The reduced conv and dense gradients are the sums of what the
ranks computed alone; after the step every variable and accumulator is tests/momentum_ref.py on the all-reduced gradient with
grad_scale = 1 / 2, bit for bit, and the replicas are bit-identical across the ranks.

    momentum_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import momentum_ref as MR          # noqa: E402
from ann3depth_amd import dp, models          # noqa: E402
from oracle import msdn as O          # noqa: E402

B = 2
MU = 0.9


def same(a, b):
    a, b = (np.ascontiguousarray(x, np.float32) for x in (a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


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
    net = models.MSDNReplica(B, reducer=dp.GradReducer(), **kw)
    assert net.dense_exchange is not None and net.keep_dense_grads
    before = {gn: (g.var.cpu().numpy(), g.m.cpu().numpy()) for gn, g in net.groups.items()}
    net.step(cu(img[sl]), cu(dep[sl]), cu(keep[sl]))
    net.settle()
    torch.cuda.synchronize()
    checks = {'not sharded': not net._m_sharded and all(g.v is None for g in net.groups.values())}
    for gn in ('CoarseConv', 'CoarseDense'):
        g = net.groups[gn]
        # the exchange itself: the gradients are the sums of what the ranks computed alone (two addends: the same bits in any order)
        total = torch.nn.functional.pad(solo.groups[gn].grad.clone(), (0, g.count - solo.groups[gn].grad.numel()))
        dist.all_reduce(total)
        checks[gn + ' all-reduce'] = bool(torch.equal(g.grad, total)) and float(total.abs().sum()) > 0
        var, accum = MR.step(before[gn][0], before[gn][1], total.cpu().numpy(), g.lr, MU, 0.5)
        checks[gn + ' accum'] = same(g.m.cpu().numpy(), accum) and bool(np.any(accum != 0))
        checks[gn + ' var'] = same(g.var.cpu().numpy(), var) and not same(var, before[gn][0])
    for gn in ('FineA', 'FineB'):                                            # the coarse phase leaves them alone
        g = net.groups[gn]
        checks[gn + ' untouched'] = same(g.var.cpu().numpy(), before[gn][0]) and not bool(g.m.any())
    print(f'momentum dp rank {rank}: {checks}', flush=True)
    ok = all(checks.values())
    for grp in net.groups.values():                                        # replicas stay bit-identical
        for buf in (grp.var, grp.m):
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
