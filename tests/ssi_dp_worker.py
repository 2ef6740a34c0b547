"""Rank body of tests/test_gpu_ssi_train.py::test_two_ranks_equal_one_rank_on_the_concatenated_batch: two ranks share cuda:0
and reduce over gloo (the tests/dcnf_valid_dp_worker.py pattern).  Every rank builds the same four records with holes; rank k
steps an MSDNReplica(objective='ssi', valid_range=...) under a reducer on records 2k, 2k + 1, one without a reducer on the
same two, and a replica of batch 4 on all four.  The fit is per sample, so a sample's scale, shift and gradient row do not
depend on the batch it is in: two ranks of 2 are one batch of 4, with 1 / 2 against 1 / 4 in front.

    ssi_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ann3depth_amd import dp, models, ops          # noqa: E402
from oracle import msdn as O          # noqa: E402

B = 2
RANGE = (0.0, 0.99)


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (2 * B, 48, 64, 3), dtype=np.uint8)
    dep = rng.integers(1, 255, (2 * B, 48, 64, 1), dtype=np.uint8)
    dep[:, 5:20, 10:30] = 0
    dep[:, 40:, 50:] = 0
    keep = (rng.random((2 * B, 4096)) >= 0.5).astype(np.uint8)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    sl = slice(rank * B, (rank + 1) * B)
    params = O.init_params(3000)
    kw = dict(params=params, beta2=0.999, objective='ssi', valid_range=RANGE)
    whole = models.MSDNReplica(2 * B, **kw)
    whole.step(cu(img), cu(dep), cu(keep))
    solo = models.MSDNReplica(B, **kw)
    solo.step(cu(img[sl]), cu(dep[sl]), cu(keep[sl]))
    net = models.MSDNReplica(B, reducer=dp.GradReducer(), **kw)
    out = net.step(cu(img[sl]), cu(dep[sl]), cu(keep[sl]))
    net.settle()
    torch.cuda.synchronize()
    checks = {}
    # the exchange itself: the gradients are the sums of what the ranks computed alone (two addends: the same bits in any order)
    for gn in ('CoarseConv',):
        total = torch.nn.functional.pad(solo.groups[gn].grad.clone(), (0, net.groups[gn].count - solo.groups[gn].grad.numel()))
        dist.all_reduce(total)
        checks[gn + '_allreduce'] = bool(torch.equal(net.groups[gn].grad, total)) and float(total.abs().sum()) > 0
    # per sample, exactly: the loss launches of a batch of 2 on the batch-of-4 replica's OWN outputs and targets give its rows
    # (times 2: 1 / 2 against 1 / 4), its scales, shifts, counts and flags
    o4, t4 = whole.coarse.view(2 * B, -1), whole.t.view(2 * B, -1)
    ws, loss = ops.ssi_ws(B, 'cuda'), torch.empty(4, device='cuda')
    g = torch.empty((B, o4.shape[1]), device='cuda')
    ops.ssi_loss_fwd(o4[sl].contiguous(), t4[sl].contiguous(), 1, loss, ws)
    ops.ssi_loss_bwd(o4[sl].contiguous(), t4[sl].contiguous(), 1, ws, g)
    torch.cuda.synchronize()
    mine = whole.ws_c[2 + 4 * B * rank:2 + 4 * B * (rank + 1)]
    checks['rows'] = bool(torch.equal((g * 0.5).view(torch.int32), whole.dz1[sl].view(torch.int32))) and float(g.abs().sum()) > 0
    checks['fit'] = bool(torch.equal(ws[2:2 + 4 * B].view(torch.int32), mine.view(torch.int32)))
    fit = net.ws_c[2:2 + 4 * B].view(B, 4)
    checks['counts'] = bool(torch.equal(fit[:, 2:], mine.view(B, 4)[:, 2:])) and bool((fit[:, 3] == 0).all())
    # the rank's own step against the batch of 4: the forward goes through other tiles with the batch (tests/dp_gpu_worker.py),
    # so the outputs differ by eps = max |delta o| / std(o) per sample.  r = s (o - mean o) - (d - mean d) with s = cov / var:
    # such a perturbation moves s (o - mean o) by at most about 3 eps |s| std(o) (o - mean o itself, and s through cov and
    # var), so the loss, the fit and the gradient move by a small multiple of eps of their scale: 8 eps, and 1e-5 for the
    # float32 sums themselves
    delta = (net.coarse.view(B, -1) - o4[sl]).abs().max(dim=1).values
    eps = float((delta / o4[sl].std(dim=1)).max())
    tol = 8 * eps + 1e-5
    checks['dz1'] = float((net.dz1 * 0.5 - whole.dz1[sl]).abs().max()) <= tol * float(whole.dz1[sl].abs().max())
    checks['scale'] = float((fit[:, 0] - mine.view(B, 4)[:, 0]).abs().max()) <= tol * float(mine.view(B, 4)[:, 0].abs().max())
    mean = out['coarse_loss'].clone().cpu()
    dist.all_reduce(mean)
    checks['mean'] = abs(float(mean) / 2 - float(whole.loss_coarse)) <= tol * float(whole.loss_coarse)
    print(f'ssi dp rank {rank}: {checks}, eps {eps:.3g}, losses {float(mean) / 2:.6g} / {float(whole.loss_coarse):.6g}, fit '
          f'{fit.tolist()}', flush=True)
    ok = all(checks.values())
    for grp in net.groups.values():                                        # replicas stay bit-identical
        theirs = grp.var.clone()
        dist.broadcast(theirs, 0)
        ok &= bool(torch.equal(theirs.view(torch.int32), grp.var.view(torch.int32)))
    flag = torch.tensor([int(ok)])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        open(out_path, 'w').write(str(int(flag.item())))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
