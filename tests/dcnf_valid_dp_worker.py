"""Rank body of tests/test_gpu_dcnf_valid_train.py::test_two_ranks_equal_one_rank_on_the_concatenated_batch: two ranks
share cuda:0 and reduce over gloo (the tests/dcnf_pair_dp_worker.py pattern).  Every rank builds the same four images with
holes; rank k steps a DCNFReplica(valid_range=..., train_pairwise=True) under a reducer on images 2k, 2k + 1, and a
replica of batch 4 without one on all four.  The likelihood is a sum over images divided by the batch: the two ranks'
all-reduced gradients with 1 / world folded into the learning rate are the batch-of-4 step up to the order of the sums.

    dcnf_valid_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ann3depth_amd import dp, models          # noqa: E402
from test_gpu_dcnf_valid_train import RANGE, cuda, holed_batch, start_params          # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    ok = True
    params = start_params()
    img, dep = cuda(*holed_batch(4, 70))
    whole = models.DCNFReplica(4, params=params, train_pairwise=True, valid_range=RANGE)
    whole.step(img, dep)
    solo = models.DCNFReplica(2, params=params, train_pairwise=True, valid_range=RANGE)
    solo.step(img[2 * rank:2 * rank + 2], dep[2 * rank:2 * rank + 2])
    net = models.DCNFReplica(2, params=params, train_pairwise=True, valid_range=RANGE, reducer=dp.GradReducer())
    out = net.step(img[2 * rank:2 * rank + 2], dep[2 * rank:2 * rank + 2])
    torch.cuda.synchronize()
    checks = {}
    # the exchange itself: both groups' gradients are the sums of what the ranks computed alone (two addends: the same
    # bits in any order), and the ranks did bring different ones
    for name, g, h in (('unary', net.unary.group, solo.unary.group), ('pairwise', net.pair_group, solo.pair_group)):
        total = h.grad.clone()
        dist.all_reduce(total)
        checks[name + '_allreduce'] = bool(torch.equal(g.grad.view(torch.int32), total.view(torch.int32))) and \
            not torch.equal(total, h.grad * 2)
    # the images' own numbers do not depend on the batch they are in, up to the unary stack's z: 96 and 192 patches go
    # through other tiles of the same float32 sums, so the comparisons carry the 1e-4 of the DCNF step tests
    sl = slice(2 * rank, 2 * rank + 2)
    checks['nobs'] = bool(torch.equal(net.nobs, whole.nobs[sl])) and 0 < int(net.nobs.min()) and int(net.nobs.max()) < 48
    checks['status'] = not bool(net.status_observed.any()) and not bool(whole.status_observed.any())
    checks['per_image'] = float((net.loss_per_image - whole.loss_per_image[sl]).abs().max()) <= \
        1e-4 * float(whole.loss_per_image.abs().max())
    checks['dz'] = rel(net.dz * 0.5, whole.dz[sl]) < 1e-4                  # 1 / 2 against 1 / 4
    checks['dr'] = rel(net.dr * 0.5, whole.dr[sl]) < 1e-4
    # the mean of the two ranks' losses is the batch's
    mean = out['mean_loss'].clone().cpu()
    dist.all_reduce(mean)
    checks['mean'] = abs(float(mean) / 2 - float(whole.loss)) <= 1e-4 * float(whole.loss_per_image.abs().max())
    # gradients: all-reduced sums / world against the batch of 4; then the variables.  dz agrees to 1e-4 above and the
    # backward is linear in it, but 96 and 192 patches go through other tiles and split-K factors of five chained conv
    # layers, each feeding its rounding into the next, and nothing holds the batch of 4 to float64 the way the step tests
    # hold 1 and 2 (1e-4 each): 1e-3, ten times that, is room for the order of the sums, not a measured figure
    worst, each = 0.0, {}
    for n in net.unary.shapes:
        g = net.unary.group.view(net.unary.group.grad, n) * 0.5
        w = whole.unary.group.view(whole.unary.group.grad, n)
        if float(w.norm()) > 0:
            each[n] = (round(rel(g, w), 7), float(w.norm()))
            worst = max(worst, rel(g, w))
    print(f'rank {rank} unary gradients (rel, norm): {each}; var rel {rel(net.unary.group.var, whole.unary.group.var):.3g}', flush=True)
    checks['unary_grad'] = worst < 1e-3
    gp, wp = net.pair_group.grad * 0.5, whole.pair_group.grad
    scale = float((whole.dr.abs().unsqueeze(-1) * whole.sims.abs()).sum())
    checks['pair_grad'] = float((gp - wp).abs().max()) <= 1e-4 * scale and float(wp.abs().max()) > 0
    gnorm, vnorm = float(whole.unary.group.grad.double().norm()), float(whole.unary.group.var.double().norm())
    checks['unary_var'] = rel(net.unary.group.var, whole.unary.group.var) <= 0.1 * 1e-3 * gnorm / vnorm + 2.0 ** -22
    checks['pair_var'] = float((net.pair_group.var - whole.pair_group.var).abs().max()) <= 0.1 * 1e-4 * scale + 2.0 ** -22 \
        and bool((net.pair_group.var >= 0).all())
    print(f'dcnf valid dp rank {rank}: {checks}, worst unary gradient {worst:.3g}, losses {net.loss_per_image.tolist()} / '
          f'{whole.loss_per_image[sl].tolist()}', flush=True)
    ok = all(checks.values())
    for g in net.groups.values():                                          # replicas stay bit-identical, both groups
        theirs = g.var.clone()
        dist.broadcast(theirs, 0)
        ok &= bool(torch.equal(theirs.view(torch.int32), g.var.view(torch.int32)))
    flag = torch.tensor([int(ok)])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        open(out_path, 'w').write(str(int(flag.item())))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
