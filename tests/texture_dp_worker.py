"""Rank body of tests/test_gpu_texture_train.py::test_two_ranks_keep_the_four_pairwise_values_bit_identical: two ranks
share cuda:0 and reduce over gloo (the tests/dcnf_pair_dp_worker.py pattern).  Each rank steps a
DCNFReplica(train_pairwise=True, pairwise_texture=True) on its own two images; the three kernel gradients and the bias
gradient are all-reduced like the unary group's and descend with 1 / world folded into the learning rate.

    texture_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import crf_pair_grad_ref as G                 # noqa: E402
from ann3depth_amd import dp, models          # noqa: E402
from test_gpu_dcnf_pairwise_train import batch_for          # noqa: E402
from test_gpu_texture_train import start_params3            # noqa: E402


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    B, ok = 2, True
    params = start_params3()
    solo = models.DCNFReplica(B, params=params, train_pairwise=True, pairwise_texture=True)
    img, dep = batch_for(solo, B, seed=50 + rank)                          # another batch on each rank
    before = solo.pair_group.var.clone()
    solo.step(img, dep)
    net = models.DCNFReplica(B, params=params, train_pairwise=True, pairwise_texture=True, reducer=dp.GradReducer())
    net.step(img, dep)
    torch.cuda.synchronize()
    total = solo.pair_group.grad.clone()
    dist.all_reduce(total)                                                 # two addends: the same bits in any order
    ok &= bool(torch.equal(net.pair_group.grad.view(torch.int32), total.view(torch.int32)))
    ok &= bool((total[[0, 1, 2, 64]] != 0).all())                          # all four values have a gradient
    want = G.sgd_floor32(before.cpu().numpy(), total.cpu().numpy(), 0.1 * (1.0 / world), 0.0)
    ok &= bool(np.array_equal(net.pair_group.var.cpu().numpy().view(np.uint32), want.view(np.uint32)))
    ok &= bool((net.pair_group.var[[0, 1, 2, 64]] != before[[0, 1, 2, 64]]).all())
    ok &= tuple(net.pair_var('kernel').shape) == (3, 1)
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
