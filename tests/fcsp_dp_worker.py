"""Rank body of tests/test_gpu_fcsp_train.py::test_two_ranks_stay_identical_and_match_the_one_rank_step: two ranks share
cuda:0 and reduce over gloo (the tests/dcnf_pair_dp_worker.py pattern).  Every rank builds the same two images (white
noise: dcnf_pair_ref's images are tiled or nearly flat by construction, so that thousands of pool windows hold values
that agree to the last bits, and a batch of two, under another tile plan's summation order, picks other positions than
a batch of one in 16 windows of conv2d_4 on the flat image, measured; that moves the gradient by 4e-4 and, as
tests/test_gpu_dcnf.py notes, says nothing about the code under test); rank k
steps a DCNFReplica(1, unary='fcsp') twice on image k, the unary gradients all-reduced and 1 / world folded into the
learning rate, and a one-rank replica steps twice on both images at once (see the loop for how last-bit ties are kept
out of the comparison).

    fcsp_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ann3depth_amd import dp, models          # noqa: E402
from test_gpu_dcnf_pairwise_train import KERNEL, BIAS          # noqa: E402
from test_gpu_fcsp_train import fcsp_params, rel          # noqa: E402


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    ok = True
    params = fcsp_params()
    params[KERNEL], params[BIAS] = np.ones((2, 1), np.float32), np.ones((1,), np.float32)       # r in [1, 3]: a live loss
    solo = models.DCNFReplica(2, params=params, unary='fcsp')
    rng = np.random.default_rng(60)                                        # the same two images on both ranks
    img = torch.from_numpy((rng.integers(0, 256, (2, 240, 320, 3)) / 255).astype(np.float32)).cuda()
    solo.unary.forward(img)
    z = solo.unary.z.view(2, solo.rows, solo.cols).cpu().numpy()
    y = (z + 0.05 * rng.standard_normal(z.shape)).astype(np.float32)       # targets around the current z: a live gradient
    dep = torch.from_numpy(np.ascontiguousarray(np.kron(y, np.ones((40, 40), np.float32))[..., None])).cuda()
    before = solo.unary.group.var.clone()
    net = models.DCNFReplica(1, params=params, unary='fcsp', reducer=dp.GradReducer())
    for step in range(2):
        net.step(img[rank:rank + 1], dep[rank:rank + 1])
        # the one-rank step on both images, taken apart: its forward is held to the ranks' own, then its backward runs on
        # the ranks' activations and pool positions, as tests/test_gpu_dcnf.py does at the baseline size.  A batch of two
        # runs under another tile plan than a batch of one; where two values of a pool window (or a ReLU input and zero)
        # agree to the last bit the two forwards decide differently, which moves a whole gradient element: measured
        # here, ONE such window in conv2d_4 put the weights 1.05e-4 apart after the first step and 2.5e-4 after the second
        solo.forward(img, dep)
        torch.cuda.synchronize()
        flips = {}
        for k in range(world):
            for name, mine in list(net.unary.act.items()) + [('argmax:' + n, t) for n, t in net.unary.argmax.items()]:
                t = mine.clone() if rank == k else torch.empty_like(mine)
                dist.broadcast(t, k)
                theirs = (solo.unary.argmax[name[7:]] if name.startswith('argmax:') else solo.unary.act[name])
                rows = theirs.shape[0] // world
                sl = theirs[k * rows:(k + 1) * rows]
                if name.startswith('argmax:'):
                    flips[name[7:]] = flips.get(name[7:], 0) + int((sl != t).sum())
                else:
                    ok &= rel(sl.cpu().numpy(), t.cpu().numpy()) < (1e-3 if name == 'dense_2' else 1e-4)
                sl.copy_(t)
        print(f'rank {rank} step {step + 1}: pool positions the batch of two chose differently {flips}', flush=True)
        solo.unary.backward(solo.dz)
        solo.unary.group.apply_sgd(1.0)
        solo.global_step += 1
    torch.cuda.synchronize()
    ok &= net.global_step == 2 and not torch.equal(net.unary.group.var, before)
    for g in net.groups.values():                                          # replicas stay bit-identical
        theirs = g.var.clone()
        dist.broadcast(theirs, 0)
        ok &= bool(torch.equal(theirs.view(torch.int32), g.var.view(torch.int32)))
    for n in net.unary.shapes:                                             # ... and took the step of the whole batch
        a = net.unary.group.view(net.unary.group.var, n).cpu().numpy()
        b = solo.unary.group.view(solo.unary.group.var, n).cpu().numpy()
        ok &= rel(a, b) < 1e-4
        moved = rel(a - solo.unary.group.view(before, n).cpu().numpy(), b - solo.unary.group.view(before, n).cpu().numpy())
        print(f'rank {rank} {n}: weights {rel(a, b):.3g}, the two steps themselves {moved:.3g}', flush=True)
    flag = torch.tensor([int(ok)])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        open(out_path, 'w').write(str(int(flag.item())))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
