"""Rank body of tests/test_gpu_dcnf_superpixel.py::test_two_ranks_match_a_batch_of_four_at_20: two ranks share cuda:0 and
reduce over gloo (the tests/fcsp_dp_worker.py pattern, whose docstring says why the images are white noise and how last-bit
pool ties are kept out of the comparison).  Every rank builds the same four images; rank k steps a
DCNFReplica(2, unary='fcsp', superpixel=20) twice on images 2k, 2k + 1, the unary gradients all-reduced and 1 / world folded
into the learning rate, and a one-rank replica of batch 4 steps twice on all four.  The banded likelihood's dz carries 1 / 2
on a rank and 1 / 4 in the batch of four: the all-reduce's 1 / world makes them the same step.

    superpixel_dp_worker.py OUT        writes '1' when every check held on every rank"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ann3depth_amd import dp, models          # noqa: E402
from test_gpu_dcnf_superpixel import rel, start_params          # noqa: E402

SP, PER_RANK = 20, 2


def main(out_path):
    rank, local_rank, world = dp.init_from_env()
    assert world == 2 and dist.get_backend() == 'gloo'
    ok = True
    params = start_params()
    total = world * PER_RANK
    solo = models.DCNFReplica(total, params=params, unary='fcsp', superpixel=SP)
    rng = np.random.default_rng(61)                                        # the same four images on both ranks
    img = torch.from_numpy((rng.integers(0, 256, (total, 240, 320, 3)) / 255).astype(np.float32)).cuda()
    solo.unary.forward(img)
    z = solo.unary.z.view(total, solo.rows, solo.cols).cpu().numpy()
    y = (z + 0.05 * rng.standard_normal(z.shape)).astype(np.float32)       # targets around the current z: a live gradient
    dep = torch.from_numpy(np.ascontiguousarray(np.kron(y, np.ones((SP, SP), np.float32))[..., None])).cuda()
    before = solo.unary.group.var.clone()
    net = models.DCNFReplica(PER_RANK, params=params, unary='fcsp', superpixel=SP, reducer=dp.GradReducer())
    mine = slice(rank * PER_RANK, (rank + 1) * PER_RANK)
    for step in range(2):
        net.step(img[mine], dep[mine])
        # the one-rank step on all four images, taken apart as tests/fcsp_dp_worker.py does: its forward is held to the
        # ranks' own, then its backward runs on the ranks' activations and pool positions
        solo.forward(img, dep)
        torch.cuda.synchronize()
        ok &= not bool(net.status.any()) and not bool(solo.status.any())
        flips = {}
        for k in range(world):
            for name, own in list(net.unary.act.items()) + [('argmax:' + n, t) for n, t in net.unary.argmax.items()]:
                t = own.clone() if rank == k else torch.empty_like(own)
                dist.broadcast(t, k)
                theirs = (solo.unary.argmax[name[7:]] if name.startswith('argmax:') else solo.unary.act[name])
                rows = theirs.shape[0] // world
                sl = theirs[k * rows:(k + 1) * rows]
                if name.startswith('argmax:'):
                    flips[name[7:]] = flips.get(name[7:], 0) + int((sl != t).sum())
                else:
                    ok &= rel(sl.cpu().numpy(), t.cpu().numpy()) < (1e-3 if name == 'dense_2' else 1e-4)
                sl.copy_(t)
        # dz of the batch of four from the ranks' z: the banded likelihood again, now that z is the ranks' own
        solo.forward_crf(dep)
        for k in range(world):
            t = net.dz.clone() if rank == k else torch.empty_like(net.dz)
            dist.broadcast(t, k)
            ok &= rel(solo.dz[k * PER_RANK:(k + 1) * PER_RANK].cpu().numpy() * world, t.cpu().numpy()) < 1e-5
        print(f'rank {rank} step {step + 1}: pool positions the batch of four chose differently {flips}', flush=True)
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
