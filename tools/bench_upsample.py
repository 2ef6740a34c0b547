"""ops.joint_bilateral_upsample on one GPU, beside the launch it replaces (ops.resize_bilinear_tf1 to the same output size,
in the same process): the two shapes the models produce, float32 and uint8 guides, R = 1, 2, 4.  Each call is timed by a
pair of events of its own, two warm-up and ten timed calls; reported are the mean and the fastest and slowest call, the
ratio to the bilinear resize, and the bytes the call has to move (guide and depth in, depth map out) per second beside
HBM's 8 TB/s.  Then the forward pass the upsampling follows (predict() at the same batch), and with `--evaluate N` the
evaluation loop's wall time over a synthetic NYU-shaped split of N records with and without --upsample joint, once each
after a warming pass.
    python tools/bench_upsample.py [--evaluate 320] > profiles/bench_upsample.json"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import data, evaluate, models, ops  # noqa: E402
from bench_eval import remove_shard, write_shard  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
WARMUP, CALLS = 2, 10
# (name, n, gh, gw, H, W, kind, sp)
SHAPES = [('msdn_b32_55x74_to_480x640', 32, 55, 74, 480, 640, 'corner', None),
          ('dcnf_b16_24x32_to_240x320', 16, 24, 32, 240, 320, 'block', 10)]


def timed(fn):
    """(mean, min, max) ms over CALLS calls, each between two events of its own, after WARMUP calls."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    marks = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        marks.append((a, b))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in marks]
    return sum(ms) / len(ms), min(ms), max(ms)


def kernel_rows(rng):
    rows = []
    for name, n, gh, gw, H, W, kind, sp in SHAPES:
        depth = torch.from_numpy(rng.uniform(0.5, 9, (n, gh, gw)).astype(np.float32)).cuda()
        k = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
        guides = {'float32': torch.from_numpy(k.astype(np.float32) / np.float32(255)).cuda(), 'uint8': torch.from_numpy(k).cuda()}
        tables = ops.UpsampleMap(gh, gw, H, W, kind, sp)
        out = torch.empty((n, H, W), device='cuda')
        out4 = out.view(n, H, W, 1)
        base = timed(lambda: ops.resize_bilinear_tf1(depth.view(n, gh, gw, 1), out4))
        base_bytes = n * (H * W + gh * gw) * 4
        rows.append({'shape': name, 'op': 'resize_bilinear_tf1', 'ms': round(base[0], 5), 'ms_min': round(base[1], 5),
                     'ms_max': round(base[2], 5), 'bytes': base_bytes,
                     'share_of_hbm_peak': round(base_bytes / (base[0] * 1e-3) / HBM_BYTES_PER_S, 4)})
        for gname, guide in guides.items():
            for R in (1, 2, 4):
                t = timed(lambda: ops.joint_bilateral_upsample(depth, guide, tables, R, out=out))
                nbytes = n * (H * W * (4 + 3 * guide.element_size()) + gh * gw * 4)
                rows.append({'shape': name, 'op': 'joint_bilateral_upsample', 'guide': gname, 'radius': R,
                             'ms': round(t[0], 5), 'ms_min': round(t[1], 5), 'ms_max': round(t[2], 5),
                             'ratio_to_bilinear': round(t[0] / base[0], 2), 'bytes': nbytes,
                             'bytes_per_s': round(nbytes / (t[0] * 1e-3), 0),
                             'share_of_hbm_peak': round(nbytes / (t[0] * 1e-3) / HBM_BYTES_PER_S, 4),
                             'exp_per_s': round(n * H * W * (2 * R + 1) ** 2 / (t[0] * 1e-3), 0)})
    return rows


def predict_rows(rng):
    """The forward pass the upsampling follows, from resident uint8 batches of 480 x 640 images."""
    rows = []
    for name, B, make in (('msdn', 32, lambda: models.MSDNReplica(32, device='cuda:0', keep_dense_grads=False)),
                          ('dcnf_fcsp_sp10', 16, lambda: models.DCNFReplica(16, device='cuda:0', unary='fcsp', superpixel=10))):
        net = make()
        img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
        t = timed(lambda: net.predict(img))
        rows.append({'model': name, 'batch': B, 'predict_ms': round(t[0], 4), 'predict_ms_min': round(t[1], 4),
                     'predict_ms_max': round(t[2], 4)})
        del net
        torch.cuda.empty_cache()
    return rows


def evaluate_walls(n_records, rng):
    """Wall seconds of the evaluation loop (EvalOp + Evaluator, msdn, batch 32, grid targets) over a synthetic split, without
    and with the third output; one pass each after a pass that warms the shard's pages and the pinned allocator."""
    B = 32
    root = write_shard(n_records, rng)
    net = models.MSDNReplica(B, device='cuda:0', keep_dense_grads=False)
    out = {'records': n_records, 'batch': B, 'model': 'msdn'}
    for name, up in (('warm', None), ('without', None), ('with_upsample_joint', ops.JointUpsampler('corner'))):
        ev = evaluate.Evaluator(net, 'grid', upsample=up)
        inputs, _ = data.inputs(root, 'nyu', B, 'test', shuffle=False)
        t0 = time.perf_counter()
        op = evaluate.EvalOp(inputs.pipeline, B, net.device)
        while True:
            try:
                op.run(ev)
            except data.OutOfRangeError:
                break
        ev.results()
        wall = time.perf_counter() - t0
        inputs.pipeline.close()
        if name != 'warm':
            out[f'wall_s_{name}'] = round(wall, 3)
    remove_shard(root)
    return out


def main():
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'warmup_calls': WARMUP, 'timed_calls': CALLS,
           'hbm_peak_bytes_per_s': HBM_BYTES_PER_S, 'kernel': kernel_rows(rng), 'predict': predict_rows(rng)}
    if '--evaluate' in sys.argv:
        out['evaluate'] = evaluate_walls(int(sys.argv[sys.argv.index('--evaluate') + 1]), rng)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
