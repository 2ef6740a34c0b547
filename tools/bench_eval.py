"""Evaluation's costs on one GPU: MSDNReplica.predict from resident batches, ops.depth_metrics at the model grid and at
full record resolution (achieved GB/s), and the evaluation loop end to end (ordered reader -> pinned -> H2D -> predict ->
metrics) on a synthetic converter-written test shard, as a fraction of the resident predict rate.
    python tools/bench_eval.py [n_records] > profiles/bench_eval.json
With `dcnf` as the second argument, the same for DCNF at batch 16 (BASELINE config 4's batch): DCNFReplica.predict, its
parts that are not the unary stack (ops.crf_map alone, at 16 and 64 images, and the pairwise features), the objective,
and the loop end to end.
    python tools/bench_eval.py 320 dcnf > profiles/bench_eval_dcnf.json
With `--align MODE` (median, scale, affine or all; include/a3d_align.h) instead: the align launches and
a3da_depth_metrics_aligned beside a3d_depth_metrics on the same inputs, batch 32, targets 55 x 74 and 480 x 640, in rounds
that alternate the calls; `--parent-lib PATH` adds the a3d_depth_metrics of another build of liba3d.so (the parent commit's)
to every round and says whether this build's median lies inside that build's own spread.
    python tools/bench_eval.py --align all --parent-lib ../parent/ann3depth_amd/liba3d.so > profiles/bench_eval_align.json"""
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import data, evaluate, models, ops, tfrecord  # noqa: E402


def timed(fn, iters=20, warmup=3):
    """Mean ms per call from events around `iters` back-to-back calls on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def write_shard(n_records, rng):
    """A converter-written NYU-shaped test shard in /dev/shm; returns the data directory."""
    root = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    os.makedirs(os.path.join(root, 'nyu'))
    img = rng.integers(0, 256, (480, 640, 3)).astype(np.float32) / np.float32(255) - np.float32(.5)
    dep = rng.integers(0, 256, (480, 640, 1)).astype(np.float32) / np.float32(255) - np.float32(.5)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'test.tfrecords')) as w:
        for _ in range(n_records):
            w.write_example(img, dep)
    return root


def remove_shard(root):
    for f in os.listdir(os.path.join(root, 'nyu')):
        os.remove(os.path.join(root, 'nyu', f))
    os.rmdir(os.path.join(root, 'nyu'))
    os.rmdir(root)


def loop_rates(root, B, net, ev):
    """The driver's loop (EvalOp + the model's evaluator) over the shard: images per second of the whole pass (pool
    allocation and the first batch's decode included) and of the batches after the first."""
    inputs, _ = data.inputs(root, 'nyu', B, 'test', shuffle=False)
    t0 = time.perf_counter()
    op = evaluate.EvalOp(inputs.pipeline, B, net.device)      # (allocates and pins the staging pool)
    op.run(ev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    while True:
        try:
            op.run(ev)
        except data.OutOfRangeError:
            break
    ev.results()
    t2 = time.perf_counter()
    inputs.pipeline.close()
    return sum(ev.counts) / (t2 - t0), (sum(ev.counts) - ev.counts[0]) / (t2 - t1)


def main_dcnf(n_records):
    B = 16
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'model': 'dcnf', 'batch': B}
    net = models.DCNFReplica(B, device='cuda:0')
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    dep = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 1)).astype(np.uint8)).cuda()
    predict_ms = timed(lambda: net.predict(img))
    out[f'predict_ms_b{B}'] = round(predict_ms, 4)
    out[f'predict_images_per_s_b{B}'] = round(B / predict_ms * 1e3, 1)
    out[f'nll_us_b{B}'] = round(timed(lambda: net.nll(dep, B), iters=100, warmup=10) * 1e3, 2)
    u = net.unary

    def pairwise():
        ops.superpixel_hist(u.resized, models.DCNF_SP, net.hist)
        ops.pair_similarity(u.resized, models.DCNF_SP, net.hist, net.left, net.right, net.pair_var('kernel'),
                            net.pair_var('bias'), models.DCNF_GAMMA)
    out[f'pairwise_us_b{B}'] = round(timed(pairwise, iters=200, warmup=10) * 1e3, 2)
    for n in (B, 64):                 # a3d_crf_map alone: one wavefront per image; pair weights as the layer produces them
        z = torch.from_numpy(rng.standard_normal((n, net.nsp)).astype(np.float32)).cuda()
        r = torch.from_numpy(rng.uniform(-0.1, 0.7, (n, net.left.numel())).astype(np.float32)).cuda()
        y = torch.empty_like(z)
        status = torch.empty((n,), dtype=torch.int32, device='cuda')
        us = timed(lambda: ops.crf_map(z, r, net.left, net.right, y, status), iters=500, warmup=20) * 1e3
        out[f'crf_map_us_b{n}'] = round(us, 2)
        if n == B:
            out[f'crf_map_share_of_predict_b{B}'] = round(us * 1e-3 / predict_ms, 5)
    root = write_shard(n_records, rng)
    for res in ('grid', 'grid', 'record'):           # the first pass warms the shard's pages and the pinned allocator
        rate_all, rate = loop_rates(root, B, net, evaluate.DCNFEvaluator(net, res))
        out[f'evaluate_images_per_s_b{B}_{res}_whole_pass'] = round(rate_all, 1)
        out[f'evaluate_images_per_s_b{B}_{res}'] = round(rate, 1)
        out[f'evaluate_fraction_of_resident_predict_b{B}_{res}'] = round(rate / (B / predict_ms * 1e3), 3)
    out['evaluate_records'] = n_records
    out['reader_threads'] = data.default_reader_threads()
    remove_shard(root)
    print(json.dumps(out))


def main_align(mode, parent_path, rounds=9, iters=200):
    from ann3depth_amd import _lib
    B = 32
    rng = np.random.default_rng(0)
    lib = _lib.load()
    parent = None
    if parent_path:
        parent = ctypes.CDLL(parent_path)
        for name in ('a3d_depth_metrics_ws_bytes', 'a3d_depth_metrics'):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    modes = ops.ALIGN_MODES if mode == 'all' else (mode,)
    pred = torch.from_numpy(rng.uniform(0.1, 9, (B, 55, 74)).astype(np.float32)).cuda()
    cases = {'grid_f32': torch.from_numpy(rng.uniform(0.1, 9, (B, 55, 74)).astype(np.float32)).cuda(),
             'record_u8': torch.from_numpy(rng.integers(0, 256, (B, 480, 640)).astype(np.uint8)).cuda(),
             'record_f32': torch.from_numpy(rng.uniform(0.1, 9, (B, 480, 640)).astype(np.float32)).cuda()}
    rows = {k: torch.zeros((B, len(ops.METRIC_COLUMNS)), dtype=torch.float64, device='cuda') for k in ('parent', 'plain', 'aligned')}
    coef = torch.empty((B, 2), dtype=torch.float32, device='cuda')
    count = torch.empty(B, dtype=torch.int32, device='cuda')
    status = torch.empty(B, dtype=torch.int32, device='cuda')
    ws = torch.empty(64 << 20, dtype=torch.uint8, device='cuda')
    P, stream = ops._ptr, ops._stream
    out = {'device': torch.cuda.get_device_name(0), 'batch': B, 'rounds': rounds, 'iters_per_round': iters,
           'unit': 'microseconds per call, events around back-to-back calls; median [min, max] over the rounds',
           'parent_lib': bool(parent)}

    def stats(v):
        return {'median': round(float(np.median(v)), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}

    for name, tgt in cases.items():
        th, tw = tgt.shape[1:]
        head = (B, 55, 74, P(pred), th, tw, P(tgt), int(tgt.dtype == torch.uint8), 0.0, float('inf'))

        def metrics(l, r):
            return lambda: ops.check(l.a3d_depth_metrics(*head, 1e-3, float('inf'), P(r), P(ws), ws.numel(), stream()), 'metrics')

        def aligned():
            ops.check(lib.a3da_depth_metrics_aligned(*head, 1e-3, float('inf'), P(coef), P(rows['aligned']), P(ws), ws.numel(),
                                                     stream()), 'aligned')

        def align(m):
            return lambda: ops.check(lib.a3da_depth_align(*head, m, P(coef), P(count), P(status), P(ws), ws.numel(), stream()),
                                     'align')
        calls = {'depth_metrics': metrics(lib, rows['plain']), 'depth_metrics_aligned': aligned}
        if parent is not None:
            calls = {'parent_depth_metrics': metrics(parent, rows['parent']), **calls}
        calls.update({f'depth_align_{m}': align(ops.ALIGN_MODES.index(m)) for m in modes})
        align(ops.ALIGN_MODES.index(modes[-1]))()                      # coefficients for the aligned launch
        us = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                us[k].append(timed(fn, iters=iters, warmup=10) * 1e3)
        res = {k: stats(v) for k, v in us.items()}
        if parent is not None:
            torch.cuda.synchronize()
            res['same_bits_as_parent'] = bool(torch.equal(rows['plain'].view(torch.int64), rows['parent'].view(torch.int64)))
            lo, hi = res['parent_depth_metrics']['min'], res['parent_depth_metrics']['max']
            res['plain_median_inside_parent_spread'] = bool(lo <= res['depth_metrics']['median'] <= hi)
        for m in modes:
            res[f'depth_align_{m}_over_depth_metrics'] = round(res[f'depth_align_{m}']['median'] / res['depth_metrics']['median'], 2)
        out[name] = res
    print(json.dumps(out))


def main():
    if '--align' in sys.argv:
        mode = sys.argv[sys.argv.index('--align') + 1]
        if mode not in ops.ALIGN_MODES + ('all',):
            sys.exit(f'--align {mode}: one of {ops.ALIGN_MODES + ("all",)}')
        parent = sys.argv[sys.argv.index('--parent-lib') + 1] if '--parent-lib' in sys.argv else ''
        return main_align(mode, parent)
    n_records = int(sys.argv[1]) if len(sys.argv) > 1 else 320
    if len(sys.argv) > 2 and sys.argv[2] == 'dcnf':
        return main_dcnf(n_records)
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0)}
    predict_ms = {}
    for B, prec in ((32, 'fp32'), (64, 'bf16s')):
        net = models.MSDNReplica(B, device='cuda:0', precision=prec)
        img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
        ms = timed(lambda: net.predict(img))
        predict_ms[(B, prec)] = ms
        out[f'predict_ms_b{B}_{prec}'] = round(ms, 4)
        out[f'predict_images_per_s_b{B}_{prec}'] = round(B / ms * 1e3, 1)
        del net
        torch.cuda.empty_cache()
    B = 32
    pred = torch.from_numpy(rng.uniform(0.1, 9, (B, 55, 74)).astype(np.float32)).cuda()
    rows = torch.empty((B, len(ops.METRIC_COLUMNS)), dtype=torch.float64, device='cuda')
    cases = {'grid_f32': torch.from_numpy(rng.uniform(0.1, 9, (B, 55, 74)).astype(np.float32)).cuda(),
             'record_u8': torch.from_numpy(rng.integers(0, 256, (B, 480, 640)).astype(np.uint8)).cuda(),
             'record_f32': torch.from_numpy(rng.uniform(0.1, 9, (B, 480, 640)).astype(np.float32)).cuda()}
    for name, tgt in cases.items():
        ms = timed(lambda: ops.depth_metrics(pred, tgt, rows=rows), iters=200, warmup=10)
        nbytes = tgt.numel() * tgt.element_size() + pred.numel() * 4
        out[f'depth_metrics_us_b{B}_{name}'] = round(ms * 1e3, 2)
        out[f'depth_metrics_GBps_b{B}_{name}'] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        out[f'depth_metrics_share_of_predict_b{B}_{name}'] = round(ms / predict_ms[(32, 'fp32')], 4)
    # end to end: the driver's loop (EvalOp + Evaluator) on a converter-written NYU-shaped test shard in /dev/shm
    root = write_shard(n_records, rng)
    net = models.MSDNReplica(B, device='cuda:0')
    for res in ('grid', 'grid', 'record'):           # the first pass warms the shard's pages and the pinned allocator
        rate_all, rate = loop_rates(root, B, net, evaluate.Evaluator(net, res))
        out[f'evaluate_images_per_s_b{B}_{res}_whole_pass'] = round(rate_all, 1)
        out[f'evaluate_images_per_s_b{B}_{res}'] = round(rate, 1)
        out[f'evaluate_fraction_of_resident_predict_b{B}_{res}'] = round(rate / (B / predict_ms[(32, 'fp32')] * 1e3), 3)
    out['evaluate_records'] = n_records
    out['reader_threads'] = data.default_reader_threads()
    remove_shard(root)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
