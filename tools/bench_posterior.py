"""a3dc_crf_band_posterior (include/a3d_posterior.h) on one MI355X: the launch alone at batch 16 on the three DCNF grids
(6 x 8, 12 x 16, 24 x 32 superpixels, the model's pair lists), with and without var, with 0 %, 50 % and 100 % of the
superpixels observed, beside a3db_crf_band_map on the same z and r in the same process, and as a share of
DCNFReplica.posterior() on 480 x 640 images (the patch unary at 6 x 8, the fully convolutional one on the finer grids).

Every figure is one HIP event pair around one call: two warm-up calls, ten timed calls, reported as the mean with the
fastest and the slowest.  There is no target time; this states what was measured.

    python tools/bench_posterior.py [batch]          # writes profiles/bench_posterior.json and prints it"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ann3depth_amd import models, ops  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
WARMUP, CALLS = 2, 10


def timed(fn):
    """-> {'mean_ms', 'min_ms', 'max_ms'} of CALLS calls, each between its own pair of events."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
    return {'mean_ms': round(float(np.mean(ms)), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def main():
    rng = np.random.default_rng(1000)
    img = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3)).astype(np.uint8)).cuda()
    grids = []
    for sp in models.DCNF_SUPERPIXELS:
        rep = models.DCNFReplica(B, unary='patch' if sp == models.DCNF_SP else 'fcsp', superpixel=sp)
        nsp, band = rep.nsp, rep.band
        z = torch.from_numpy(rng.uniform(0.2, 1.0, (B, nsp)).astype(np.float32)).cuda()
        r = torch.from_numpy(rng.uniform(0.0, 2.0, (B, rep.left.numel())).astype(np.float32)).cuda()
        y_full = rng.uniform(0.2, 1.0, (B, nsp)).astype(np.float32)
        mean, var = torch.empty_like(z), torch.empty_like(z)
        mu, st = torch.empty_like(z), torch.empty((B,), dtype=torch.int32, device='cuda')
        row = {'grid': [rep.rows, rep.cols], 'superpixels': nsp, 'band': band, 'pairs': int(rep.left.numel()),
               'lds_bytes_per_workgroup': (nsp * ((band + 2) & ~1) + 3 * nsp) * 4, 'workgroups': B,
               'threads_per_workgroup': 256,
               'map': timed(lambda: ops.crf_band_map(z, r, rep.left, rep.right, band, mu, st)), 'posterior': {}}
        for share in (0.0, 0.5, 1.0):
            y = np.where(rng.random((B, nsp)) < share, y_full, np.float32(np.nan)).astype(np.float32)
            yd = torch.from_numpy(y).cuda()
            with_var = timed(lambda: ops.crf_band_posterior(z, yd, r, rep.left, rep.right, band, True, mean, var))
            no_var = timed(lambda: ops.crf_band_posterior(z, yd, r, rep.left, rep.right, band, False, mean))
            _, _, nobs, status = ops.crf_band_posterior(z, yd, r, rep.left, rep.right, band, True, mean, var)
            row['posterior'][f'observed_{int(share * 100)}'] = {
                'observed_fraction': round(float(nobs.sum().item()) / (B * nsp), 4), 'rejected': int(status.sum().item()),
                'with_var': with_var, 'without_var': no_var}
        whole = timed(lambda: rep.posterior(img))
        launch = row['posterior']['observed_0']['with_var']['mean_ms']
        row['replica_posterior'] = dict(whole, unary=rep.unary_form, launch_share=round(launch / whole['mean_ms'], 4))
        grids.append(row)
        del rep
        torch.cuda.empty_cache()
    out = {'workload': f'a3dc_crf_band_posterior, batch {B}, one workgroup of 256 threads per image',
           'device': torch.cuda.get_device_name(0), 'warmup_calls': WARMUP, 'timed_calls': CALLS,
           'timing': 'one HIP event pair per call; mean, fastest and slowest of the timed calls', 'grids': grids}
    path = os.path.join(ROOT, 'profiles', 'bench_posterior.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
