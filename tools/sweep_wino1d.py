"""The sweeps behind the two work-division rules of csrc/wino1d.hip, on conv2d_1 (27 x 37, 96 -> 256, 5 x 5) at B = 8, 16, 32:
the stream-K blocks per plane of bwd-data's products (wino1d_bwd_blocks) and the splits of the filter gradient's pixel axis
(wino1d_grad_splits), each count forced through its tuning switch and timed as tools/bench_layers.py times a row; `rule` is the
unforced call.  Run as a tuning process:
    A3D_TUNING=1 python tools/sweep_wino1d.py > profiles/wino1d_split_sweep.txt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ann3depth_amd import ops  # noqa: E402
from tools.bench_layers import timeit  # noqa: E402

BLOCKS = (32, 48, 56, 64, 72, 96, 128)
SPLITS = (1, 2, 3, 4, 5, 6, 7, 8)


def main():
    assert os.environ.get('A3D_TUNING') == '1', 'the switches are read in tuning processes only'
    h, w, c, k = 27, 37, 96, 256
    for B in (8, 16, 32):
        d = ops.conv_desc(B, h, w, c, k, 5, 5, 1, 'SAME')
        x = torch.randn((B, h, w, c), device='cuda')
        wt = torch.randn((5, 5, c, k), device='cuda') * 0.01
        dz = torch.randn((B, h, w, k), device='cuda')
        dx, dw, db = torch.empty_like(x), torch.empty_like(wt), torch.empty(k, device='cuda')
        pl = ops.PreparedFilter(d, x.device, 'bwd_d_wino1d')
        pl.refresh(wt)
        for name, env, counts, fn in (
                ('bwd_d blocks/plane', 'A3D_WINO1D_BLOCKS', BLOCKS, lambda: ops.conv2d_bwd_data_wino1d(pl.desc_prepared, dz, pl.buf, dx)),
                ('bwd_f splits', 'A3D_WINO1D_GRAD_SPLIT', SPLITS, lambda: ops.conv2d_bwd_filter_wino1d(d, x, dz, dw, db))):
            os.environ.pop(env, None)
            row = [f'rule {timeit(fn):.1f}']
            for n in counts:
                os.environ[env] = str(n)
                row.append(f'{n}: {timeit(fn):.1f}')
            os.environ.pop(env, None)
            print(f'B={B:2d} {name:18s} us  ' + '  '.join(row), flush=True)


if __name__ == '__main__':
    main()
