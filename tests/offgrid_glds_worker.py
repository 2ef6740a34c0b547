"""Child process of tests/test_gpu_exact_offgrid.py::test_forward_on_the_lds_dma_staged_kernel, started with A3D_TUNING=1 and
A3D_FORCE_CFG=9: the forward on the LDS-DMA-staged fp32 kernel (igemm_glds.h), which the planner never picks by itself, with its
operands off the 16-byte grid.  Prints the sweep's ROUTE lines and one `verified` line per case."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import exact_ops as E                       # noqa: E402
import test_gpu_exact_offgrid as T          # noqa: E402


def main():
    from ann3depth_amd import _lib, ops
    assert os.environ.get('A3D_TUNING') == '1' and os.environ.get('A3D_FORCE_CFG') == '9'
    lib = _lib.load()
    smallest = T.lds_dma_forward_case(ops, lib)
    assert smallest is not None, 'no E.GENERIC forward has an on-grid record with lds_dma == 1 under the pinned configuration'
    for case in (smallest, E.OFFGRID_GENERIC[1]):
        T.sweep(lib, T.conv_job(ops, lib, 'conv2d_fwd', case))
        print(f'verified {case}')


if __name__ == '__main__':
    main()
