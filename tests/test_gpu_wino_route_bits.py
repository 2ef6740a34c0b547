"""The Winograd routes after their plane-batched GEMM launch, product builder and workspace carve were written once: every route
leaves the bits it left before, and every workspace query answers the bytes it answered before
(tests/golden/wino_route_bits.json, recorded twice on the parent's library with equal entries).  The cases are those of
tests/wino_ref.py (the forward, bwd-data, the filter gradient and the chain, which wino_grad_ref.py shares) and of
tests/wino1d_ref.py, on the seeded operands of tests/test_gpu_wino_bwd.py and wino1d_ref.operands.  Equality is exact: no
launch's grid, tile, split count, sum order or workspace layout differs."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import wino1d_ref as W1
import wino_ref as W
from test_gpu_wino1d import desc_of, padded
from test_gpu_wino_bwd import POOLED, Problem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wino_route_bits.json')
GUARD = 7.0
CASES_2D = {'2d:' + 'x'.join(map(str, c[:6])) + ('' if c[6] is None else ':guard'): c for c in W.CASES}
CASES_1D = {'1d:' + W1.case_id(c) + ('' if c[7] is None else ':guard'): c for c in W1.CASES}
POOL_CASE = POOLED[0]
NAMES = list(CASES_2D) + list(CASES_1D) + ['2d:pool']


def sha(*tensors):
    """one digest per tensor, guard columns included"""
    torch.cuda.synchronize()
    return [hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for t in tensors]


def full(*shape):
    return torch.full(shape, GUARD, device='cuda')


def observe_2d(case):
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    n, h, w, c, k = case[:5]
    p = Problem(case)
    bias = torch.from_numpy(np.random.default_rng(61).standard_normal(k).astype(np.float32)).cuda()
    pf = ops.PreparedFilter(p.dw_, p.x.device)
    assert pf.ok
    pf.refresh(p.g)
    out = {}
    q = lambda fn, d, *a: int(fn(ctypes.byref(d), *a))      # noqa: E731
    out['ws'] = {
        'fwd': [q(lib.a3d_conv2d_fwd_ws_bytes, p.dw_), q(lib.a3d_conv2d_fwd_ws_bytes, pf.desc_prepared)],
        'bwd_data': [q(lib.a3d_conv2d_bwd_data_ws_bytes, p.dw_), q(lib.a3d_conv2d_bwd_data_ws_bytes, p.pb.desc_prepared)],
        'bwd_filter': q(lib.a3dwg_conv2d_bwd_filter_ws_bytes, p.d),
        'chain': [q(lib.a3dwb_conv2d_bwd_ws_bytes, p.dw_, 0, 0), q(lib.a3dwb_conv2d_bwd_ws_bytes, p.pb.desc_prepared, 1, 0)],
        'prepared': [q(lib.a3d_conv2d_fwd_prepared_filter_bytes, p.dw_), q(lib.a3dw_conv2d_bwd_data_prepared_filter_bytes, p.dw_)],
    }
    for tag, (d, f) in (('per_call', (p.dw_, p.g)), ('prepared', (pf.desc_prepared, pf.buf))):
        y = full(n, p.d.ho, p.d.wo, p.ldy)
        ops.conv2d_fwd(d, p.x, f, bias, y, 'relu')
        out['fwd:' + tag] = sha(y)
    for prepared in (False, True):
        d, f = p.filter(prepared)
        for mask in (False, True):
            dx = full(n, h, w, p.ldx)
            ops.conv2d_bwd_data(d, p.dz, f, dx, relu_mask=p.mask if mask else None)
            out[f'bwd_data:prepared={int(prepared)}:mask={int(mask)}'] = sha(dx)
            dw, db, dx = p.chain(prepared, mask)
            out[f'chain:prepared={int(prepared)}:mask={int(mask)}'] = sha(dw, db, dx)
    for want_db in (True, False):
        dw, db = full(3, 3, c, k), full(k)
        ops.conv2d_bwd_filter_wino(p.d, p.x, p.dz, dw, db if want_db else None)
        out[f'bwd_filter:db={int(want_db)}'] = sha(dw, db)
    return out


def observe_pool():
    case, h2, w2, ldp = POOL_CASE
    n, h, w, c, k = case[:5]
    p = Problem(case, seed=42)
    rng = np.random.default_rng(43)
    arg = torch.from_numpy(rng.integers(0, 4, (n, h, w, c)).astype(np.uint8)).cuda()
    y = padded(rng.standard_normal((n, h, w, c)).astype(np.float32), ldp or c)
    y[..., :c][y[..., :c].abs() < 0.4] = 0.0
    return {f'chain_pool:prepared={int(prepared)}': sha(*p.chain(prepared, False, pool=(arg, y), dx_shape=(n, h2, w2, c)))
            for prepared in (False, True)}


def observe_1d(case):
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    n, h, w, c, k, r = case[:6]
    x, dz, wt, relu = W1.operands(case, 51)
    d = desc_of(case)
    xd, dzd, md = padded(x, d.ldx), padded(dz, d.ldy), padded(relu, d.ldx)
    wd = torch.from_numpy(wt).cuda()
    pf = ops.PreparedFilter(d, xd.device, 'bwd_d_wino1d')
    assert pf.ok
    pf.refresh(wd)
    q = lambda fn, dd: int(fn(ctypes.byref(dd)))      # noqa: E731
    out = {'ws': {
        'bwd_data': [q(lib.a3dl_conv2d_bwd_data_ws_bytes, d), q(lib.a3dl_conv2d_bwd_data_ws_bytes, pf.desc_prepared)],
        'bwd_filter': q(lib.a3dl_conv2d_bwd_filter_ws_bytes, d),
        'prepared': q(lib.a3dl_conv2d_bwd_data_prepared_filter_bytes, d),
    }}
    for tag, (dd, f) in (('per_call', (d, wd)), ('prepared', (pf.desc_prepared, pf.buf))):
        dx = full(n, h, w, d.ldx)
        ops.conv2d_bwd_data_wino1d(dd, dzd, f, dx, relu_mask=md)
        out['bwd_data:mask:' + tag] = sha(dx)
    dw, db = full(r, 5, c, k), full(k)
    ops.conv2d_bwd_filter_wino1d(d, xd, dzd, dw, db)
    out['bwd_filter'] = sha(dw, db)
    return out


def observe(name):
    """What the routes leave on case `name`, in a form JSON holds exactly."""
    if name == '2d:pool':
        return observe_pool()
    return observe_2d(CASES_2D[name]) if name in CASES_2D else observe_1d(CASES_1D[name])


def test_the_golden_file_holds_every_case_and_nothing_else():
    assert sorted(json.load(open(GOLDEN))) == sorted(NAMES) and len(NAMES) == len(W.CASES) + len(W1.CASES) + 1


@pytest.mark.parametrize('name', NAMES)
def test_routes_leave_the_recorded_bits(name):
    want = json.load(open(GOLDEN))[name]
    got = json.loads(json.dumps(observe(name)))
    assert sorted(got) == sorted(want)
    assert got == want, [key for key in want if got[key] != want[key]]
