"""Both Winograd gradients of a layer as one chain (include/a3d_wino_bwd.h, csrc/wino.hip) on the GPU: dw, db and dx are THE BITS
of a3dwg_conv2d_bwd_filter followed by a3d_conv2d_bwd_data under 'fp32w' — torch.equal, with and without a prepared filter, with
and without a ReLU mask; the pool form against the route's dx followed by a3d_maxpool2x2_bwd_idx(relu_mask=1); run-to-run bits;
the descriptors the routes hand on; a short workspace; the timing records; and the coarse step of MSDNReplica with the chain
against the same step on the three separate calls, every array of the step's outputs."""
import ctypes

import numpy as np
import pytest
import torch

import wino_ref as W

pytestmark = pytest.mark.gpu

GUARD = 7.0
# W.CASES and the 13x18 layer at n = 13: 819 tiles, the filter gradient's tile axis in five uneven splits
CASES = list(W.CASES) + [(13, 13, 18, 256, 384, 'SAME', None, None)]
# (case, unpooled extents): an odd last row and column, even extents, conv2d_2 of the network at n = 3; the last entry's pooled
# map has a pixel stride off the 16-byte grid (the scalar form of the scatter)
POOLED = [((2, 5, 6, 8, 8, 'SAME', None, None), 11, 13, None), ((2, 5, 6, 8, 8, 'SAME', None, None), 10, 12, None),
          ((3, 13, 18, 384, 256, 'SAME', None, None), 27, 37, None), ((2, 5, 6, 8, 8, 'SAME', None, None), 11, 13, 9)]


def padded(a, ld):
    """a [..., c] on the device as the first c channels of pixels `ld` apart; the other channels hold GUARD"""
    t = torch.full(a.shape[:-1] + (ld,), GUARD, device='cuda')
    t[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def guarded(shape, lead=64):
    """a GUARD-filled allocation and the view of `shape` that starts `lead` floats into it"""
    n = int(np.prod(shape))
    big = torch.full((lead + n + 64,), GUARD, device='cuda')
    return big, big[lead:lead + n].view(shape)


class Problem:
    """The operands of one case on the device, and the descriptors of the calls on them"""

    def __init__(self, case, seed=41):
        from ann3depth_amd import ops
        n, h, w, c, k, padding, ldx, ldy = case
        self.shape = (n, h, w, c, k)
        self.ldx, self.ldy = ldx or c, ldy or k
        ho, wo, _, _ = W.geometry(h, w, padding)
        rng = np.random.default_rng(seed)
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
        self.x, self.dz, self.mask = padded(draw(n, h, w, c), self.ldx), padded(draw(n, ho, wo, k), self.ldy), padded(draw(n, h, w, c), self.ldx)
        self.g = torch.from_numpy((draw(3, 3, c, k) / np.sqrt(9 * c)).astype(np.float32)).cuda()
        self.d = ops.conv_desc(n, h, w, c, k, 3, 3, 1, padding, ldx=self.ldx, ldy=self.ldy)
        self.dw_ = ops.conv_desc(n, h, w, c, k, 3, 3, 1, padding, ldx=self.ldx, ldy=self.ldy, precision='fp32w')
        self.pb = ops.PreparedFilter(self.dw_, self.x.device, 'bwd_d')
        assert self.pb.ok
        self.pb.refresh(self.g)

    def filter(self, prepared):
        return (self.pb.desc_prepared, self.pb.buf) if prepared else (self.dw_, self.g)

    def outputs(self, dx_shape=None):
        n, h, w, c, k = self.shape
        self.bigs = [guarded((3, 3, c, k)), guarded((k,)), guarded(dx_shape or (n, h, w, self.ldx))]
        return [v for _, v in self.bigs]

    def untouched(self):
        """nothing around dw, db, dx was written, nor the guard columns of x, dz and dx"""
        n, h, w, c, k = self.shape
        for big, v in self.bigs:
            b = big.cpu().numpy()
            assert (b[:64] == GUARD).all() and (b[64 + v.numel():] == GUARD).all()
        assert (self.x[..., c:] == GUARD).all() and (self.dz[..., k:] == GUARD).all() and (self.mask[..., c:] == GUARD).all()

    def separate(self, prepared, mask, dx_shape=None):
        from ann3depth_amd import ops
        dw, db, dx = self.outputs(dx_shape)
        d, f = self.filter(prepared)
        ops.conv2d_bwd_filter_wino(self.d, self.x, self.dz, dw, db)
        ops.conv2d_bwd_data(d, self.dz, f, dx, relu_mask=self.mask if mask else None)
        self.untouched()
        return dw.clone(), db.clone(), dx.clone()

    def chain(self, prepared, mask, pool=None, dx_shape=None):
        from ann3depth_amd import ops
        dw, db, dx = self.outputs(dx_shape)
        d, f = self.filter(prepared)
        ops.conv2d_bwd_wino(d, self.x, self.dz, f, dw, db, dx, relu_mask=self.mask if mask else None, pool=pool)
        self.untouched()
        return dw.clone(), db.clone(), dx.clone()


def same_bits(got, want, what):
    for name, a, b in zip(('dw', 'db', 'dx'), got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: {name}'


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:6])) + ('' if c[6] is None else 'guard'))
def test_the_bits_of_the_two_calls(case):
    p = Problem(case)
    for prepared in (False, True):
        for mask in (False, True):
            want = p.separate(prepared, mask)
            got = p.chain(prepared, mask)
            same_bits(got, want, f'prepared {prepared} mask {mask}')
            if case[6] is not None:                      # dx's guard columns are part of the comparison and hold GUARD
                assert (got[2][..., case[3]:] == GUARD).all()


@pytest.mark.parametrize('case,h2,w2,ldp', POOLED, ids=lambda v: 'x'.join(map(str, v[:5])) if isinstance(v, tuple) else str(v))
def test_the_pool_form_is_the_route_followed_by_the_pool_gradient(case, h2, w2, ldp):
    from ann3depth_amd import ops
    n, h, w, c, k = case[:5]
    assert (h2 // 2, w2 // 2) == (h, w)
    p = Problem(case, seed=42)
    rng = np.random.default_rng(43)
    arg = torch.from_numpy(rng.integers(0, 4, (n, h, w, c)).astype(np.uint8)).cuda()
    y = padded(rng.standard_normal((n, h, w, c)).astype(np.float32), ldp or c)      # a third of the maxima not above zero
    y[..., :c][y[..., :c].abs() < 0.4] = 0.0
    for prepared in (False, True):
        dw0, db0, dx0 = p.separate(prepared, False)
        big, want = guarded((n, h2, w2, c))
        ops.maxpool2x2_bwd_idx(arg, y, dx0, want, relu_mask=True)
        dw1, db1, got = p.chain(prepared, False, pool=(arg, y), dx_shape=(n, h2, w2, c))
        same_bits((dw1, db1, got), (dw0, db0, want), f'prepared {prepared}')
        assert (got != GUARD).all()                      # every element written, the zero last row / column included
        if h2 % 2:
            assert (got[:, -1] == 0).all()
        if w2 % 2:
            assert (got[:, :, -1] == 0).all()
        assert (got != 0).any()


def test_two_runs_give_the_same_bits():
    p = Problem(CASES[-1])                               # five splits
    same_bits(p.chain(True, True), p.chain(True, True), 'run to run')


@pytest.mark.parametrize('shape,kw', [((2, 11, 9, 16, 24, 5, 5, 1, 'SAME'), {}), ((2, 13, 18, 32, 48, 3, 3, 2, 'VALID'), {}),
                                      ((2, 13, 18, 32, 48, 3, 3, 1, 'SAME'), {'precision': 'bf16', 'storage': 7})],
                         ids=['5x5', 'stride 2', 'bf16 storage'])
def test_descriptors_the_routes_do_not_take_run_the_two_direct_calls(shape, kw):
    from ann3depth_amd import ops
    n, h, w, c, k = shape[:5]
    assert not kw or kw['storage'] == ops.STORE_X | ops.STORE_W | ops.STORE_Y
    tdt = torch.bfloat16 if kw else torch.float32
    rng = np.random.default_rng(44)
    d = ops.conv_desc(*shape, **kw)
    draw = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()      # noqa: E731
    x, dz, mask = draw(n, h, w, c).to(tdt), draw(n, d.ho, d.wo, k).to(tdt), draw(n, h, w, c).to(tdt)
    g = (draw(*shape[5:7], c, k) / np.sqrt(c * shape[5] * shape[6])).to(tdt)
    got = []
    for chain in (False, True):
        dw, db = torch.full(shape[5:7] + (c, k), GUARD, device='cuda'), torch.full((k,), GUARD, device='cuda')
        dx = torch.full((n, h, w, c), GUARD, device='cuda', dtype=tdt)
        if chain:
            ops.conv2d_bwd_wino(d, x, dz, g, dw, db, dx, relu_mask=mask)
        else:
            ops.conv2d_bwd_filter(d, x, dz, dw, db)
            ops.conv2d_bwd_data(d, dz, g, dx, relu_mask=mask)
        got.append((dw, db, dx.float()))
    same_bits(got[1], got[0], 'forwarded')
    assert (got[1][2] != GUARD).any()


def test_a_workspace_one_byte_short_is_refused_and_the_outputs_untouched():
    from ann3depth_amd import _lib
    lib = _lib.load()
    p = Problem(CASES[3])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for prepared in (False, True):
        d, f = p.filter(prepared)
        dw, db, dx = p.outputs()
        need = lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(d), int(prepared), 0)
        assert need == lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(d), int(prepared), 1) > 0
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        args = (ctypes.byref(d), ptr(p.x), ptr(p.dz), ptr(f), ptr(dw), ptr(db), ptr(dx), None, None, ptr(ws))
        rc = lib.a3dwb_conv2d_bwd(*args, need - 1, None)
        torch.cuda.synchronize()
        assert rc == -2 and 'workspace' in _lib.last_error()
        assert bool((dw == GUARD).all()) and bool((db == GUARD).all()) and bool((dx == GUARD).all())
        rc = lib.a3dwb_conv2d_bwd(*args, need, None)
        torch.cuda.synchronize()
        assert rc == 0                                   # the queried size itself is enough
        same_bits((dw, db, dx), p.separate(prepared, False), f'prepared {prepared}')


def records_of(call):
    from ann3depth_amd import _lib
    lib = _lib.load()
    lib.a3d_timing_select(None)
    lib.a3d_timing_enable(1)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        lib.a3d_timing_enable(0)
        arr = (_lib.TimingRecord * 8)()
        recs = [arr[i] for i in range(lib.a3d_timing_collect(arr, 8))]
    return [(r.mode, r.m, r.n, r.k, r.splitk) for r in recs]


def test_with_timing_the_products_are_the_two_launches_their_records_describe():
    from ann3depth_amd import _lib
    lib = _lib.load()
    for case in (CASES[3], CASES[-1]):                   # one split; five splits
        p = Problem(case)
        want_recs = records_of(lambda: setattr(p, 'want', p.separate(True, True)))
        got_recs = records_of(lambda: setattr(p, 'got', p.chain(True, True)))
        assert len(want_recs) == 2 and got_recs == want_recs
        assert [r[0] for r in got_recs] == [2, 1]        # MODE_BWD_F, then MODE_BWD_D
        same_bits(p.got, p.want, 'timed')
        same_bits(p.chain(True, True), p.want, 'untimed')      # ... and the paired launch gives the same bits
        arr = (_lib.TimingRecord * 8)()
        assert lib.a3d_timing_collect(arr, 8) == 0       # timing off: no record


def test_the_coarse_step_with_the_chain_is_the_step_with_the_three_calls():
    """B = 8 (504 tiles: both routes on): both losses, both maps and every variable and Adam slot of every optimizer are the bits
    of the step that runs a3dwg_conv2d_bwd_filter, a3d_conv2d_bwd_data and a3d_maxpool2x2_bwd_idx."""
    from ann3depth_amd import models
    from oracle import msdn as O
    B = 8
    rng = np.random.default_rng(45)
    img = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)).cuda()
    dep = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 1)) / 255).astype(np.float32)).cuda()
    keep = torch.from_numpy(rng.random((B, 4096)) >= 0.5).cuda()
    params = O.init_params(3000)

    class Separate(models.MSDNReplica):
        WINO_BWD_CHAIN = False

    nets = [models.MSDNReplica(B, device='cuda:0', params=params), Separate(B, device='cuda:0', params=params)]
    layers = set(models.MSDNReplica.WINO_LAYERS)
    assert all(set(net.d_wino) == layers and net.wino_grad == layers for net in nets)
    assert all(nets[0]._wino_chain(n) and not nets[1]._wino_chain(n) for n in layers)
    outs = []
    for net in nets:
        net.step(img, dep, keep)
        net.gather_state()
        out = {'coarse_loss': net.loss_coarse, 'fine_loss': net.loss_fine, 'coarse': net.coarse, 'fine': net.fine,
               'dc1': net.dc1, 'dc2': net.dc2}
        for name, g in net.groups.items():
            out.update({f'{name}_var': g.var, f'{name}_m': g.m, f'{name}_v': g.v, f'{name}_grad': g.grad})
        outs.append(out)
    torch.cuda.synchronize()
    assert set(outs[0]) == set(outs[1]) and 'CoarseConv_m' in outs[0]
    for key, a in outs[0].items():
        b = outs[1][key]
        assert (a is None) == (b is None), key
        if a is not None:
            assert a.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), key
