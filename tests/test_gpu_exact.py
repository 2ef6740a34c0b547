"""Every contraction route, element by element.  The operands are small integers for which every float32 / bf16 MFMA, every
bf16x3 split, every split-K slab, stream-K share and reduction order is exact (tests/exact_ops.py asserts the conditions, and
test_exact_cpu.py checks them without a GPU), so each output must EQUAL the float64 oracle: np.testing.assert_array_equal on
the whole allocation — pad columns and guard rows included, pre-filled with NaN (argmax bytes: 9) — with no tolerance and no
element left out.  A localized error (the last row of an M tail, one column tile, one product of a k-tile that straddles two
taps, a pad float of a window run, a stream-K share added twice) changes an element by at least 1 and names it.

Where a case is here for a route, the launch is bracketed (a3d_timing_enable / a3d_timing_collect) and the record's kernel
family (prec, lds_dma) asserted — never the tile — so a planner change that moves the case onto another kernel fails the test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_ops as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
BF = torch.bfloat16
# kernel families as (a3d_timing_record.prec, .lds_dma)
IGEMM_F32 = {(0, 0), (0, 1)}         # igemm.h register-staged / igemm_glds.h
CONV3, CONV3B = {(0, 2)}, {(2, 2)}   # conv3.hip: float32 and the bf16 image form
FEWCH, FEWCH16 = {(0, 4)}, {(2, 4)}  # fewch.hip / fewch16.hip
IGEMM_BF16X3, IGEMM_BF16 = {(1, 0)}, {(2, 0)}
RING = {(2, 3)}                      # igemm_ring.h


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda().to(dtype)


def guarded(rows, ld, dtype=torch.float32, fill=NAN):
    """an allocation of `rows` rows of pitch `ld` followed by guard rows, all of it `fill`"""
    return torch.full((rows + 67, ld), fill, device='cuda', dtype=dtype)


def expect(big, rows, cols, ref, fill=np.nan, what=''):
    """the WHOLE allocation: `ref` in its first rows x cols, the fill everywhere else"""
    want = np.full(tuple(big.shape), fill, np.float64)
    want[:rows, :cols] = np.asarray(ref, np.float64).reshape(rows, cols)
    got = big.cpu().numpy() if big.dtype == torch.uint8 else big.float().cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=what)


def launched(fn):
    """runs fn with every launch bracketed -> its timing records"""
    from ann3depth_amd import _lib
    lib = _lib.load()
    lib.a3d_timing_select(None)
    lib.a3d_timing_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.a3d_timing_enable(0)
    arr = (_lib.TimingRecord * 64)()
    return [arr[i] for i in range(lib.a3d_timing_collect(arr, 64))]


def on_family(recs, family, what):
    assert recs and {(r.prec, r.lds_dma) for r in recs} <= family, (what, [(r.mode, r.prec, r.lds_dma) for r in recs])
    return recs


def conv_fwd_exact(ops, cs, d, x, wt, b, family, tdt=torch.float32, what=''):
    """conv + bias, conv + bias + ReLU, conv alone -> a pitched, guarded y"""
    n, h, w, c, k, ks, st, pad = cs.shape
    rows = n * cs.ho * cs.wo
    for bias, act, ref in ((b, None, cs.y), (b, 'relu', np.maximum(cs.y, 0)), (None, None, cs.y - E.f64(cs.b))):
        if tdt == BF:
            ref = cs.stored('y', ref)                          # <= 256, or the RNE of a rounded-store case
        big = guarded(rows, d.ldy, tdt)
        recs = launched(lambda: ops.conv2d_fwd(d, x, wt, bias, big[:rows].view(n, cs.ho, cs.wo, d.ldy), act))
        expect(big, rows, k, ref, what=f'{what} forward {cs.shape} act {act}')
        if family:
            on_family(recs, family, f'{what} forward {cs.shape}')


def conv_bwd_filter_exact(ops, cs, d, x, dz, family, what=''):
    n, h, w, c, k, ks, st, pad = cs.shape
    dw, db = guarded(ks * ks * c, k), guarded(1, k)
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x, dz, dw[:ks * ks * c].view(ks, ks, c, k), db[0]))
    expect(dw, ks * ks * c, k, cs.dw, what=f'{what} dw {cs.shape}')
    expect(db, 1, k, cs.db, what=f'{what} db {cs.shape}')
    if family:
        on_family(recs, family, f'{what} bwd-filter {cs.shape}')
    dw.fill_(NAN)                                            # without the fused BiasAddGrad
    ops.conv2d_bwd_filter(d, x, dz, dw[:ks * ks * c].view(ks, ks, c, k), None)
    expect(dw, ks * ks * c, k, cs.dw, what=f'{what} dw alone {cs.shape}')


def conv_bwd_data_exact(ops, cs, d, dz, wt, xmask, family, tdt=torch.float32, what='', one_launch=False):
    """plain, and with the ReluGrad of the layer below (x has zeros and negatives: a third each) -> a guarded dx"""
    n, h, w, c, k, ks, st, pad = cs.shape
    rows = n * h * w
    for mask in (None, xmask):
        ref = cs.dx if mask is None else cs.dx * (cs.x > 0)
        if tdt == BF:
            ref = cs.stored('dx', ref)
        big = guarded(rows, c, tdt)
        recs = launched(lambda: ops.conv2d_bwd_data(d, dz, wt, big[:rows].view(n, h, w, c), relu_mask=mask))
        expect(big, rows, c, ref, what=f'{what} dx {cs.shape} mask {mask is not None}')
        if family:
            on_family(recs, family, f'{what} bwd-data {cs.shape}')
        if one_launch:     # the parity classes of a strided bwd-data as ONE launch: its flops are the classes' sum, not 2 m n k
            assert len(recs) == 1 and recs[0].mode == 1 and recs[0].flops != 2.0 * recs[0].m * recs[0].n * recs[0].k, what


def conv_exact_f32_tensors(ops, cs, precision='fp32', fwd=None, bwd_d=None, bwd_f=None, one_launch=False, hints=0):
    """all three directions on float32 tensors, in the arithmetic `precision`"""
    n, h, w, c, k, ks, st, pad = cs.shape
    d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, precision=precision, hints=hints)
    assert (d.ho, d.wo) == (cs.ho, cs.wo)
    x, wt, b, dz = dev(cs.x), dev(cs.w), dev(cs.b), dev(cs.dz)
    conv_fwd_exact(ops, cs, d, x, wt, b, fwd, what=precision)
    conv_bwd_filter_exact(ops, cs, d, x, dz, bwd_f, what=precision)
    conv_bwd_data_exact(ops, cs, d, dz, wt, x, bwd_d, what=precision, one_launch=one_launch)


def conv_exact_bf16_tensors(ops, cs, fwd=None, bwd_d=None, bwd_f=None, one_launch=False, directions=(0, 1, 2)):
    """... on bf16-stored x, filter copy, y, dz and dx (the filter gradient stays float32)"""
    n, h, w, c, k, ks, st, pad = cs.shape
    X, W, Y = ops.STORE_X, ops.STORE_W, ops.STORE_Y
    d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, precision='bf16')
    x, wt, b, dz = dev(cs.x, BF), dev(cs.w, BF), dev(cs.b), dev(cs.dz, BF)
    if 0 in directions:
        conv_fwd_exact(ops, cs, ops.with_storage(d, X | W | Y), x, wt, b, fwd, tdt=BF, what='bf16 tensors')
    if 2 in directions:
        conv_bwd_filter_exact(ops, cs, ops.with_storage(d, X | Y), x, dz, bwd_f, what='bf16 tensors')
    if 1 in directions:
        if not cs.rounds:
            cs.bf16('dx')
        conv_bwd_data_exact(ops, cs, ops.with_storage(d, X | W | Y), dz, wt, x, bwd_d, tdt=BF, what='bf16 tensors', one_launch=one_launch)


# ---- generic fp32 implicit GEMM ----
@pytest.mark.parametrize('case', E.GENERIC + [E.WIDE])
def test_generic_fp32_implicit_gemm(ops, case):
    conv_exact_f32_tensors(ops, E.conv_case(*case), fwd=IGEMM_F32, bwd_d=IGEMM_F32, bwd_f=IGEMM_F32)


@pytest.mark.parametrize('n,h,w,c,k,ks,ld', E.GUARD)
def test_tile_epilogues_with_a_pitch_wider_than_n(ops, n, h, w, c, k, ks, ld):
    """rows of the last tile past M, columns past N, output pitch wider than N: forward (plain, bias + ReLU, fused pool with
    its argmax bytes) and bwd-data with the ReluGrad mask into a window of a wider buffer"""
    cs = E.conv_case(n, h, w, c, k, ks, 1, 'SAME')
    d = ops.conv_desc(n, h, w, c, k, ks, ks, 1, 'SAME', ldy=ld)
    x, wt, b, dz = dev(cs.x), dev(cs.w), dev(cs.b), dev(cs.dz)
    conv_fwd_exact(ops, cs, d, x, wt, b, IGEMM_F32, what='pitched')
    pool_fwd_exact(ops, cs, d, x, wt, b, ld, IGEMM_F32)
    conv_bwd_filter_exact(ops, cs, ops.conv_desc(n, h, w, c, k, ks, ks, 1, 'SAME'), x, dz, IGEMM_F32)
    ld2, rows = c + 8, n * h * w
    dd = ops.conv_desc(n, h, w, c, k, ks, ks, 1, 'SAME', ldx=ld2)
    xb = torch.zeros((rows + 67, ld2), device='cuda')
    xb[:rows, :c] = x.view(rows, c)
    dxb = guarded(rows, ld2)
    on_family(launched(lambda: ops.conv2d_bwd_data(dd, dz, wt, dxb[:rows].view(n, h, w, ld2), relu_mask=xb[:rows].view(n, h, w, ld2))),
              IGEMM_F32, 'pitched bwd-data')
    expect(dxb, rows, c, cs.dx * (cs.x > 0), what=f'pitched dx {cs.shape}')


# ---- strided bwd-data as one launch ----
@pytest.mark.parametrize('case', E.STRIDED_ONE_LAUNCH)
def test_strided_bwd_data_as_one_launch(ops, case):
    conv_exact_f32_tensors(ops, E.conv_case(*case), fwd=IGEMM_F32, bwd_d=IGEMM_F32, bwd_f=IGEMM_F32, one_launch=True)


@pytest.mark.parametrize('case', E.STRIDED_ONE_LAUNCH_BF16)
def test_strided_bwd_data_on_bf16_tensors_as_one_launch(ops, case):
    """igemm_bf16_multi_kernel: unequal classes, SAME padding; a 1 x 1 filter whose odd classes receive no tap: exact zeros"""
    cs = E.conv_case(*case)
    conv_exact_bf16_tensors(ops, cs, bwd_d=IGEMM_BF16, one_launch=True, directions=(1,))
    if case[5] == 1:
        assert (cs.dx[:, 1::2] == 0).all() and (cs.dx[:, :, 1::2] == 0).all() and (cs.dx != 0).any()


# ---- few-channel forward (conv3.hip) and window runs ----
@pytest.mark.parametrize('case', E.FEW_CHANNEL)
def test_few_channel_forward_and_window_runs(ops, case):
    """... with and without A3D_HINT_SHARE_CU and with a prepared filter where the forward repacks one; >= 33 filters without
    padding: conv3.hip, fewer: the generic kernel (window runs where the row geometry allows them)"""
    cs = E.conv_case(*case)
    n, h, w, c, k, ks, st, pad = case
    fwd = CONV3 if (k >= 33 and pad == 'VALID') else IGEMM_F32
    conv_exact_f32_tensors(ops, cs, fwd=fwd)
    x, wt, b = dev(cs.x), dev(cs.w), dev(cs.b)
    hinted = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, hints=ops.HINT_SHARE_CU)
    conv_fwd_exact(ops, cs, hinted, x, wt, b, fwd, what='share-cu')
    for d in (ops.conv_desc(n, h, w, c, k, ks, ks, st, pad), hinted):
        pf = ops.PreparedFilter(d, x.device)
        assert pf.ok == (pad == 'VALID'), 'which forwards repack their filter'
        if pf.ok:
            pf.refresh(wt)
            conv_fwd_exact(ops, cs, pf.desc_prepared, x, pf.buf, b, fwd, what='prepared filter')


# ---- few-channel filter gradients (fewch.hip, fewch16.hip), plain and pool-fused ----
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', E.POOLED_BWDF)
def test_few_channel_filter_gradients(ops, case, dtype):
    """MaxPoolGrad by index + ReluGrad + Conv2DBackpropFilter + BiasAddGrad in one launch.  A third of the pooled maxima are
    exactly 0: their gradient must be 0 (ReluGrad is `> 0`), and any leak changes dw by an integer."""
    cs = E.pooled_bwdf_case(*case)
    n, h, w, c, k, ks, st, ld, lda = case
    tdt = BF if dtype == 'bf16' else torch.float32
    x, arg = dev(cs.x), torch.from_numpy(cs.arg).cuda()
    dpool, pooled = dev(cs.dpool, tdt), dev(cs.pooled, tdt)
    runs = [('fp32', FEWCH)] + ([('bf16', FEWCH16)] if dtype == 'bf16' else [])
    for precision, family in runs:
        d = ops.conv_desc(n, h, w, c, k, ks, ks, st, 'VALID', precision=precision)
        assert ops.conv2d_bwd_filter_pooled_supported(d)
        dw, db = guarded(ks * ks * c, k), guarded(1, k)
        on_family(launched(lambda: ops.conv2d_bwd_filter_pooled(d, x, dpool, pooled, arg, dw[:ks * ks * c].view(ks, ks, c, k), db[0])),
                  family, f'pool-fused filter gradient {precision}')
        expect(dw, ks * ks * c, k, cs.dw, what=f'pool-fused dw {precision} {case}')
        expect(db, 1, k, cs.db, what=f'pool-fused db {precision} {case}')
    if dtype == 'f32':        # the plain form on the materialised gradient
        d = ops.conv_desc(n, h, w, c, k, ks, ks, st, 'VALID')
        dw, db = guarded(ks * ks * c, k), guarded(1, k)
        on_family(launched(lambda: ops.conv2d_bwd_filter(d, x, dev(cs.dz), dw[:ks * ks * c].view(ks, ks, c, k), db[0])), FEWCH, 'plain')
        expect(dw, ks * ks * c, k, cs.dw, what=f'plain dw {case}')
        expect(db, 1, k, cs.db, what=f'plain db {case}')


# ---- Cout = 1 stencils and conv2d_bwd_both ----
@pytest.mark.parametrize('dx16', [False, True])
@pytest.mark.parametrize('case', E.BOTH)
def test_one_filter_stencils(ops, case, dx16):
    """stencil1.hip: forward, filter gradient, and the whole backward in one pass — twice on one state buffer (the arrival
    counters must come back to zero); dx float32 or bf16, with and without ReluGrad, at its own pitch"""
    cs = E.both_case(*case)
    n, h, w, c, pad, ldx, lddx = case
    d = ops.conv_desc(n, h, w, c, 1, 5, 5, 1, pad, ldx=ldx)
    assert ops.conv2d_bwd_both_supported(d)
    ho, wo = cs.y.shape[1:3]
    xb, wt, b, dz = dev(cs.xbuf), dev(cs.w), dev(cs.b), dev(cs.dz)
    rows = n * ho * wo
    if not dx16:
        for act, ref in ((None, cs.y), ('relu', np.maximum(cs.y, 0))):
            y = guarded(rows, 1)
            ops.conv2d_fwd(d, xb, wt, b, y[:rows].view(n, ho, wo, 1), act)
            expect(y, rows, 1, ref, what=f'one-filter forward {case}')
        dw, db = guarded(25 * c, 1), guarded(1, 1)
        ops.conv2d_bwd_filter(d, xb, dz, dw[:25 * c].view(5, 5, c, 1), db[0])
        expect(dw, 25 * c, 1, cs.dw, what=f'one-filter dw {case}')
        expect(db, 1, 1, cs.db, what=f'one-filter db {case}')
    for mask in (True, False):
        for again in range(2):
            dw, db = guarded(25 * c, 1), guarded(1, 1)
            dx = guarded(n * h * w, lddx, BF if dx16 else torch.float32)
            ops.conv2d_bwd_both(d, xb, dz, wt, dw[:25 * c].view(5, 5, c, 1), db[0], dx[:n * h * w].view(n, h, w, lddx), relu_mask=mask)
            expect(dw, 25 * c, 1, cs.dw, what=f'bwd_both dw {case} run {again}')
            expect(db, 1, 1, cs.db, what=f'bwd_both db {case} run {again}')
            expect(dx, n * h * w, c, cs.dx * (cs.x > 0) if mask else cs.dx, what=f'bwd_both dx {case} mask {mask} run {again}')


# ---- conv + ReLU + 2x2 pool in one launch, and maxpool2x2_bwd_idx from its bytes ----
def pool_fwd_exact(ops, cs, d, x, wt, b, ld, family, tdt=torch.float32, acts=(('relu', True), (None, False)), ties=10):
    """pooled values and argmax bytes against the first maximum of the exact reference; then the by-index MaxPoolGrad
    (+ ReluGrad) from the bytes and values the launch wrote -> (pooled allocation, argmax allocation) of the last run"""
    n, h, w, c, k, ks, st, pad = cs.shape
    ph, pw = cs.ho // 2, cs.wo // 2
    prow = n * ph * pw
    for act, with_bias in acts:
        y = np.maximum(cs.y, 0) if act else cs.y - E.f64(cs.b)
        if tdt == BF and cs.rounds:      # the first maximum of the ROUNDED window: rounding creates ties (asserted in >= `ties` windows)
            pooled, arg = E.rounded_pool(cs, y, ties)
        else:
            pooled, arg = E.pool_reference(y)
        if tdt == BF:
            pooled = cs.stored('pooled', pooled)
        pbig, abig = guarded(prow, ld, tdt), guarded(prow, k, torch.uint8, 9)
        recs = launched(lambda: ops.conv2d_pool_fwd(d, x, wt, b if with_bias else None, pbig[:prow].view(n, ph, pw, ld), act,
                                                    abig[:prow].view(n, ph, pw, k)))
        expect(pbig, prow, k, pooled, what=f'pooled map {cs.shape} act {act}')
        expect(abig, prow, k, arg, fill=9, what=f'argmax bytes {cs.shape} act {act}')
        on_family(recs, family, f'fused pool {cs.shape}')
        p2 = guarded(prow, ld, tdt)                          # without the argmax bytes: the same map
        ops.conv2d_pool_fwd(d, x, wt, b if with_bias else None, p2[:prow].view(n, ph, pw, ld), act, None)
        expect(p2, prow, k, pooled, what=f'pooled map without argmax {cs.shape} act {act}')
        if not act:
            continue
        dy = E.ternary(np.random.default_rng(prow + k), (n, ph, pw, ld))
        # bf16 pooled map: a bf16 gradient; dx bf16 where the kernel's 16-byte pieces allow it, float32 otherwise
        dxt = BF if (tdt == BF and k % 8 == 0 and ld % 8 == 0) else torch.float32
        for relu in (True, False):
            dx = guarded(n * cs.ho * cs.wo, k, dxt)
            ops.maxpool2x2_bwd_idx(abig[:prow].view(n, ph, pw, k), pbig[:prow].view(n, ph, pw, ld), dev(dy, tdt),
                                   dx[:n * cs.ho * cs.wo].view(n, cs.ho, cs.wo, k), relu_mask=relu)
            want = E.pool_grad_reference(arg, pooled, E.f64(dy[..., :k]), (n, cs.ho, cs.wo, k), relu)
            expect(dx, n * cs.ho * cs.wo, k, want, what=f'MaxPoolGrad by index {cs.shape} relu {relu}')


@pytest.mark.parametrize('case', E.POOL_FWD)
def test_fused_pool_fp32(ops, case):
    cs = E.conv_case(*case)
    n, h, w, c, k, ks, st, pad = case
    d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad)
    x, wt, b = dev(cs.x), dev(cs.w), dev(cs.b)
    family = CONV3 if (c <= 4 and k >= 33 and pad == 'VALID') else IGEMM_F32
    for ld in (k, k + 1):                  # dense, and a concat buffer with one more channel
        pool_fwd_exact(ops, cs, d, x, wt, b, ld, family)


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_IMAGE)
def test_fused_pool_bf16_image_form(ops, case):
    """a 3-channel image as bf16 pixels of 4 channels (a3d_pad_channels_bf16), bf16 output at a pitch of whole 16-byte pieces;
    the filter's 4th channel holds anything (its pixels are zero); per-call repack and prepared filter"""
    bf16_image_form_exact(ops, E.conv_case(*case).bf16('y'))


def bf16_image_form_exact(ops, cs, ties=10):
    n, h, w, c, k, ks, st, pad = cs.shape
    x4 = torch.full((n, h, w, 4), NAN, device='cuda', dtype=BF)
    ops.pad_channels_bf16(dev(cs.x), x4)
    np.testing.assert_array_equal(x4.float().cpu().numpy(), np.concatenate([cs.x, np.zeros((n, h, w, 1), np.float32)], -1))
    w4 = dev(np.concatenate([cs.w, np.full((ks, ks, 1, k), 5.0, np.float32)], axis=2))
    b = dev(cs.b)
    ldy = (k + 7) // 8 * 8
    d = ops.with_storage(ops.conv_desc(n, h, w, 4, k, ks, ks, st, 'VALID', ldy=ldy, precision='bf16'), ops.STORE_X | ops.STORE_Y)
    family = CONV3B if k >= 33 else IGEMM_BF16
    pf = ops.PreparedFilter(d, x4.device)
    assert pf.ok
    pf.refresh(w4)
    for dd, filt in ((d, w4), (pf.desc_prepared, pf.buf)):
        conv_fwd_exact(ops, cs, dd, x4, filt, b, family, tdt=BF, what='bf16 image')
        pool_fwd_exact(ops, cs, dd, x4, filt, b, ldy, family, tdt=BF, acts=(('relu', True),), ties=ties)


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_STORED)
def test_fused_pool_on_bf16_stored_operands(ops, case):
    """bf16 x, w and pooled map: the pooling epilogue of the LDS-DMA kernel, and a3d_maxpool2x2_bwd_idx_bf16s from its bytes"""
    bf16_stored_pool_exact(ops, E.conv_case(*case).bf16('y'))


def bf16_stored_pool_exact(ops, cs):
    n, h, w, c, k, ks, st, pad = cs.shape
    d = ops.with_storage(ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, precision='bf16'), ops.STORE_X | ops.STORE_W | ops.STORE_Y)
    pool_fwd_exact(ops, cs, d, dev(cs.x, BF), dev(cs.w, BF), dev(cs.b), k, RING, tdt=BF, acts=(('relu', True),))


# ---- bf16 arithmetic ----
@pytest.mark.parametrize('precision,family', [('bf16x3', IGEMM_BF16X3), ('bf16', IGEMM_BF16)])
@pytest.mark.parametrize('case', E.BF16_ARITH)
def test_bf16_arithmetic_on_float32_tensors(ops, case, precision, family):
    """integers up to 256 are their own bf16 hi plane (the lo plane of the x3 split is zero): both modes are exact"""
    conv_exact_f32_tensors(ops, E.conv_case(*case), precision=precision, fwd=family, bwd_d=family, bwd_f=family)


@pytest.mark.parametrize('case', [c for c in E.BF16_ARITH if E.stores_bf16(c)])
def test_bf16_arithmetic_on_bf16_tensors(ops, case):
    conv_exact_bf16_tensors(ops, E.conv_case(*case).bf16('y', 'dx'), fwd=IGEMM_BF16, bwd_d=IGEMM_BF16, bwd_f=IGEMM_BF16)


@pytest.mark.parametrize('case', E.RING)
def test_lds_dma_kernel_by_the_planner_s_own_pick(ops, case):
    """enough tiles for igemm_ring.h in all three directions (bwd-data of 96 input channels: the 96-column tile)"""
    conv_exact_bf16_tensors(ops, E.conv_case(*case).bf16('y', 'dx'), fwd=RING, bwd_d=RING, bwd_f=RING)


# ---- dense ----
@pytest.mark.parametrize('m,k,n', E.DENSE)
def test_dense_fp32(ops, m, k, n):
    """relu and no activation, dropout (x 2 is exact), bwd-data plain and with mask and scale = 2.0, the filter gradient; the
    small batches with k n >= 2^16 (2^20 for the forward) run dense.hip's weight-streaming kernels"""
    cs = E.dense_case(m, k, n)
    x, w, b, dz = dev(cs.x), dev(cs.w), dev(cs.b), dev(cs.dz)
    keep = dev(cs.keep, torch.uint8)
    for act, drop, ref in ((None, None, cs.y), ('relu', None, np.maximum(cs.y, 0)), ('relu', keep, 2.0 * np.maximum(cs.y, 0) * cs.keep),
                           (None, keep, 2.0 * cs.y * cs.keep)):
        y = guarded(m, n)
        ops.dense_fwd(x, w, b, y[:m], act, drop_keep=drop)
        expect(y, m, n, ref, what=f'dense forward {cs.shape} act {act} dropout {drop is not None}')
    y = guarded(m, n)
    ops.dense_fwd(x, w, None, y[:m], None)
    expect(y, m, n, cs.y - E.f64(cs.b), what=f'dense forward without bias {cs.shape}')
    for mask, scale, ref in ((None, 1.0, cs.dx), (x, 2.0, 2.0 * cs.dx * (cs.x > 0)), (x, 1.0, cs.dx * (cs.x > 0))):
        dx = guarded(m, k)
        ops.dense_bwd_data(dz, w, dx[:m], mask=mask, scale=scale)
        expect(dx, m, k, ref, what=f'dense dx {cs.shape} scale {scale}')
    dw, db = guarded(k, n), guarded(1, n)
    ops.dense_bwd_filter(x, dz, dw[:k], db[0])
    expect(dw, k, n, cs.dw, what=f'dense dw {cs.shape}')
    expect(db, 1, n, cs.db, what=f'dense db {cs.shape}')


@pytest.mark.parametrize('m,k,n', E.DENSE_BF16)
def test_dense_on_bf16_tensors(ops, m, k, n):
    """a3d_dense_fwd_ex / a3d_dense_bwd_data_ex on bf16 x / dz / dx beside bf16 weights (64-row tiles of the LDS-DMA kernel, K
    split over several blocks, activation / dropout / mask applied by the reduction), with a bf16 second output"""
    cs = E.dense_case(m, k, n).bf16()
    x, w, b, dz = dev(cs.x, BF), dev(cs.w, BF), dev(cs.b), dev(cs.dz, BF)
    keep = dev(cs.keep, torch.uint8)
    st = ops.STORE_W | ops.STORE_X
    for act, drop, ref in ((None, None, cs.y), ('relu', keep, 2.0 * np.maximum(cs.y, 0) * cs.keep)):
        y, y16 = guarded(m, n), guarded(m, n, BF)
        recs = launched(lambda: ops.dense_fwd_ex(x, w, b, y[:m], act, drop_keep=drop, precision='bf16', storage=st,
                                                 out2=ops.second_output(y16[:m])))
        expect(y, m, n, ref, what=f'bf16 dense forward {cs.shape} act {act}')
        expect(y16, m, n, ref, what=f'bf16 dense forward, second output {cs.shape} act {act}')
        on_family(recs, RING, 'bf16 dense forward')
    st = ops.STORE_W | ops.STORE_X | ops.STORE_Y
    for mask, scale, ref in ((None, 1.0, cs.dx), (x, 2.0, 2.0 * cs.dx * (cs.x > 0))):
        dx, dx32 = guarded(m, k, BF), guarded(m, k)
        recs = launched(lambda: ops.dense_bwd_data_ex(dz, w, dx[:m], mask=mask, scale=scale, precision='bf16', storage=st,
                                                      out2=ops.second_output(dx32[:m])))
        expect(dx, m, k, ref, what=f'bf16 dense dx {cs.shape} scale {scale}')
        expect(dx32, m, k, ref, what=f'bf16 dense dx, second output {cs.shape} scale {scale}')
        on_family(recs, RING, 'bf16 dense bwd-data')


# ---- pinned tiles, split-K and stream-K: one child process ----
def test_pinned_tiles_split_k_and_stream_k_in_a_tuning_process():
    """tests/exact_forced_worker.py (A3D_TUNING=1: the A3D_FORCE_* switches are read per launch; A3D_PLAN_LOG=1: it checks in
    every launch's plan line that the pinned configuration, split factor and stream-K grid were applied) — every float32 tile
    configuration x direction x split-K factor / stream-K grid, the bf16 kernel's column widths x split-K factors, every tile of
    the LDS-DMA kernel, all element by element."""
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    env.update(A3D_TUNING='1', A3D_PLAN_LOG='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'exact_forced_worker.py')], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'MISMATCH' not in r.stdout, r.stdout[-3000:]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith('verified ')]
    assert len(done) == 1 and int(done[0].split()[1]) == E.forced_count(), r.stdout[-2000:]
