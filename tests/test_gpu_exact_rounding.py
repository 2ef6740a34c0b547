"""Every bf16 rounding site, bit for bit.  test_gpu_exact.py chooses operands for which nothing is ever rounded; here the
rounding is NOT the identity but is known exactly (tests/exact_ops.py):
  * rounded stores: integer sums far above 256 stored as bf16 must be bf16_rne(exact sum) — round to nearest, ties to even,
    once (a split-K launch after its slabs are added; a second output from the value the first one holds);
  * the fused pool must pick the first maximum of the ROUNDED window: in the cases here rounding creates ties;
  * rounded operands: a `bf16` kernel on float32 tensors must multiply bf16_rne(operand) — one operand at a time is wide
    (integers up to 4000), so each conversion is isolated in each direction that reads it;
  * the bf16x3 split: with a wide operand the lo plane is live, and hi hi + hi lo + lo hi must be the unrounded oracle (one
    operand wide) or the oracle minus lo lo (both wide).
Same comparison as test_gpu_exact.py, whose helpers these tests use: np.testing.assert_array_equal on the whole guarded
allocation, no tolerance, no mask, no element left out."""
import numpy as np
import pytest
import torch

import exact_ops as E
from test_gpu_exact import (BF, FEWCH, FEWCH16, IGEMM_BF16, IGEMM_BF16X3, IGEMM_F32, RING, bf16_image_form_exact,
                            bf16_stored_pool_exact, conv_exact_bf16_tensors, conv_exact_f32_tensors, conv_fwd_exact, dev, expect, guarded,
                            launched, on_family, ops, pool_fwd_exact)  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


def rne(a):
    return E.f64(E.bf16_rne(a))


# ---- rounded stores ----
@pytest.mark.parametrize('case', E.ROUNDED_GENERIC)
def test_rounded_stores_on_bf16_tensors(ops, case):
    """forward with bias, with ReLU and plain; bwd-data plain and masked; the filter gradient (float32: exact)"""
    conv_exact_bf16_tensors(ops, E.rounded_case(case, 'y', 'dx'), fwd=IGEMM_BF16, bwd_d=IGEMM_BF16, bwd_f=IGEMM_BF16)


@pytest.mark.parametrize('case', E.RING)
def test_rounded_stores_of_the_lds_dma_kernel(ops, case):
    conv_exact_bf16_tensors(ops, E.rounded_case(case, 'y', 'dx'), fwd=RING, bwd_d=RING, bwd_f=RING)


@pytest.mark.parametrize('case', E.ROUNDED_STRIDED)
def test_rounded_stores_of_the_strided_bwd_data_as_one_launch(ops, case):
    """... the 1 x 1 filter: rounded stores in the class that receives the tap, exact zeros in the three that receive none"""
    cs = E.rounded_case(case, 'dx')
    conv_exact_bf16_tensors(ops, cs, bwd_d=IGEMM_BF16, one_launch=True, directions=(1,))
    if case[5] == 1:
        assert (cs.dx[:, 1::2] == 0).all() and (cs.dx[:, :, 1::2] == 0).all() and (cs.dx != 0).any()


@pytest.mark.parametrize('second', [torch.float32, BF])
@pytest.mark.parametrize('case', E.ROUNDED_GENERIC)
def test_second_output_beside_a_rounded_first_output(ops, case, second):
    """a3d_conv2d_fwd_ex2: the second output is the value the bf16 first output holds — RNE(sum) in float32, and unchanged by
    the second conversion in bf16 (the split-K reduction and second_output_kernel both convert twice).  Here the split is the
    planner's; exact_forced_worker.py writes both types of second output under pinned split factors 1, 2 and 3."""
    cs = E.rounded_case(case, 'y')
    n, h, w, c, k, ks, st, pad = cs.shape
    d = ops.with_storage(ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, precision='bf16'), ops.STORE_X | ops.STORE_W | ops.STORE_Y)
    x, wt, b = dev(cs.x, BF), dev(cs.w, BF), dev(cs.b)
    rows = n * cs.ho * cs.wo
    for act, ref in (('relu', np.maximum(cs.y, 0)), (None, cs.y)):
        y, y2 = guarded(rows, k, BF), guarded(rows, k, second)
        on_family(launched(lambda: ops.conv2d_fwd(d, x, wt, b, y[:rows].view(n, cs.ho, cs.wo, k), act, out2=ops.second_output(y2[:rows]))),
                  IGEMM_BF16, f'second output {case}')
        expect(y, rows, k, rne(ref), what=f'first output {case} act {act}')
        expect(y2, rows, k, rne(ref), what=f'second output {second} {case} act {act}')


@pytest.mark.parametrize('precision,family', [('fp32', IGEMM_F32), ('bf16', IGEMM_BF16)])
@pytest.mark.parametrize('n,h,w,c,k,ks,ld', E.ROUNDED_GUARD)
def test_float32_inputs_with_a_rounded_bf16_output_and_pooled_map(ops, n, h, w, c, k, ks, ld, precision, family):
    """STORE_Y alone, at a pitch wider than k with guard rows: the tile epilogues' bf16 stores, and the fused pool on the values a
    separate conv would have stored — pooled map and argmax bytes of the first maximum of the ROUNDED window"""
    cs = E.rounded_case((n, h, w, c, k, ks, 1, 'SAME'), 'y')
    d = ops.with_storage(ops.conv_desc(n, h, w, c, k, ks, ks, 1, 'SAME', ldy=ld, precision=precision), ops.STORE_Y)
    x, wt, b = dev(cs.x), dev(cs.w), dev(cs.b)
    conv_fwd_exact(ops, cs, d, x, wt, b, family, tdt=BF, what=f'{precision}, bf16 y')
    pool_fwd_exact(ops, cs, d, x, wt, b, ld, family, tdt=BF, ties=0 if cs.shape in E.POOL_NO_TIES else 10)


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_IMAGE)
def test_fused_pool_bf16_image_form_on_rounded_values(ops, case):
    bf16_image_form_exact(ops, E.rounded_case(case, 'y'), ties=0 if case in E.POOL_NO_TIES else 10)


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_STORED)
def test_fused_pool_on_bf16_stored_operands_on_rounded_values(ops, case):
    bf16_stored_pool_exact(ops, E.rounded_case(case, 'y'))


def test_one_filter_stencil_with_a_rounded_bf16_dx(ops):
    """stencil1.hip's bf16 dx of 25-tap sums in the thousands, with and without ReluGrad"""
    case, mag = E.ROUNDED_BOTH
    cs = E.both_case(*case, mag=mag)
    n, h, w, c, pad, ldx, lddx = case
    d = ops.conv_desc(n, h, w, c, 1, 5, 5, 1, pad, ldx=ldx)
    assert ops.conv2d_bwd_both_supported(d)
    xb, wt, dz = dev(cs.xbuf), dev(cs.w), dev(cs.dz)
    for mask in (True, False):
        dw, db, dx = guarded(25 * c, 1), guarded(1, 1), guarded(n * h * w, lddx, BF)
        ops.conv2d_bwd_both(d, xb, dz, wt, dw[:25 * c].view(5, 5, c, 1), db[0], dx[:n * h * w].view(n, h, w, lddx), relu_mask=mask)
        expect(dw, 25 * c, 1, cs.dw, what=f'bwd_both dw {case}')
        expect(db, 1, 1, cs.db, what=f'bwd_both db {case}')
        expect(dx, n * h * w, c, cs.dx16 * (cs.x > 0) if mask else cs.dx16, what=f'bwd_both rounded dx {case} mask {mask}')


@pytest.mark.parametrize('m,k,n', E.DENSE_BF16)
def test_rounded_stores_of_the_dense_layers(ops, m, k, n):
    """bf16 second output of the forward (after ReLU and dropout x 2); bf16 dx with mask and scale 3 — tripling does not commute
    with the rounding, so a kernel that scales what it has rounded differs — beside a second output of either type"""
    cs = E.dense_case(m, k, n, (8, 8, 8), (2.0, 3.0)).rounded_store()
    x, w, b, dz = dev(cs.x, BF), dev(cs.w, BF), dev(cs.b), dev(cs.dz, BF)
    keep = dev(cs.keep, torch.uint8)
    st = ops.STORE_W | ops.STORE_X
    for act, drop, ref in ((None, None, cs.y), ('relu', keep, 2.0 * np.maximum(cs.y, 0) * cs.keep)):
        y, y16 = guarded(m, n), guarded(m, n, BF)
        recs = launched(lambda: ops.dense_fwd_ex(x, w, b, y[:m], act, drop_keep=drop, precision='bf16', storage=st,
                                                 out2=ops.second_output(y16[:m])))
        expect(y, m, n, ref, what=f'bf16 dense forward {cs.shape} act {act}')
        expect(y16, m, n, rne(ref), what=f'bf16 dense forward, rounded second output {cs.shape} act {act}')
        on_family(recs, RING, 'bf16 dense forward')
    st = ops.STORE_W | ops.STORE_X | ops.STORE_Y
    for second in (torch.float32, BF):
        for mask, scale in ((None, 1.0), (x, 2.0), (x, 3.0)):
            ref = rne(scale * cs.dx * (cs.x > 0 if mask is not None else 1))
            dx, dx2 = guarded(m, k, BF), guarded(m, k, second)
            recs = launched(lambda: ops.dense_bwd_data_ex(dz, w, dx[:m], mask=mask, scale=scale, precision='bf16', storage=st,
                                                          out2=ops.second_output(dx2[:m])))
            expect(dx, m, k, ref, what=f'bf16 dense rounded dx {cs.shape} scale {scale}')
            expect(dx2, m, k, ref, what=f'bf16 dense dx, second output {second} {cs.shape} scale {scale}')
            on_family(recs, RING, 'bf16 dense bwd-data')


# ---- rounded operands and the lo plane of bf16x3 ----
@pytest.mark.parametrize('precision,family', [('bf16x3', IGEMM_BF16X3), ('bf16', IGEMM_BF16)])
@pytest.mark.parametrize('wide', ['x', 'w', 'dz'])
@pytest.mark.parametrize('case', E.BF16_ARITH)
def test_one_wide_operand_on_float32_tensors(ops, case, wide, precision, family):
    """bf16: store_bf16 must round the wide operand to nearest even (the oracle on bf16_rne(operand)); bf16x3: hi lo and lo hi,
    never multiplied by anything but zero elsewhere, must restore the unrounded oracle"""
    cs = dict(E.wide_variants(case))[wide]
    conv_exact_f32_tensors(ops, cs.arith_bf16 if precision == 'bf16' else cs.arith_bf16x3, precision=precision, fwd=family, bwd_d=family,
                           bwd_f=family)


@pytest.mark.parametrize('precision,family', [('bf16x3', IGEMM_BF16X3), ('bf16', IGEMM_BF16)])
@pytest.mark.parametrize('case', E.BOTH_WIDE_CASES)
def test_both_operands_wide_on_float32_tensors(ops, case, precision, family):
    """odd integers in 257..511: every element is a bf16 tie and has lo = +-1.  bf16x3 must omit lo lo (non-zero in more than
    half of the outputs); bf16 must round every tie to even"""
    cs = E.conv_case(*case, mags=(E.BOTH_WIDE,) * 3)
    conv_exact_f32_tensors(ops, cs.arith_bf16 if precision == 'bf16' else cs.arith_bf16x3, precision=precision, fwd=family, bwd_d=family,
                           bwd_f=family)


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_IMAGE)
def test_filter_packs_of_the_bf16_image_form_round_a_wide_filter(ops, case):
    """conv3b_pack_kernel (>= 33 filters) and the image-form pack of the bf16 implicit GEMM, per call and prepared: the float32
    filter is wide, the reference the oracle on bf16_rne(w) — stored as bf16, so rounded once more"""
    cs = E.conv_case(*case, mags=(1, E.WIDE_OPERAND, 1)).arith_bf16
    bf16_image_form_exact(ops, cs.view('y stored as bf16', rounds=True), ties=0)


@pytest.mark.parametrize('case', E.POOLED_BWDF)
def test_few_channel_filter_gradient_rounds_a_wide_image(ops, case):
    """fewch16.hip converts the float32 image itself (packed convert of neighbouring taps): dw is the oracle on bf16_rne(x)"""
    cs = E.pooled_bwdf_case(*case, xmag=E.WIDE_OPERAND)
    n, h, w, c, k, ks, st, ld, lda = case
    x, arg = dev(cs.x), torch.from_numpy(cs.arg).cuda()
    dpool, pooled = dev(cs.dpool, BF), dev(cs.pooled, BF)
    for precision, family, ref in (('fp32', FEWCH, cs.dw), ('bf16', FEWCH16, cs.dw16)):
        d = ops.conv_desc(n, h, w, c, k, ks, ks, st, 'VALID', precision=precision)
        assert ops.conv2d_bwd_filter_pooled_supported(d)
        dw, db = guarded(ks * ks * c, k), guarded(1, k)
        on_family(launched(lambda: ops.conv2d_bwd_filter_pooled(d, x, dpool, pooled, arg, dw[:ks * ks * c].view(ks, ks, c, k), db[0])),
                  family, f'pool-fused filter gradient {precision}')
        expect(dw, ks * ks * c, k, ref, what=f'pool-fused dw {precision} {case}, x wide')
        expect(db, 1, k, cs.db, what=f'pool-fused db {precision} {case}')


@pytest.mark.parametrize('wide', ['x', 'dz'])
@pytest.mark.parametrize('m,k,n', E.DENSE_STREAM_BF16)
def test_dense_streaming_filter_gradient_rounds_a_wide_operand(ops, m, k, n, wide):
    """dense.hip's bf16 form (a3d_dense_bwd_filter_adam_tf1_ex, more than 32 rows): x is rounded while it is parked in LDS, dz
    into packed registers.  With beta1 = 0 and a zero m slot, ApplyAdam's m = 0 + (g - 0) 1 is the gradient itself: the oracle
    on bf16_rne(operand); the bias slot is the sum of the UNROUNDED dz (BiasAddGrad stays float32); alpha = 0 leaves var and v."""
    cs = E.dense_case(m, k, n, (E.WIDE_OPERAND, 1, 1) if wide == 'x' else (1, 1, E.WIDE_OPERAND))
    for precision, ref in (('fp32', cs.dw), ('bf16', rne(cs.x).T @ rne(cs.dz))):
        m_w, m_b = guarded(k, n), guarded(1, n)
        m_w[:k] = 0
        m_b[0] = 0
        var_w, v_w, var_b, v_b = (torch.full(shape, 0.25, device='cuda') for shape in ((k, n), (k, n), (n,), (n,)))
        ops.dense_bwd_filter_adam_tf1(dev(cs.x), dev(cs.dz), var_w, m_w[:k], v_w, var_b, m_b[0], v_b, 0.1, 0.0, 1.0, 0.0, 1.0, 1.0,
                                      precision=precision)
        expect(m_w, k, n, ref, what=f'dense filter gradient {precision} {cs.shape}, {wide} wide')
        expect(m_b, 1, n, cs.db, what=f'dense bias gradient {precision} {cs.shape}')
        assert all((t == 0.25).all() for t in (var_w, v_w, var_b, v_b))
