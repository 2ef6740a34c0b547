"""The conv, pool and cast routes on tensors between 2 and 8 GiB, held to exact results over the WHOLE tensor.

check_desc admits every tensor below 2^31 ELEMENTS (8 GiB of float32) while the kernels address through buffer descriptors with
31-bit BYTE offsets: each route either re-bases its descriptors (per tile, per image, per band) or is declined on the host at
2 GiB.  These cases put an operand on both sides of byte 2^31 and byte 2^32 and assert, per route, that the result is the float64
reference bit for bit and which kernel family ran (the timing record), or that the documented decline / refusal happened.

Method (tests/large_cases.py): image i of every big tensor is template i mod 7; the float64 reference of the 7 templates is
uploaded once and compared with EVERY image on the device, slab by slab (torch.ne, no tolerance, nothing sampled).  An offset that
wraps or is cut moves an access by a number of images that is no multiple of 7 (asserted per operand), i.e. onto another
template.  Filter gradients take dz = 0 outside 8 chosen images (around bytes 2^31 and 2^32, first and last).  Operands are small
integers whose sums stay below 2^24 (asserted), so every arithmetic and summation order gives the same bits.  Every big output is
a view 64 KiB into a NaN-filled (argmax bytes: 9) allocation with 64 KiB behind it; the guards and the pad columns of pitched
outputs must keep the sentinel.

2^32 bytes of a bf16 tensor would be 2^31 elements, which check_desc refuses: the bf16 cases pass 2^31 bytes only."""
import numpy as np
import pytest
import torch

import exact_ops as E
import large_cases as L
from oracle import tf13_ops as T
from pointwise_ref import bf16_values
from test_gpu_exact import (CONV3, FEWCH, FEWCH16, IGEMM_BF16, IGEMM_BF16X3, IGEMM_F32, RING, launched, on_family, ops)  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

NAN = float('nan')
F32, BF, U8 = torch.float32, torch.bfloat16, torch.uint8
ESZ = {F32: 4, BF: 2, U8: 1}
GIB = 1 << 30
SLAB_BYTES = 1 << 28          # what a comparison or a fill keeps live beside the tensors
PEAK_LIMIT = 16 * GIB
ARG_FILL = 9                  # sentinel of uint8 tensors


@pytest.fixture(autouse=True)
def device_memory():
    """frees what the test (and the workspace it grew) held, and holds the test to 16 GiB of device memory"""
    from ann3depth_amd import ops as O
    O._WS.clear()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    O._WS.clear()
    torch.cuda.empty_cache()
    print(f'peak device memory {peak / GIB:.2f} GiB')
    assert peak <= PEAK_LIMIT, f'peak device memory {peak / GIB:.2f} GiB'


def need(gib):
    """the one permitted skip: less free device memory than the case states it needs (none on an MI355X)"""
    free = torch.cuda.mem_get_info()[0]
    if free < gib * GIB:
        pytest.skip(f'needs {gib} GiB of device memory, {free / GIB:.1f} free')


def sentinel(dtype):
    return ARG_FILL if dtype == U8 else NAN


def is_sentinel(t):
    return (t == ARG_FILL) if t.dtype == U8 else torch.isnan(t)


class Guarded:
    """a tensor of `shape` 64 KiB into a sentinel-filled allocation, with 64 KiB behind it (byte_off: the view starts that many
    bytes later — an operand off the 16-byte grid)"""

    def __init__(self, shape, dtype=F32, byte_off=0):
        g = L.GUARD_BYTES // ESZ[dtype]
        self.numel = int(np.prod(shape))
        self.first = g + byte_off // ESZ[dtype]
        self.alloc = torch.full((self.first + self.numel + g,), sentinel(dtype), dtype=dtype, device='cuda')
        self.t = self.alloc[self.first:self.first + self.numel].view(shape)
        assert self.t.data_ptr() == self.alloc.data_ptr() + self.first * ESZ[dtype]

    def intact(self, what):
        assert bool(is_sentinel(self.alloc[:self.first]).all()), f'{what}: bytes in front of the tensor were written'
        assert bool(is_sentinel(self.alloc[self.first + self.numel:]).all()), f'{what}: bytes behind the tensor were written'


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32 if dtype != U8 else np.uint8)).cuda().to(dtype)


def stored(what, a, dtype):
    """a reference as the device tensor of `dtype` it must equal: a bf16 tensor holds integers up to 256 exactly"""
    if dtype == BF:
        E.require_bf16(what, np.asarray(a))
    return dev(a, dtype)


def images(t, n):
    """[n, pixels, ld] view of an NHWC (or flat) tensor of n images"""
    return t.view(n, -1, t.shape[-1])


def template_index(n):
    return torch.arange(n, device='cuda') % L.NT


def fill_templates(big, tem, c0=0):
    """image i of big [n, pixels, ld] takes template i mod 7 in its channels c0 .. c0 + c (tem [7, pixels, c]): with one
    index_select straight into the tensor where the templates have its pitch, slab by slab otherwise; nothing else is written"""
    n, pix, ld = big.shape
    assert tem.shape[:2] == (L.NT, pix) and tem.dtype == big.dtype
    L.shift_condition('operand', pix * ld * ESZ[big.dtype])
    idx = template_index(n)
    if tem.shape[2] == ld:
        ptr = big.data_ptr()
        torch.index_select(tem, 0, idx, out=big)
        assert big.data_ptr() == ptr and tuple(big.shape) == (n, pix, ld)
    else:
        step = max(1, SLAB_BYTES // (pix * tem.shape[2] * ESZ[big.dtype]))
        for i0 in range(0, n, step):
            big[i0:i0 + step, :, c0:c0 + tem.shape[2]] = tem[idx[i0:i0 + step]]
    return big


def templated(n, tem, dtype=F32, ld=None, pad=5.0):
    """a big input [n, pixels, ld] filled from the host templates tem [7, ..., c] (pad columns: a finite value no kernel may use)"""
    t = np.asarray(tem)
    c = t.shape[-1]
    d = stored('input', t.reshape(L.NT, -1, c), dtype)
    ld = ld or c
    assert L.fits(n, d.shape[1], ld)
    big = torch.empty((n, d.shape[1], ld), dtype=dtype, device='cuda') if ld == c else torch.full((n, d.shape[1], ld), pad, dtype=dtype, device='cuda')
    return fill_templates(big, d)


def assert_templates(out, ref, what, c0=0):
    """EVERY image i of out [n, pixels, ld] equals ref[i mod 7] [pixels, c] in its channels c0 .. c0 + c, and every other column
    holds the sentinel; torch.ne over the whole tensor in slabs of images, no tolerance"""
    n, pix, ld = out.shape
    c = ref.shape[2]
    assert ref.shape[:2] == (L.NT, pix) and ref.dtype == out.dtype and not bool(is_sentinel(ref).any())
    L.shift_condition(what, pix * ld * ESZ[out.dtype])
    idx = template_index(n)
    bad = torch.zeros(n, dtype=torch.bool, device='cuda')
    step = max(1, SLAB_BYTES // (pix * ld * ESZ[out.dtype]))
    for i0 in range(0, n, step):
        got = out[i0:i0 + step]
        bad[i0:i0 + step] = (got[:, :, c0:c0 + c] != ref[idx[i0:i0 + step]]).flatten(1).any(1)      # (NaN != x: an unwritten element differs)
        if c0:
            bad[i0:i0 + step] |= (~is_sentinel(got[:, :, :c0])).flatten(1).any(1)
        if c0 + c < ld:
            bad[i0:i0 + step] |= (~is_sentinel(got[:, :, c0 + c:])).flatten(1).any(1)
    wrong = torch.nonzero(bad).flatten().cpu().tolist()
    assert not wrong, (f'{what}: {len(wrong)} of {n} images differ from their template (image i holds template i mod {L.NT}), the first '
                       f'{wrong[:8]}; image bytes {pix * ld * ESZ[out.dtype]}: byte 2^31 lies in image {L.LINE31 // (pix * ld * ESZ[out.dtype])}, '
                       f'byte 2^32 in image {L.LINE32 // (pix * ld * ESZ[out.dtype])}')


def chosen_only(n, pixels, ld, imgs, values, dtype=F32):
    """a big gradient tensor [n, pixels, ld]: zero but for the chosen images"""
    big = torch.zeros((n, pixels, ld), dtype=dtype, device='cuda')
    v = stored('gradient', np.asarray(values).reshape(len(imgs), pixels, -1), dtype)
    big[torch.tensor(imgs, device='cuda'), :, :v.shape[2]] = v
    return big


def small_equal(got, want, what):
    """a small output (dw, db) in a guarded allocation against its float64 reference, element by element"""
    np.testing.assert_array_equal(got.t.double().cpu().numpy(), np.asarray(want, np.float64).reshape(tuple(got.t.shape)), err_msg=what)
    got.intact(what)


def families(recs):
    return sorted({(r.prec, r.lds_dma) for r in recs})


def report(what, recs):
    print(f'{what}: ' + ', '.join(f'mode {r.mode} prec {r.prec} lds_dma {r.lds_dma} {r.bm}x{r.bn} splitk {r.splitk} {r.ms:.2f} ms' for r in recs))


def conv_desc(ops, n, g, **kw):
    d = ops.conv_desc(n, g['h'], g['w'], g['c'], g['k'], g['ks'], g['ks'], g['st'], g['pad'], **kw)
    assert L.fits(n, d.h * d.w, d.ldx) and L.fits(n, d.ho * d.wo, d.ldy)
    return d


def geom(g):
    return tuple(g[k] for k in ('h', 'w', 'c', 'k', 'ks', 'st', 'pad'))


# ------------------------------------------------------------------------------------------------ 1. generic implicit GEMM
PRECISIONS = {'fp32': IGEMM_F32, 'bf16x3': IGEMM_BF16X3, 'bf16': IGEMM_BF16}


@pytest.mark.parametrize('precision,ldy', [(p, None) for p in PRECISIONS] + [('fp32', L.GENERIC_LDY)],
                         ids=list(PRECISIONS) + ['fp32-pitched'])
def test_generic_forward(ops, precision, ldy):
    """bias + ReLU; x 4.33 GB, y 4.33 GB (pitched: 5.41 GB).  igemm.h / igemm_bf16.h re-base the A descriptor at the image of each
    tile's first pixel with a 64-bit sum; the epilogue's descriptor starts at the tile's first row (size_t)."""
    need(12)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision=precision, ldy=ldy)
    assert L.straddles(n, d.h * d.w * d.c * 4, L.LINE32) and L.straddles(n, d.ho * d.wo * d.ldy * 4, L.LINE32)
    x = templated(n, tm.x)
    y = Guarded((n, d.ho, d.wo, d.ldy))
    recs = launched(lambda: ops.conv2d_fwd(d, x.view(n, d.h, d.w, d.c), dev(tm.w), dev(tm.b), y.t, 'relu'))
    report(f'generic forward {precision}', recs)
    assert_templates(images(y.t, n), stored('y', tm.relu_y.reshape(L.NT, -1, d.k), F32), f'generic forward {precision}')
    y.intact('generic forward')
    on_family(recs, PRECISIONS[precision], f'generic forward {precision}')
    del x, y


@pytest.mark.parametrize('precision', list(PRECISIONS))
def test_generic_bwd_data(ops, precision):
    """with the ReluGrad mask of the layer below: dz, the mask x and dx are 4.33 GB each"""
    need(15)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision=precision)
    dz, x = templated(n, tm.dz), templated(n, tm.x)
    dx = Guarded((n, d.h, d.w, d.c))
    recs = launched(lambda: ops.conv2d_bwd_data(d, dz.view(n, d.ho, d.wo, d.k), dev(tm.w), dx.t, relu_mask=x.view(n, d.h, d.w, d.c)))
    report(f'generic bwd-data {precision}', recs)
    assert_templates(images(dx.t, n), stored('dx', tm.masked_dx.reshape(L.NT, -1, d.c), F32), f'generic bwd-data {precision}')
    dx.intact('generic bwd-data')
    on_family(recs, PRECISIONS[precision], f'generic bwd-data {precision}')
    del dz, x, dx


@pytest.mark.parametrize('precision', list(PRECISIONS))
def test_generic_bwd_filter(ops, precision):
    """dw and db over 67.6 M pixels of which 8 images are non-zero: before / at / after bytes 2^31 and 2^32 of dz, first, last"""
    need(10)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision=precision)
    imgs, dzv, dw_ref, db_ref = tm.filter_grad(n, d.ho * d.wo * d.k * 4)
    assert len(imgs) == 8
    x = templated(n, tm.x)
    dz = chosen_only(n, d.ho * d.wo, d.k, imgs, dzv)
    dw, db = Guarded((d.r, d.s, d.c, d.k)), Guarded((d.k,))
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x.view(n, d.h, d.w, d.c), dz.view(n, d.ho, d.wo, d.k), dw.t, db.t))
    report(f'generic bwd-filter {precision}', recs)
    small_equal(dw, dw_ref, f'generic dw {precision}, chosen images {imgs}')
    small_equal(db, db_ref, f'generic db {precision}')
    on_family(recs, PRECISIONS[precision], f'generic bwd-filter {precision}')
    del x, dz


# ------------------------------------------------------------------------------------------------ 2. bf16 storage: the LDS-DMA kernels
def stored16(ops):
    return ops.STORE_X | ops.STORE_W | ops.STORE_Y


@pytest.mark.parametrize('ldy', [None, L.RING_LDY], ids=['dense', 'pitched'])
def test_bf16_stored_forward(ops, ldy):
    """igemm_ring.h: x and y 2.16 GB of bf16 (pitched y: 3.24 GB); the A descriptor is re-based at the tile's image"""
    need(8)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision='bf16', storage=stored16(ops), ldy=ldy)
    assert L.straddles(n, d.h * d.w * d.c * 2, L.LINE31)
    x = templated(n, tm.x, BF)
    y = Guarded((n, d.ho, d.wo, d.ldy), BF)
    recs = launched(lambda: ops.conv2d_fwd(d, x.view(n, d.h, d.w, d.c), dev(tm.w, BF), dev(tm.b), y.t, 'relu'))
    report('bf16-stored forward', recs)
    assert_templates(images(y.t, n), stored('y', tm.relu_y.reshape(L.NT, -1, d.k), BF), 'bf16-stored forward')
    y.intact('bf16-stored forward')
    on_family(recs, RING, 'bf16-stored forward')
    del x, y


def test_bf16_stored_bwd_data(ops):
    need(8)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision='bf16', storage=stored16(ops))
    dz, x = templated(n, tm.dz, BF), templated(n, tm.x, BF)
    dx = Guarded((n, d.h, d.w, d.c), BF)
    recs = launched(lambda: ops.conv2d_bwd_data(d, dz.view(n, d.ho, d.wo, d.k), dev(tm.w, BF), dx.t, relu_mask=x.view(n, d.h, d.w, d.c)))
    report('bf16-stored bwd-data', recs)
    assert_templates(images(dx.t, n), stored('dx', tm.masked_dx.reshape(L.NT, -1, d.c), BF), 'bf16-stored bwd-data')
    dx.intact('bf16-stored bwd-data')
    on_family(recs, RING, 'bf16-stored bwd-data')
    del dz, x, dx


def test_bf16_stored_bwd_filter_of_the_same_layer(ops):
    """144 rows of M: the planner keeps this filter gradient on igemm_bf16.h (re-based per k-tile), never on the LDS-DMA kernel,
    which addresses both tensors from their first byte"""
    need(6)
    g = L.GENERIC
    n, tm = g['n'], L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision='bf16', storage=ops.STORE_X | ops.STORE_Y)
    imgs, dzv, dw_ref, db_ref = tm.filter_grad(n, d.ho * d.wo * d.k * 2)
    x = templated(n, tm.x, BF)
    dz = chosen_only(n, d.ho * d.wo, d.k, imgs, dzv, BF)
    dw, db = Guarded((d.r, d.s, d.c, d.k)), Guarded((d.k,))
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x.view(n, d.h, d.w, d.c), dz.view(n, d.ho, d.wo, d.k), dw.t, db.t))
    report('bf16-stored bwd-filter', recs)
    small_equal(dw, dw_ref, f'bf16-stored dw, chosen images {imgs}')
    small_equal(db, db_ref, 'bf16-stored db')
    on_family(recs, IGEMM_BF16, 'bf16-stored bwd-filter')
    del x, dz


@pytest.mark.parametrize('n', L.RING_BWD_F_N)
def test_lds_dma_filter_gradient_on_both_sides_of_2_gib(ops, n):
    """A layer the LDS-DMA kernel does take (576 rows, 128 filters): igemm_ring.h addresses x AND dz of a filter gradient from the
    tensor's first byte, pieces at 2^31 or beyond read as zeros.  dz is twice as wide as x here, so dz passes 2^31 bytes while x
    stays under it: under the line the LDS-DMA kernel runs, over it the host must decline to igemm_bf16.h."""
    need(5)
    g = L.RING_BWD_F
    tm = L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, precision='bf16', storage=ops.STORE_X | ops.STORE_Y)
    dz_image = d.ho * d.wo * d.k * 2
    over = L.straddles(n, dz_image, L.LINE31)
    assert over == (n == L.RING_BWD_F_N[1]) and not L.straddles(n, d.h * d.w * d.c * 2, L.LINE31)
    imgs, dzv, dw_ref, db_ref = tm.filter_grad(n, dz_image)
    assert not over or {L.LINE31 // dz_image, L.LINE31 // dz_image + 1} <= set(imgs)
    x = templated(n, tm.x, BF)
    dz = chosen_only(n, d.ho * d.wo, d.k, imgs, dzv, BF)
    dw, db = Guarded((d.r, d.s, d.c, d.k)), Guarded((d.k,))
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x.view(n, d.h, d.w, d.c), dz.view(n, d.ho, d.wo, d.k), dw.t, db.t))
    report(f'LDS-DMA filter gradient n {n}', recs)
    small_equal(dw, dw_ref, f'dw, n {n}, chosen images {imgs}')
    small_equal(db, db_ref, f'db, n {n}')
    on_family(recs, IGEMM_BF16 if over else RING, f'filter gradient with dz {"over" if over else "under"} 2^31 bytes')
    del x, dz


# ------------------------------------------------------------------------------------------------ 3. few-channel forward (conv3.hip)
@pytest.mark.parametrize('form', ['per-call', 'prepared', 'pitched'])
def test_few_channel_forward_with_a_big_output(ops, form):
    """DCNF's first layer: x 252 MB (one descriptor over all of it: under 2^31 bytes by conv3_applicable), y 4.35 GB through
    size_t element offsets"""
    need(7)
    g = L.DCNF_FIRST
    n, tm = L.CONV3_N, L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g, ldy=L.CONV3_LDY if form == 'pitched' else None)
    assert L.straddles(n, d.ho * d.wo * d.ldy * 4, L.LINE32)
    x = templated(n, tm.x).view(n, d.h, d.w, d.c)
    wt, b = dev(tm.w), dev(tm.b)
    y = Guarded((n, d.ho, d.wo, d.ldy))
    if form == 'per-call':
        recs = launched(lambda: ops.conv2d_fwd(d, x, wt, b, y.t, 'relu'))
    else:
        pf = ops.PreparedFilter(d, x.device)
        assert pf.ok
        pf.refresh(wt)
        recs = launched(lambda: ops.conv2d_fwd(pf.desc_prepared, x, pf.buf, b, y.t, 'relu'))
    report(f'few-channel forward {form}', recs)
    assert_templates(images(y.t, n), stored('y', tm.relu_y.reshape(L.NT, -1, d.k), F32), f'few-channel forward {form}')
    y.intact('few-channel forward')
    on_family(recs, CONV3, f'few-channel forward {form}')
    del x, y


def test_few_channel_fused_pool_with_a_big_output(ops):
    """conv + ReLU + 2x2 max pool in one launch.  check_desc counts the unpooled y (n ho wo ldy < 2^31 - 1) although the call never
    writes it: 4142 images are the most it admits — a pooled map of 4.30 GB (n = 8300) is refused in words — so the pooled map
    passes 2^31 bytes by its pitch of 72 (2.42 GB, argmax bytes 0.54 GB).  Both against the first maximum of the float64 conv
    output (ties at 0 in every template)"""
    need(5)
    from ann3depth_amd._lib import A3dError
    g = L.DCNF_FIRST
    n, ld, tm = L.POOLED_N, L.CONV3_POOL_LD, L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g)
    ph, pw = d.ho // 2, d.wo // 2
    pooled, arg = tm.pooled
    assert L.straddles(n, ph * pw * ld * 4, L.LINE31) and not L.fits(n + 1, d.ho * d.wo, d.k)
    x = templated(n, tm.x).view(n, d.h, d.w, d.c)
    p, a = Guarded((n, ph, pw, ld)), Guarded((n, ph, pw, d.k), U8)
    recs = launched(lambda: ops.conv2d_pool_fwd(d, x, dev(tm.w), dev(tm.b), p.t, 'relu', a.t))
    report('few-channel fused pool', recs)
    assert_templates(images(p.t, n), stored('pooled', pooled.reshape(L.NT, -1, d.k), F32), 'fused pool: pooled map')
    assert_templates(images(a.t, n), dev(arg.reshape(L.NT, -1, d.k), U8), 'fused pool: argmax bytes')
    p.intact('pooled map')
    a.intact('argmax bytes')
    on_family(recs, CONV3, 'few-channel fused pool')
    for refused in L.POOLED_REFUSED_N:
        e = ops.conv_desc(refused, g['h'], g['w'], g['c'], g['k'], g['ks'], g['ks'], g['st'], g['pad'])
        with pytest.raises(A3dError, match='31-bit indexing'):
            ops.conv2d_pool_fwd(e, x, dev(tm.w), dev(tm.b), p.t, 'relu', a.t)
    del x, p, a


# ------------------------------------------------------------------------------------------------ 4. few-channel filter gradients
@pytest.mark.parametrize('n', L.FEWCH_PLAIN_N)
def test_few_channel_filter_gradient_on_both_sides_of_2_gib(ops, n):
    """fewch.hip holds one descriptor over the whole dz: under 2^31 bytes it runs, over it the front end falls back to the implicit
    GEMM (fewch_extents_ok)"""
    need(4)
    g = L.DCNF_FIRST
    tm = L.conv_templates(*geom(g))
    d = conv_desc(ops, n, g)
    dz_image = d.ho * d.wo * d.k * 4
    over = L.straddles(n, dz_image, L.LINE31 - 1)
    assert over == (n == L.FEWCH_PLAIN_N[1])
    imgs, dzv, dw_ref, db_ref = tm.filter_grad(n, dz_image)
    x = templated(n, tm.x)
    dz = chosen_only(n, d.ho * d.wo, d.k, imgs, dzv)
    dw, db = Guarded((d.r, d.s, d.c, d.k)), Guarded((d.k,))
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x.view(n, d.h, d.w, d.c), dz.view(n, d.ho, d.wo, d.k), dw.t, db.t))
    report(f'few-channel filter gradient n {n}', recs)
    small_equal(dw, dw_ref, f'dw, n {n}, chosen images {imgs}')
    small_equal(db, db_ref, f'db, n {n}')
    on_family(recs, IGEMM_F32 if over else FEWCH, f'few-channel filter gradient with dz {"over" if over else "under"} 2^31 bytes')
    del x, dz


@pytest.mark.parametrize('side,dtype,precision', [(s, t, p) for t, p in (('f32', 'fp32'), ('bf16', 'fp32'), ('bf16', 'bf16')) for s in ('under', 'over')],
                         ids=lambda v: v)
def test_pool_fused_filter_gradient_on_both_sides_of_2_gib(ops, side, dtype, precision):
    """a3d_conv2d_bwd_filter_pooled: the pooled gradient and the pooled activations straddle 2^31 bytes — by their pitch, at the
    4142 images check_desc admits of this layer (it counts the unpooled gradient).  Under the line fewch.hip (fp32 arithmetic) or
    fewch16.hip (bf16 arithmetic on bf16 tensors) runs; over it the call is refused in words, before any launch: there is no
    other route that reads pooled tensors"""
    need(7)
    from ann3depth_amd._lib import A3dError
    g = L.DCNF_FIRST
    n, ld = L.POOLED_N, L.FEWCH_POOLED_LD[dtype][side == 'over']
    tdt = BF if dtype == 'bf16' else F32
    tm = L.pooled_grad_templates(g['h'], g['w'], g['c'], g['k'], g['ks'])
    d = conv_desc(ops, n, g, precision=precision)
    image = tm.ph * tm.pw * ld * ESZ[tdt]
    assert L.straddles(n, image, L.LINE31 - 1) == (side == 'over')
    assert ops.conv2d_bwd_filter_pooled_supported(d)          # (the query sees the descriptor, not the tensors' types and pitches)
    imgs, dpv, dw_ref, db_ref = tm.filter_grad(n, image)
    x = templated(n, tm.x).view(n, d.h, d.w, d.c)
    pooled = templated(n, tm.pooled, tdt, ld=ld).view(n, tm.ph, tm.pw, ld)
    arg = templated(n, tm.arg, U8).view(n, tm.ph, tm.pw, d.k)
    dpool = chosen_only(n, tm.ph * tm.pw, ld, imgs, dpv, tdt).view(n, tm.ph, tm.pw, ld)
    dw, db = Guarded((d.r, d.s, d.c, d.k)), Guarded((d.k,))
    if side == 'over':
        with pytest.raises(A3dError, match='pooled tensors of 2 GiB or more'):
            ops.conv2d_bwd_filter_pooled(d, x, dpool, pooled, arg, dw.t, db.t)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw.t).all()) and bool(torch.isnan(db.t).all()), 'a refused call wrote its outputs'
        return
    recs = launched(lambda: ops.conv2d_bwd_filter_pooled(d, x, dpool, pooled, arg, dw.t, db.t))
    report(f'pool-fused filter gradient {dtype} {precision} pitch {ld}', recs)
    small_equal(dw, dw_ref, f'pool-fused dw {dtype} {precision}, chosen images {imgs}')
    small_equal(db, db_ref, f'pool-fused db {dtype} {precision}')
    on_family(recs, FEWCH16 if precision == 'bf16' else FEWCH, f'pool-fused filter gradient {dtype} {precision}')
    del x, pooled, arg, dpool


# ------------------------------------------------------------------------------------------------ 5. one-filter stencils (stencil1.hip)
class StencilTemplates:
    def __init__(self):
        h, w, c = L.STENCIL['h'], L.STENCIL['w'], L.STENCIL['c']
        rng = np.random.default_rng(8100)
        self.x = L.distinct('stencil x', E.ternary(rng, (L.NT, h, w, c)))
        self.w = E.ternary(rng, (5, 5, c, 1))
        self.b = E.small_bias(rng, 1)
        self.y = T.conv2d_fwd(E.f64(self.x), E.f64(self.w), E.f64(self.b), 1, 'SAME')
        self.relu_y = L.distinct('stencil relu(y)', np.maximum(self.y, 0))
        self.dz = L.distinct('stencil dz', E.ternary(rng, self.y.shape))
        self.dx = T.conv2d_bwd_data(E.f64(self.dz), E.f64(self.w), self.x.shape, 1, 'SAME')
        self.masked_dx = L.distinct('stencil dx', self.dx * (self.x > 0))
        E.require_headroom('stencil forward', 25 * c, self.x, self.w, self.b)
        E.require_headroom('stencil bwd-data', 25, self.dz, self.w)

    def filter_grad(self, n):
        h, w, c = L.STENCIL['h'], L.STENCIL['w'], L.STENCIL['c']
        imgs = L.chosen_images(n, h * w * c * 4)
        rng = np.random.default_rng(8200 + n)
        dz = E.ternary(rng, (len(imgs), h, w, 1))
        x = self.x[[i % L.NT for i in imgs]]
        dw, db = T.conv2d_bwd_filter(E.f64(x), E.f64(dz), (5, 5, c, 1), 1, 'SAME')
        E.require_headroom('stencil bwd-filter', len(imgs) * h * w, x, dz)
        return imgs, dz, dw, db


@pytest.fixture(scope='module')
def stencil():
    return StencilTemplates()


def stencil_desc(ops, n):
    h, w, c = L.STENCIL['h'], L.STENCIL['w'], L.STENCIL['c']
    return ops.conv_desc(n, h, w, c, 1, 5, 5, 1, 'SAME')


@pytest.mark.parametrize('n,byte_off,ldy', [(L.STENCIL_MFMA_N[0], 0, 1), (L.STENCIL_MFMA_N[0], 8, 1), (L.STENCIL_MFMA_N[1], 0, 1), (L.STENCIL_N, 0, 2)],
                         ids=['mfma-under-2GiB', 'lanes-off-grid', 'lanes-over-2GiB', 'lanes-4.37GB-pitched'])
def test_one_filter_forward(ops, stencil, n, byte_off, ldy):
    """The MFMA form takes an x of less than 2^31 bytes on the 16-byte grid (its descriptor is re-based per band, the host line is
    stencil1_mfma_applicable's); past it, or off the grid, the lane-per-channel form runs on size_t offsets.  The stencils carry
    no timing record: equality on both sides of the line is the check.  The 4.37 GB case writes y at a pitch of 2."""
    need(6)
    h, w, c = L.STENCIL['h'], L.STENCIL['w'], L.STENCIL['c']
    d = ops.conv_desc(n, h, w, c, 1, 5, 5, 1, 'SAME', ldy=ldy)
    image = d.h * d.w * d.c * 4
    assert L.straddles(L.STENCIL_MFMA_N[1], image, L.LINE31 - 1) and not L.straddles(L.STENCIL_MFMA_N[0], image, L.LINE31 - 1)
    assert n != L.STENCIL_N or L.straddles(n, image, L.LINE32)
    xg = Guarded((n, d.h * d.w, d.c), byte_off=byte_off)
    fill_templates(xg.t, dev(stencil.x.reshape(L.NT, -1, d.c)))
    y = Guarded((n, d.ho, d.wo, ldy))
    recs = launched(lambda: ops.conv2d_fwd(d, xg.t.view(n, d.h, d.w, d.c), dev(stencil.w), dev(stencil.b), y.t, 'relu'))
    assert not recs, 'the stencils carry no timing record: the implicit GEMM ran'
    assert_templates(images(y.t, n), dev(stencil.relu_y.reshape(L.NT, -1, 1)), f'one-filter forward n {n}')
    y.intact('one-filter forward')
    xg.intact('x')
    del xg, y


def test_one_filter_bwd_filter(ops, stencil):
    """stencil1_bwdf_kernel over an x of 4.37 GB"""
    need(6)
    n = L.STENCIL_N
    d = stencil_desc(ops, n)
    imgs, dzv, dw_ref, db_ref = stencil.filter_grad(n)
    assert len(imgs) == 8
    x = templated(n, stencil.x)
    dz = chosen_only(n, d.ho * d.wo, 1, imgs, dzv)
    dw, db = Guarded((5, 5, d.c, 1)), Guarded((1,))
    recs = launched(lambda: ops.conv2d_bwd_filter(d, x.view(n, d.h, d.w, d.c), dz.view(n, d.ho, d.wo, 1), dw.t, db.t))
    assert not recs
    small_equal(dw, dw_ref, f'one-filter dw, chosen images {imgs}')
    small_equal(db, db_ref, 'one-filter db')
    del x, dz


@pytest.mark.parametrize('dx16', [False, True], ids=['dx-f32', 'dx-bf16'])
def test_one_filter_bwd_both_up_to_its_line(ops, stencil, dx16):
    """a3d_conv2d_bwd_both takes an x of at most 2^30 bytes (stencil1_bwd_both_applicable): the largest such batch is exact, dx
    over every image and dw / db by the chosen images; one image more, and the 4.37 GB case, are refused in words"""
    need(6)
    from ann3depth_amd._lib import A3dError
    n = L.STENCIL_BOTH_N[0]
    d = stencil_desc(ops, n)
    image = d.h * d.w * d.c * 4
    assert n * image <= GIB < (n + 1) * image and ops.conv2d_bwd_both_supported(d)
    for refused in (L.STENCIL_BOTH_N[1], L.STENCIL_N):
        assert not ops.conv2d_bwd_both_supported(stencil_desc(ops, refused))
    tdt = BF if dx16 else F32
    x = templated(n, stencil.x).view(n, d.h, d.w, d.c)
    dz = templated(n, stencil.dz).view(n, d.ho, d.wo, 1)
    # every image contributes here: n / 7 copies of each template (+ the first n mod 7 once more), still far below 2^24
    counts = np.bincount(np.arange(n) % L.NT, minlength=L.NT).astype(np.float64)
    per = [T.conv2d_bwd_filter(E.f64(stencil.x[t:t + 1]), E.f64(stencil.dz[t:t + 1]), (5, 5, d.c, 1), 1, 'SAME') for t in range(L.NT)]
    dw_ref = sum(c * p[0] for c, p in zip(counts, per))
    db_ref = sum(c * p[1] for c, p in zip(counts, per))
    assert n * d.ho * d.wo < E.F32_EXACT
    dw, db = Guarded((5, 5, d.c, 1)), Guarded((1,))
    dx = Guarded((n, d.h, d.w, d.c), tdt)
    ops.conv2d_bwd_both(d, x, dz, dev(stencil.w), dw.t, db.t, dx.t, relu_mask=True)
    torch.cuda.synchronize()
    assert_templates(images(dx.t, n), stored('dx', stencil.masked_dx.reshape(L.NT, -1, d.c), tdt), f'bwd_both dx bf16 {dx16}')
    dx.intact('bwd_both dx')
    small_equal(dw, dw_ref, 'bwd_both dw')
    small_equal(db, db_ref, 'bwd_both db')
    with pytest.raises(A3dError, match='x below 1 GiB'):
        ops.conv2d_bwd_both(stencil_desc(ops, L.STENCIL_BOTH_N[1]), x, dz, dev(stencil.w), dw.t, db.t, dx.t, relu_mask=True)
    del x, dz, dx


# ------------------------------------------------------------------------------------------------ 6. the max pool family
def pool_case():
    p = L.POOL
    return p['n'], p['h'], p['w'], p['c'], L.pool_templates(p['h'], p['w'], p['c'])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('ldy', [64, 72], ids=['dense', 'pitched'])
def test_maxpool_forward(ops, dtype, ldy):
    """pool.hip: size_t element offsets throughout; x 4.35 GB float32 (past 2^32 bytes), 2.18 GB bf16 (past 2^31)"""
    need(7)
    n, h, w, c, tm = pool_case()
    tdt = BF if dtype == 'bf16' else F32
    assert L.straddles(n, h * w * c * ESZ[tdt], L.LINE32 if tdt == F32 else L.LINE31)
    x = templated(n, tm.x, tdt).view(n, h, w, c)
    y = Guarded((n, h // 2, w // 2, ldy), tdt)
    (ops.maxpool2x2_fwd_bf16 if tdt == BF else ops.maxpool2x2_fwd)(x, y.t)
    torch.cuda.synchronize()
    assert_templates(images(y.t, n), stored('y', tm.y.reshape(L.NT, -1, c), tdt), f'maxpool forward {dtype}')
    y.intact('maxpool forward')
    del x, y


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'plain'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_maxpool_bwd(ops, dtype, relu):
    """MaxPoolGrad recomputing the first maximum from x (ties at 0 in the templates), with and without ReluGrad; dy at a pitch"""
    need(12)
    n, h, w, c, tm = pool_case()
    tdt = BF if dtype == 'bf16' else F32
    x = templated(n, tm.x, tdt).view(n, h, w, c)
    dy = templated(n, tm.dy, tdt, ld=c + 8).view(n, h // 2, w // 2, c + 8)
    dx = Guarded((n, h, w, c), tdt)
    if tdt == BF:
        ops.maxpool2x2_bwd_bf16(x, dy, dx.t, relu_mask=relu)
    else:
        ops.maxpool2x2_bwd(x, dy, dx.t, relu_mask=relu)
    torch.cuda.synchronize()
    assert_templates(images(dx.t, n), stored('dx', tm.dx[relu].reshape(L.NT, -1, c), tdt), f'maxpool bwd {dtype} relu {relu}')
    dx.intact('maxpool bwd')
    del x, dy, dx


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'plain'])
@pytest.mark.parametrize('form', ['vec4', 'scalar', 'bf16', 'bf16s'])
def test_maxpool_bwd_by_index(ops, form, relu):
    """from recorded argmax bytes and pooled values: the 16-byte form (uint32 counters behind its own guard), the scalar form
    (a pooled map whose pixel stride is off the 16-byte grid), bf16 pooled values with a float32 dx, bf16 throughout"""
    need(8)
    n, h, w, c, tm = pool_case()
    ph, pw = h // 2, w // 2
    tdt = BF if form in ('bf16', 'bf16s') else F32
    dxt = BF if form == 'bf16s' else F32
    ldy = {'vec4': c, 'scalar': c + 1, 'bf16': c + 1, 'bf16s': c + 8}[form]
    assert L.straddles(n, h * w * c * ESZ[dxt], L.LINE32 if dxt == F32 else L.LINE31)
    arg = templated(n, tm.arg, U8).view(n, ph, pw, c)
    y = templated(n, tm.pooled, tdt, ld=ldy).view(n, ph, pw, ldy)
    dy = templated(n, tm.dy, tdt, ld=ldy).view(n, ph, pw, ldy)
    dx = Guarded((n, h, w, c), dxt)
    ops.maxpool2x2_bwd_idx(arg, y, dy, dx.t, relu_mask=relu)
    torch.cuda.synchronize()
    assert_templates(images(dx.t, n), stored('dx', tm.dx_idx[relu].reshape(L.NT, -1, c), dxt), f'maxpool bwd by index {form} relu {relu}')
    dx.intact('maxpool bwd by index')
    del arg, y, dy, dx


# ------------------------------------------------------------------------------------------------ 7. row casts and channel copies
def cast_templates():
    """float32 values most of which no bf16 holds, with ties of both directions planted (no NaN: the comparison is !=)"""
    rows, ld = L.CAST_IMAGE
    rng = np.random.default_rng(8500)
    t = (rng.standard_normal((L.NT, rows, ld)) * 100).astype(np.float32)
    t[:, :, 0] = np.float32(257.0) * rng.choice((-1, 1), (L.NT, rows))       # ties down to 256
    t[:, :, 1] = np.float32(259.0) * rng.choice((-1, 1), (L.NT, rows))       # ties up to 260
    assert (bf16_values(t) != t).mean() > 0.9
    return L.distinct('cast templates', t)


@pytest.mark.parametrize('src16,dst16', [(False, False), (False, True), (True, False), (True, True)], ids=['f32-f32', 'f32-bf16', 'bf16-f32', 'bf16-bf16'])
def test_cast_rows(ops, src16, dst16):
    """rows of 63 columns at a pitch of 64 on both sides: the 64th column of dst is zeroed, the 64th of src never read; 1.07 G
    elements, so a float32 side passes 2^32 bytes and a bf16 side 2^31"""
    need(9)
    rows, ld = L.CAST_IMAGE
    n, cols = L.CAST_N, ld - 1
    assert n * rows * ld > GIB
    t = cast_templates()
    src_vals = bf16_values(t) if src16 else t
    want = (bf16_values(src_vals) if dst16 else src_vals).copy()
    want[:, :, cols:] = 0
    sdt, ddt = (BF if src16 else F32), (BF if dst16 else F32)
    src = fill_templates(torch.empty((n, rows, ld), dtype=sdt, device='cuda'), dev(src_vals, sdt))
    dst = Guarded((n * rows, ld), ddt)
    ops.cast_rows(src.view(n * rows, ld), dst.t, cols=cols)
    torch.cuda.synchronize()
    assert_templates(dst.t.view(n, rows, ld), dev(want, ddt), f'cast_rows bf16 {src16} -> bf16 {dst16}')
    dst.intact('cast_rows')
    del src, dst


@pytest.mark.parametrize('to_bf16', [True, False], ids=['f32-bf16', 'bf16-f32'])
def test_cast_bf16(ops, to_bf16):
    """the flat cast, with a tail of 3 elements behind 1.07 G (the last block's scalar part)"""
    need(7)
    rows, ld = L.CAST_IMAGE
    n, tail = L.CAST_N, 3
    t = cast_templates()
    src_vals = t if to_bf16 else bf16_values(t)
    want = bf16_values(t)
    sdt, ddt = (F32, BF) if to_bf16 else (BF, F32)
    count = n * rows * ld + tail
    src = torch.empty(count, dtype=sdt, device='cuda')
    fill_templates(src[:count - tail].view(n, rows, ld), dev(src_vals, sdt))
    src[count - tail:] = dev(src_vals[0, 0, :tail], sdt)
    dst = Guarded((count,), ddt)
    ops.cast_bf16(src, dst.t)
    torch.cuda.synchronize()
    assert_templates(dst.t[:count - tail].view(n, rows, ld), dev(want, ddt), f'cast_bf16 to bf16 {to_bf16}')
    assert torch.equal(dst.t[count - tail:], dev(want[0, 0, :tail], ddt)), 'cast_bf16: the tail'
    dst.intact('cast_bf16')
    del src, dst


@pytest.mark.parametrize('dst16', [False, True], ids=['f32', 'bf16'])
def test_copy_channel(ops, dst16):
    """channel 3 of a 4-channel float32 tensor into channel 1 of a 4-channel tensor: 2^28 + pixels, the other channels keep the
    sentinel"""
    need(9)
    pix, n = L.CHANNEL_PIXELS, L.CAST_N
    assert n * pix * 4 > GIB
    rng = np.random.default_rng(8600)
    t = L.distinct('copy_channel templates', (rng.standard_normal((L.NT, pix, 4)) * 100).astype(np.float32))
    ddt = BF if dst16 else F32
    want = t[:, :, 3:4]
    src = fill_templates(torch.empty((n, pix, 4), dtype=F32, device='cuda'), dev(t))
    dst = Guarded((n * pix, 4), ddt)
    ops.copy_channel(src.view(n * pix, 4), 3, dst.t, 1)
    torch.cuda.synchronize()
    assert_templates(dst.t.view(n, pix, 4), dev(bf16_values(want) if dst16 else want, ddt), f'copy_channel bf16 {dst16}', c0=1)
    dst.intact('copy_channel')
    del src, dst


def test_pad_channels_bf16(ops):
    """float32 [pixels, 3] -> bf16 [pixels, 4] with a zero 4th channel: 2^28 + pixels, dst past 2^31 bytes, src past 3 * 2^30"""
    need(6)
    pix, n = L.CHANNEL_PIXELS, L.CAST_N
    rng = np.random.default_rng(8700)
    t = L.distinct('pad_channels templates', (rng.standard_normal((L.NT, pix, 3)) * 100).astype(np.float32))
    want = np.concatenate([bf16_values(t), np.zeros((L.NT, pix, 1), np.float32)], axis=2)
    src = fill_templates(torch.empty((n, pix, 3), dtype=F32, device='cuda'), dev(t))
    dst = Guarded((n * pix, 4), BF)
    ops.pad_channels_bf16(src.view(n * pix, 3), dst.t)
    torch.cuda.synchronize()
    assert_templates(dst.t.view(n, pix, 4), dev(want, BF), 'pad_channels_bf16')
    dst.intact('pad_channels_bf16')
    del src, dst
