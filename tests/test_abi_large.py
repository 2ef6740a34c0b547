"""The lines the host draws around 31-bit byte offsets, one step under and one step over each, through queries and refusals that
launch nothing (no GPU needed: the checks come first, so host pointers are safe), and the host-side conditions of
tests/test_gpu_large_tensors.py (tests/large_cases.py), built and asserted here on the CPU.

check_desc counts ELEMENTS (`< 2147483647`: 2^31 - 2 is the largest tensor it admits, up to 8 GiB of float32); every route that
holds one buffer descriptor over a whole tensor counts BYTES against 2^31 - 1 and declines, or refuses in words, beyond."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import large_cases as L
from ann3depth_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (1 << 31) - 1          # the value every host check compares with
X, W, Y = ops.STORE_X, ops.STORE_W, ops.STORE_Y


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.fixture(scope='module')
def host():
    buf = ctypes.create_string_buffer(1 << 12)
    base = ctypes.addressof(buf)
    host.keep = buf
    return (base + 255) & ~255          # 256-byte aligned, so that no alignment check speaks first


def refused(lib, rc, why):
    """-1, and by the check meant"""
    assert rc == -1, rc
    assert why in _lib.last_error(), (why, _lib.last_error())


def desc(n, h, w, c, k, ks, st, pad, **kw):
    return ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, **kw)


def fwd_without_tensors(lib, d):
    """a3d_conv2d_fwd with null tensors: check_desc speaks first, 'null tensor' only for a descriptor it admits"""
    rc = lib.a3d_conv2d_fwd(ctypes.byref(d), None, None, None, None, 0, None, 0, None)
    assert rc == -1
    return _lib.last_error()


# ---- check_desc: elements ----
@pytest.mark.parametrize('under,over,exact', [
    # x: n x 1 x 1 x ldx
    (dict(n=(1 << 30) - 1, c=2, k=1), dict(n=1 << 30, c=2, k=1), dict(n=LINE, c=1, k=1)),
    # y: n x 1 x 1 x ldy
    (dict(n=(1 << 30) - 1, c=1, k=2), dict(n=1 << 30, c=1, k=2), dict(n=LINE, c=1, k=1)),
    # the filter: r x s x c x k over one pixel (2^31 - 2 = 331 * 151 * 198 * 217; a pixel of k floats must stay a small image)
    (dict(n=1, c=198, k=217, r=331, s=151), dict(n=1, c=1 << 15, k=1 << 16), dict(n=1, c=1, k=LINE)),
], ids=['x', 'y', 'filter'])
def test_check_desc_counts_elements(lib, under, over, exact):
    """2^31 - 2 elements are admitted, 2^31 - 1 and 2^31 are refused: for each of x, y and the filter"""
    make = lambda s: ops.conv_desc(s['n'], 1, 1, s['c'], s['k'], s.get('r', 1), s.get('s', 1), 1, 'SAME')
    sizes = lambda s: (s['n'] * s['c'], s['n'] * s['k'], s.get('r', 1) * s.get('s', 1) * s['c'] * s['k'])
    assert max(sizes(under)) == LINE - 1 and max(sizes(over)) == LINE + 1 and max(sizes(exact)) == LINE
    assert 'null tensor' in fwd_without_tensors(lib, make(under))
    for s in (over, exact):
        assert '31-bit indexing' in fwd_without_tensors(lib, make(s))
        d = make(s)
        for query in (lib.a3d_conv2d_fwd_ws_bytes, lib.a3d_conv2d_bwd_data_ws_bytes, lib.a3d_conv2d_bwd_filter_ws_bytes,
                      lib.a3d_conv2d_fwd_prepared_filter_bytes, lib.a3d_conv2d_bwd_filter_pooled_ws_bytes):
            assert query(ctypes.byref(d)) == 0
        assert not lib.a3d_conv2d_bwd_both_supported(ctypes.byref(d))


def test_check_desc_bounds_the_images_a_tile_reaches(lib):
    """The implicit-GEMM gathers hold int BYTE offsets from the image of a tile's first row: the images a tile of up to 256 rows
    reaches (one more than its rows cover) must lie within 2^31 bytes, whatever the element count"""
    under, over = desc(2, 8192, 8191, 4, 4, 3, 1, 'SAME'), desc(2, 8192, 8192, 4, 4, 3, 1, 'SAME')
    assert 2 * 8192 * 8191 * 4 * 4 < LINE <= 2 * 8192 * 8192 * 4 * 4 and 2 * 8192 * 8192 * 4 < LINE
    assert 'null tensor' in fwd_without_tensors(lib, under)
    assert 'single images too large' in fwd_without_tensors(lib, over)
    # rows of one pixel (a dense layer): 257 rows of k inputs
    k = LINE // (257 * 4)
    assert 'null tensor' in fwd_without_tensors(lib, desc(300, 1, 1, k, 1, 1, 1, 'VALID'))
    assert 'single images too large' in fwd_without_tensors(lib, desc(300, 1, 1, k + 1, 1, 1, 1, 'VALID'))
    # bwd-data gathers dz: the output side
    assert 'single images too large' in fwd_without_tensors(lib, desc(300, 1, 1, 1, k + 1, 1, 1, 'VALID'))
    # every case of the GPU file is far inside
    for g, n in ((L.GENERIC, L.GENERIC['n']), (L.DCNF_FIRST, L.POOLED_N), (L.RING_BWD_F, L.RING_BWD_F_N[1])):
        assert 'null tensor' in fwd_without_tensors(lib, desc(n, g['h'], g['w'], g['c'], g['k'], g['ks'], g['st'], g['pad']))


# ---- routes that hold one descriptor over a whole tensor: bytes ----
MSDN_FIRST = (228, 304, 3, 96, 11, 4, 'VALID')          # 831 744 bytes of x per image
MSDN_N = (2581, 2582)                                   # x: 2 146 731 264 bytes and 2 147 563 008


def test_few_channel_forward_declines_at_2_gib_of_x(lib):
    """conv3.hip: `n h w c 4 >= 2^31 - 1` declines; the prepared-filter query then answers for the window-run form"""
    image = 228 * 304 * 3 * 4
    assert MSDN_N[0] * image < LINE <= MSDN_N[1] * image
    small, under, over = (lib.a3d_conv2d_fwd_prepared_filter_bytes(ctypes.byref(desc(n, *MSDN_FIRST))) for n in (2,) + MSDN_N)
    assert small > 0 and under == small, 'conv3 repacks the filter into a layout that depends on the filter alone'
    assert over != small, 'past 2^31 - 1 bytes of x another forward answers'
    # ... and its own repack is the larger buffer: the launch then needs the workspace of that form
    assert lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(desc(MSDN_N[1], *MSDN_FIRST))) >= over


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_pool_fused_filter_gradient_declines_at_2_gib_of_x(lib, precision):
    """fewch.hip / fewch16.hip: the query answers 0 from the same line on"""
    under, over = (desc(n, *MSDN_FIRST, precision=precision) for n in MSDN_N)
    assert ops.conv2d_bwd_filter_pooled_supported(under) and lib.a3d_conv2d_bwd_filter_pooled_ws_bytes(ctypes.byref(under)) > 0
    assert not ops.conv2d_bwd_filter_pooled_supported(over) and lib.a3d_conv2d_bwd_filter_pooled_ws_bytes(ctypes.byref(over)) == 0


@pytest.mark.parametrize('dtype,precision', [('f32', 'fp32'), ('bf16', 'fp32'), ('bf16', 'bf16')])
def test_pool_fused_filter_gradient_refuses_pooled_tensors_of_2_gib(lib, host, dtype, precision):
    """the pooled tensors' own line depends on their type and pitch, which only the launch knows: refused there, in words"""
    g = L.DCNF_FIRST
    n, ld = L.POOLED_N, L.FEWCH_POOLED_LD[dtype][1]
    esz = 2 if dtype == 'bf16' else 4
    d = desc(n, g['h'], g['w'], g['c'], g['k'], g['ks'], g['st'], g['pad'], precision=precision)
    assert n * 45 * 45 * L.FEWCH_POOLED_LD[dtype][0] * esz < LINE < n * 45 * 45 * ld * esz and ops.conv2d_bwd_filter_pooled_supported(d)
    pooled = lambda ld, ld_arg: lib.a3d_conv2d_bwd_filter_pooled(ctypes.byref(d), host, host, ld, host, host, ld_arg, int(dtype == 'bf16'), host,
                                                                 host, host, 1 << 40, None)
    refused(lib, pooled(ld, 64), 'pooled tensors of 2 GiB or more')
    # the argmax bytes have a line of their own
    assert n * 45 * 45 * 256 < LINE < n * 45 * 45 * 257
    refused(lib, pooled(64, 257), 'pooled tensors of 2 GiB or more')


def test_the_unpooled_extent_bounds_the_pool_fused_calls(lib):
    """check_desc counts n ho wo ldy of the conv output that a pool-fused call never writes: one image past POOLED_N and the
    batch whose pooled map alone would pass 2^32 bytes are refused in words, by the query and by the forward"""
    g = L.DCNF_FIRST
    make = lambda n: desc(n, g['h'], g['w'], g['c'], g['k'], g['ks'], g['st'], g['pad'])
    assert L.POOLED_N * 90 * 90 * 64 < LINE <= L.POOLED_REFUSED_N[0] * 90 * 90 * 64 and L.POOLED_REFUSED_N[1] * 45 * 45 * 64 * 4 > 1 << 32
    assert ops.conv2d_bwd_filter_pooled_supported(make(L.POOLED_N))
    for n in L.POOLED_REFUSED_N:
        assert not ops.conv2d_bwd_filter_pooled_supported(make(n))
        rc = lib.a3d_conv2d_pool_fwd(ctypes.byref(make(n)), None, None, None, None, 64, None, 1, None, 0, None)
        refused(lib, rc, '31-bit indexing')


def test_one_filter_bwd_both_line(lib, host):
    """a3d_conv2d_bwd_both: x of at most 2^30 bytes"""
    s = L.STENCIL
    under, over = (desc(n, s['h'], s['w'], s['c'], 1, 5, 1, 'SAME') for n in L.STENCIL_BOTH_N)
    image = s['h'] * s['w'] * s['c'] * 4
    assert L.STENCIL_BOTH_N[0] * image <= 1 << 30 < L.STENCIL_BOTH_N[1] * image
    assert lib.a3d_conv2d_bwd_both_supported(ctypes.byref(under)) and lib.a3d_conv2d_bwd_both_ws_bytes(ctypes.byref(under)) > 0
    assert not lib.a3d_conv2d_bwd_both_supported(ctypes.byref(over)) and lib.a3d_conv2d_bwd_both_ws_bytes(ctypes.byref(over)) == 0
    rc = lib.a3d_conv2d_bwd_both(ctypes.byref(over), host, host, host, host, host, host, 64, 0, 1, host, host, 1 << 40, None)
    refused(lib, rc, 'x below 1 GiB')


# ---- Winograd ----
def test_winograd_declines_at_its_workspace_line(lib):
    """wino_applicable: T max(Kp, Np) 4 < 2^31 - 1 for the tiles T of both directions; beyond, 'fp32w' runs as 'fp32'"""
    n_under, n_over = (1 << 21) - 1, 1 << 21               # 1 x 1 images: T = n tiles, 256 channels
    assert n_under * 256 * 4 < LINE <= n_over * 256 * 4
    under, over = (desc(n, 1, 1, 256, 256, 3, 1, 'SAME', precision='fp32w') for n in (n_under, n_over))
    u_bytes = 16 * 256 * 256 * 4
    for query in (lib.a3dw_conv2d_bwd_data_prepared_filter_bytes, lib.a3d_conv2d_fwd_prepared_filter_bytes):
        assert query(ctypes.byref(under)) == u_bytes and query(ctypes.byref(over)) == 0
    v_bytes = 16 * n_under * 256 * 4                        # one transformed operand of the Winograd chain
    for prepared in (0, 1):
        assert lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(under), prepared, 0) > 2 * v_bytes
        generic = max(lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(over)), lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(over)))
        assert lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(over), prepared, 0) == generic < v_bytes


# ---- the LDS-DMA filter gradient ----
RING_QUERY = """
import ctypes, sys
sys.path.insert(0, %r)
from ann3depth_amd import _lib, ops
lib = _lib.load()
for n in %r:
    d = ops.conv_desc(n, %d, %d, %d, %d, 3, 3, 1, 'SAME', precision='bf16', storage=ops.STORE_X | ops.STORE_Y)
    print(lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)))
"""


def test_lds_dma_filter_gradient_declines_at_2_gib_of_dz():
    """igemm_ring.h addresses x and dz of a filter gradient from their first byte.  Under 2^31 bytes of dz the planner answers with
    the LDS-DMA kernel's slabs (another number than with that kernel turned off); over it, with x still under, it must answer as
    if the kernel were off"""
    g = L.RING_BWD_F
    dz_image, x_image = g['h'] * g['w'] * g['k'] * 2, g['h'] * g['w'] * g['c'] * 2
    assert L.RING_BWD_F_N[0] * dz_image < LINE < L.RING_BWD_F_N[1] * dz_image and L.RING_BWD_F_N[1] * x_image < LINE
    code = RING_QUERY % (ROOT, L.RING_BWD_F_N, g['h'], g['w'], g['c'], g['k'])
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    children = [subprocess.Popen([sys.executable, '-c', code], env=dict(env, **extra), stdout=subprocess.PIPE, text=True)
                for extra in ({}, {'A3D_TUNING': '1', 'A3D_RING': '0'})]
    (under, over), (under_off, over_off) = ([int(v) for v in c.communicate()[0].split()] for c in children)
    assert all(c.returncode == 0 for c in children)
    assert under != under_off, 'the case no longer reaches the LDS-DMA kernel under the line'
    assert over == over_off, 'past 2^31 bytes of dz the LDS-DMA kernel must not be planned'


# ---- resizes ----
def test_resizes_refuse_what_their_int_indices_cannot_hold(lib, host):
    """image bases are 64-bit; output rows (n oh) and the elements of one line are ints"""
    resize = lambda n, h, w, c, oh, ow: lib.a3d_resize_bilinear_tf1(n, h, w, c, host, oh, ow, host, None)
    refused(lib, resize(1 << 20, 4, 4, 1, 1 << 11, 4), 'image too large')          # n oh = 2^31
    refused(lib, resize(1, 4, 1 << 16, 1 << 15, 4, 4), 'image too large')           # w c = 2^31
    refused(lib, resize(1, 4, 4, 1 << 15, 4, 1 << 16), 'image too large')           # ow c = 2^31
    pair = lambda n, oh1: lib.a3d_resize_bilinear_tf1_pair(n, 4, 4, 3, host, 4, 4, host, 1, host, oh1, 4, host, None)
    refused(lib, pair(1 << 20, 1 << 11), 'image too large')                         # the second tensor's rows
    warp = lambda n, h, w, c: lib.a3d_warp_bilinear_pair(n, h, w, c, host, 0, 4, 4, host, 1, host, 0, 4, 4, host, host, None)
    refused(lib, warp(1, 1 << 15, 1 << 15, 3), 'image too large')                   # h w c > 2^31 - 1
    refused(lib, warp(1 << 28, 4, 4, 3), 'image too large')                         # n tables


# ---- the GPU file's cases: their conditions hold (asserted again on the GPU, where a failure would cost a run) ----
def big_operands():
    """(name, images, pixels per image, pixel stride, element bytes) of every template-filled or template-compared tensor"""
    g, d, r, p, s = L.GENERIC, L.DCNF_FIRST, L.RING_BWD_F, L.POOL, L.STENCIL
    out = []
    for esz in (4, 2):
        out += [('generic x / dx', g['n'], g['h'] * g['w'], g['c'], esz), ('generic y / dz', g['n'], g['h'] * g['w'], g['k'], esz)]
    out += [('generic y pitched', g['n'], g['h'] * g['w'], L.GENERIC_LDY, 4), ('ring y pitched', g['n'], g['h'] * g['w'], L.RING_LDY, 2)]
    out += [(f'ring bwd-f {t}', n, r['h'] * r['w'], c, 2) for n in L.RING_BWD_F_N for t, c in (('x', r['c']), ('dz', r['k']))]
    out += [('conv3 x', L.POOLED_N, 100 * 100, 3, 4), ('conv3 y', L.CONV3_N, 90 * 90, 64, 4), ('conv3 y pitched', L.CONV3_N, 90 * 90, L.CONV3_LDY, 4),
            ('conv3 pooled', L.POOLED_N, 45 * 45, L.CONV3_POOL_LD, 4), ('conv3 argmax', L.POOLED_N, 45 * 45, 64, 1)]
    out += [('fewch dz', n, 90 * 90, 64, 4) for n in L.FEWCH_PLAIN_N]
    out += [(f'fewch pooled {t}', L.POOLED_N, 45 * 45, ld, 4 if t == 'f32' else 2) for t, lds in L.FEWCH_POOLED_LD.items() for ld in lds]
    out += [('stencil x', n, s['h'] * s['w'], s['c'], 4) for n in (L.STENCIL_N,) + L.STENCIL_MFMA_N + L.STENCIL_BOTH_N]
    out += [('stencil dx bf16', L.STENCIL_BOTH_N[0], s['h'] * s['w'], s['c'], 2), ('stencil y', L.STENCIL_N, s['h'] * s['w'], 1, 4),
            ('stencil y pitched', L.STENCIL_N, s['h'] * s['w'], 2, 4)]
    for esz in (4, 2):
        out += [('pool x', p['n'], p['h'] * p['w'], p['c'], esz), ('pool y', p['n'], p['h'] * p['w'] // 4, p['c'], esz)]
        out += [(f'pool pitched {ld}', p['n'], p['h'] * p['w'] // 4, ld, esz) for ld in (p['c'] + 1, p['c'] + 8)]
        out += [('cast rows', L.CAST_N, L.CAST_IMAGE[0], L.CAST_IMAGE[1], esz), ('channels of 4', L.CAST_N, L.CHANNEL_PIXELS, 4, esz)]
    out += [('pool argmax', p['n'], p['h'] * p['w'] // 4, p['c'], 1), ('channels of 3', L.CAST_N, L.CHANNEL_PIXELS, 3, 4)]
    return out


def test_no_wrapped_or_cut_offset_lands_on_the_same_template():
    """per operand: under check_desc's element count, and a byte offset reduced mod 2^32, or cut at 2^31, moves every image to
    one of another template — over all images, not only by the condition on the two quotients"""
    for name, n, pixels, ld, esz in big_operands():
        assert L.fits(n, pixels, ld), name
        image = pixels * ld * esz
        L.shift_condition(name, image)
        first = np.arange(n, dtype=np.int64) * image             # byte offset of each image: what a 64-bit base holds
        for line in (L.LINE31, L.LINE32):
            lands = (first % line) // image                       # the image a base truncated to that many bits points into
            moved = first >= line
            assert ((lands[moved] - np.arange(n)[moved]) % L.NT != 0).all() or (first[moved] % line % image != 0).all(), (name, line)


def test_the_large_cases_build_and_straddle_their_lines():
    g = L.GENERIC
    tm = L.conv_templates(g['h'], g['w'], g['c'], g['k'], g['ks'], g['st'], g['pad'])
    for esz in (4, 2):
        imgs = tm.filter_grad(g['n'], g['h'] * g['w'] * g['k'] * esz)[0]
        assert len(imgs) == (8 if esz == 4 else 5) and imgs[0] == 0 and imgs[-1] == g['n'] - 1
    assert g['n'] * g['h'] * g['w'] * g['c'] * 4 > L.LINE32 and g['n'] * g['h'] * g['w'] * g['c'] * 2 > L.LINE31
    d = L.DCNF_FIRST
    tm = L.conv_templates(d['h'], d['w'], d['c'], d['k'], d['ks'], d['st'], d['pad'])
    assert tm.pooled[0].shape == (L.NT, 45, 45, 64)
    assert L.FEWCH_PLAIN_N[0] * 90 * 90 * 64 * 4 < LINE < L.FEWCH_PLAIN_N[1] * 90 * 90 * 64 * 4
    for t, (under, over) in L.FEWCH_POOLED_LD.items():
        esz = 4 if t == 'f32' else 2
        assert L.POOLED_N * 45 * 45 * under * esz < LINE < L.POOLED_N * 45 * 45 * over * esz and L.POOLED_N * 100 * 100 * 3 * 4 < LINE
        imgs = L.pooled_grad_templates(d['h'], d['w'], d['c'], d['k'], d['ks']).filter_grad(L.POOLED_N, 45 * 45 * over * esz)[0]
        assert len(imgs) == 5
    r = L.RING_BWD_F
    L.conv_templates(r['h'], r['w'], r['c'], r['k'], r['ks'], r['st'], r['pad']).filter_grad(L.RING_BWD_F_N[1], r['h'] * r['w'] * r['k'] * 2)
    p = L.POOL
    L.pool_templates(p['h'], p['w'], p['c'])
    s = L.STENCIL
    assert L.STENCIL_MFMA_N[0] * s['h'] * s['w'] * 64 * 4 < LINE <= L.STENCIL_MFMA_N[1] * s['h'] * s['w'] * 64 * 4
    assert L.CAST_N * L.CAST_IMAGE[0] * L.CAST_IMAGE[1] > 1 << 30 and L.CAST_N * L.CHANNEL_PIXELS * 4 > 1 << 30
