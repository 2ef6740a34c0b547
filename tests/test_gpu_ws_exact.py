"""Every conv / dense launch on EXACTLY the workspace its *_ws_bytes query returns.

include/a3d.h promises that a workspace of the size the matching query returns is enough.  ops.Workspace never allocates
less than 1 MiB, so the other tests run every launch whose query answers less on a roomier buffer than the promise names.
Here each entry point is called directly with a uint8 workspace of q + 4096 bytes filled with 0xA5 and ws_bytes = q (q == 0:
NULL, 0), q being the query's answer, and must return 0, leave the 4096 tail bytes alone, and give the bits the same call gives
through ops.* on the roomy workspace (same plan, same bits).

The cases are the smallest shapes at which each candidate of the front end (csrc/igemm_host.hip) needs a workspace below that
floor; operands are torch's own, 256-byte aligned (tests/test_gpu_exact_offgrid.py repeats the promise with every operand off
the 16-byte grid).  Stream-K plans need more than 1 MiB: the other tests already run them
on exactly q."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 1 << 20          # ops.Workspace's smallest allocation
TAIL = 4096
FILL = 0xA5
X, W, Y = 1, 2, 4        # a3d_conv_desc.storage bits
BF = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


def exact(lib, q, below_floor, ref, direct):
    """ref(): the outputs through ops.* ; direct(ws, ws_bytes) -> (rc, outputs) from the entry point itself."""
    from ann3depth_amd import _lib
    q = int(q)
    assert not below_floor or 0 < q < FLOOR, f'the query answers {q}: this case no longer sits below the 1 MiB floor'
    want = ref()
    buf = torch.full((q + TAIL,), FILL, dtype=torch.uint8, device='cuda') if q else None
    rc, got = direct(ctypes.c_void_p(buf.data_ptr()) if q else None, q)
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    if q:
        assert bool((buf[q:] == FILL).all()), 'the launch wrote past the bytes its query named'


class Conv:
    """Tensors of one conv case, in the types its storage bits name (a 4-channel bf16 image: a3d_pad_channels_bf16 of 3)."""

    def __init__(self, ops, n, h, w, c, k, ks, st, pad, precision='fp32', storage=0, ldy=None):
        self.ops, self.k = ops, k
        self.d = d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, ldy=ldy, precision=precision, storage=storage)
        self.D = ctypes.byref(d)
        rng = np.random.default_rng(n * 1000 + h * w + c + k)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        if c == 4 and storage & X:
            self.x = ops.pad_channels_bf16(dev(rng.random((n, h, w, 3))), torch.empty((n, h, w, 4), device='cuda', dtype=BF))
        else:
            self.x = dev(rng.standard_normal((n, h, w, c))).to(BF if storage & X else torch.float32)
        self.w = dev(rng.standard_normal((ks, ks, c, k)) * 0.1).to(BF if storage & W else torch.float32)
        self.bias = dev(rng.standard_normal(k) * 0.1)
        self.ydt = BF if storage & Y else torch.float32
        self.dz = dev(rng.standard_normal((n, d.ho, d.wo, d.ldy))).to(self.ydt)
        self.mask = dev(rng.standard_normal((n, h, w, c))).to(self.x.dtype)

    def out(self, *shape, dtype=torch.float32):
        return torch.full(shape, -3.0, device='cuda', dtype=dtype)

    def fwd(self, lib):
        ops, d, p = self.ops, self.d, self.ops._ptr
        new = lambda: self.out(d.n, d.ho, d.wo, d.ldy, dtype=self.ydt)
        exact(lib, lib.a3d_conv2d_fwd_ws_bytes(self.D), True,
              lambda: [ops.conv2d_fwd(d, self.x, self.w, self.bias, new(), 'relu')],
              lambda ws, nb: (lambda y: (lib.a3d_conv2d_fwd(self.D, p(self.x), p(self.w), p(self.bias), p(y), ops.ACT['relu'], ws, nb,
                                                            ops._stream()), [y]))(new()))

    def pool_fwd(self, lib, argmax):
        ops, d, p = self.ops, self.d, self.ops._ptr
        ph, pw = d.ho // 2, d.wo // 2
        new = lambda: (self.out(d.n, ph, pw, d.ldy, dtype=self.ydt),
                       torch.full((d.n, ph, pw, d.k), 9, device='cuda', dtype=torch.uint8) if argmax else None)

        def ref():
            y, a = new()
            ops.conv2d_pool_fwd(d, self.x, self.w, self.bias, y, 'relu', a)
            return [y] + ([a] if argmax else [])

        def direct(ws, nb):
            y, a = new()
            rc = lib.a3d_conv2d_pool_fwd(self.D, p(self.x), p(self.w), p(self.bias), p(y), d.ldy, p(a), ops.ACT['relu'], ws, nb,
                                         ops._stream())
            return rc, [y] + ([a] if argmax else [])
        exact(lib, lib.a3d_conv2d_fwd_ws_bytes(self.D), True, ref, direct)

    def bwd_data(self, lib, mask, below_floor=True):
        ops, d, p = self.ops, self.d, self.ops._ptr
        m = self.mask if mask else None
        new = lambda: self.out(d.n, d.h, d.w, d.ldx, dtype=self.x.dtype)
        exact(lib, lib.a3d_conv2d_bwd_data_ws_bytes(self.D), below_floor,
              lambda: [ops.conv2d_bwd_data(d, self.dz, self.w, new(), m)],
              lambda ws, nb: (lambda dx: (lib.a3d_conv2d_bwd_data(self.D, p(self.dz), p(self.w), p(dx), p(m), ws, nb, ops._stream()),
                                          [dx]))(new()))

    def bwd_filter(self, lib, db, below_floor=True):
        ops, d, p = self.ops, self.d, self.ops._ptr
        new = lambda: (self.out(d.r, d.s, d.c, d.k), self.out(d.k) if db else None)

        def ref():
            dw, b = new()
            ops.conv2d_bwd_filter(d, self.x, self.dz, dw, b)
            return [dw] + ([b] if db else [])

        def direct(ws, nb):
            dw, b = new()
            rc = lib.a3d_conv2d_bwd_filter(self.D, p(self.x), p(self.dz), p(dw), p(b), ws, nb, ops._stream())
            return rc, [dw] + ([b] if db else [])
        exact(lib, lib.a3d_conv2d_bwd_filter_ws_bytes(self.D), below_floor, ref, direct)

    def bwd_filter_pooled(self, lib, dtype):
        """the gradient of the POOLED map, pixel stride a multiple of 4"""
        ops, d, p = self.ops, self.d, self.ops._ptr
        ph, pw, ld = d.ho // 2, d.wo // 2, (d.k + 3) // 4 * 4
        g = torch.Generator(device='cuda').manual_seed(d.k)
        pooled = torch.randn((d.n, ph, pw, ld), device='cuda', generator=g).to(dtype)
        dpool = torch.randn((d.n, ph, pw, ld), device='cuda', generator=g).to(dtype)
        arg = torch.randint(0, 4, (d.n, ph, pw, d.k), device='cuda', generator=g).to(torch.uint8)
        new = lambda: (self.out(d.r, d.s, d.c, d.k), self.out(d.k))

        def ref():
            dw, b = new()
            ops.conv2d_bwd_filter_pooled(d, self.x, dpool, pooled, arg, dw, b)
            return [dw, b]

        def direct(ws, nb):
            dw, b = new()
            rc = lib.a3d_conv2d_bwd_filter_pooled(self.D, p(self.x), p(dpool), ld, p(pooled), p(arg), d.k, int(dtype == BF), p(dw),
                                                  p(b), ws, nb, ops._stream())
            return rc, [dw, b]
        exact(lib, lib.a3d_conv2d_bwd_filter_pooled_ws_bytes(self.D), True, ref, direct)

    def bwd_both(self, lib):
        ops, d, p = self.ops, self.d, self.ops._ptr
        new = lambda: (self.out(d.r, d.s, d.c, d.k), self.out(d.k), self.out(d.n, d.h, d.w, d.c))

        def ref():
            dw, b, dx = new()
            ops.conv2d_bwd_both(d, self.x, self.dz, self.w, dw, b, dx)
            return [dw, b, dx]

        def direct(ws, nb):
            dw, b, dx = new()
            state = torch.zeros(64, dtype=torch.int32, device='cuda')
            rc = lib.a3d_conv2d_bwd_both(self.D, p(self.x), p(self.dz), p(self.w), p(dw), p(b), p(dx), d.c, 0, 1, p(state), ws, nb,
                                         ops._stream())
            return rc, [dw, b, dx]
        exact(lib, lib.a3d_conv2d_bwd_both_ws_bytes(self.D), True, ref, direct)


# (n, h, w, c, k, r = s, stride, padding)
SMALL3 = (2, 20, 24, 3, 40, 5, 2, 'VALID')
CONV0 = (1, 31, 36, 3, 64, 11, 4, 'VALID')          # conv2d_0's geometry
FINE1 = (1, 40, 44, 3, 63, 9, 2, 'VALID')           # fine/first's geometry
FINE1_IMAGE = (1, 40, 44, 4, 63, 9, 2, 'VALID')     # ... on the 4-channel bf16 image
GENERIC = (2, 13, 18, 64, 64, 3, 2, 'VALID')


@pytest.mark.parametrize('case,precision', [(SMALL3, 'fp32'), (CONV0, 'fp32'), (CONV0, 'bf16'), (FINE1, 'fp32'), (FINE1, 'bf16')])
def test_three_channel_layers(ops, lib, case, precision):
    """conv3 forward and pooled forward, fewch / fewch16 and the window-run form's filter gradient, strided bwd-data"""
    c = Conv(ops, *case, precision=precision, ldy=(case[4] + 3) // 4 * 4)
    c.fwd(lib)
    if precision == 'fp32':
        c.pool_fwd(lib, argmax=False)
        c.pool_fwd(lib, argmax=True)
    c.bwd_data(lib, mask=False)
    c.bwd_data(lib, mask=True)
    c.bwd_filter(lib, db=True)
    c.bwd_filter(lib, db=False)


@pytest.mark.parametrize('case,precision,dtype', [(CONV0, 'fp32', torch.float32), (FINE1, 'fp32', torch.float32), (FINE1, 'fp32', BF),
                                                  (FINE1, 'bf16', BF)])
def test_filter_gradient_from_the_pooled_map(ops, lib, case, precision, dtype):
    """a3d_conv2d_bwd_filter_pooled: fewch on float32 or bf16 pooled tensors, fewch16 (bf16 arithmetic, bf16 pooled tensors)"""
    Conv(ops, *case, precision=precision).bwd_filter_pooled(lib, dtype)


@pytest.mark.parametrize('storage', [X, X | Y])
def test_bf16_image_form(ops, lib, storage):
    """the 4-channel bf16 image (conv3b, or the bf16 kernel's window-run form), plain and with the pool fused"""
    c = Conv(ops, *FINE1_IMAGE, precision='bf16', storage=storage, ldy=64)
    c.fwd(lib)
    c.pool_fwd(lib, argmax=False)
    c.pool_fwd(lib, argmax=True)


def test_generic_split_k_and_strided_bwd_data(ops, lib):
    """split-K slabs of the generic kernel; bwd-data as one launch per parity class (too few tiles for the one launch of all)"""
    c = Conv(ops, *GENERIC)
    c.fwd(lib)
    c.bwd_data(lib, mask=False)
    c.bwd_data(lib, mask=True)


def test_lds_dma_kernel(ops, lib):
    """bf16 x, w and y: all three directions, the filter gradient with its bias gradient"""
    c = Conv(ops, *GENERIC, precision='bf16', storage=X | W | Y)
    c.fwd(lib)
    c.bwd_data(lib, mask=True, below_floor=False)
    c.bwd_filter(lib, db=True, below_floor=False)


def test_odd_channel_counts(ops, lib):
    Conv(ops, 1, 17, 16, 32, 40, 3, 2, 'SAME').fwd(lib)
    Conv(ops, 2, 9, 11, 5, 7, 3, 1, 'SAME').bwd_filter(lib, db=True)


def test_single_output_channel_stencil(ops, lib):
    c = Conv(ops, 2, 12, 12, 64, 1, 5, 1, 'SAME')
    c.bwd_filter(lib, db=True, below_floor=False)      # (one slab per block: above the floor at any size)
    c.bwd_both(lib)


def dense(ops, m, k, n):
    g = torch.Generator(device='cuda').manual_seed(m + k + n)
    r = lambda *s: torch.randn(s, device='cuda', generator=g)
    return r(m, k), r(k, n) * 0.05, r(n), r(m, n), ops._ptr, lambda *s: torch.full(s, -3.0, device='cuda')


@pytest.mark.parametrize('m,k,n', [(2, 4096, 4070), (2, 12544, 128)])
def test_dense_fwd(ops, lib, m, k, n):
    """the weight-streaming kernel's partial sums (4096 x 4070), split-K slabs of the GEMM (12544 x 128)"""
    x, w, b, _, p, out = dense(ops, m, k, n)
    exact(lib, lib.a3d_dense_fwd_ws_bytes(m, k, n), True, lambda: [ops.dense_fwd(x, w, b, out(m, n), 'relu')],
          lambda ws, nb: (lambda y: (lib.a3d_dense_fwd(m, k, n, p(x), p(w), p(b), p(y), ops.ACT['relu'], None, ws, nb, ops._stream()),
                                     [y]))(out(m, n)))


def test_dense_bwd_data(ops, lib):
    m, k, n = 2, 4096, 4070
    x, w, _, dz, p, out = dense(ops, m, k, n)
    exact(lib, lib.a3d_dense_bwd_data_ws_bytes(m, k, n), True, lambda: [ops.dense_bwd_data(dz, w, out(m, k), x, 2.0)],
          lambda ws, nb: (lambda dx: (lib.a3d_dense_bwd_data(m, k, n, p(dz), p(w), p(dx), p(x), ops.ACT['relu'], 2.0, ws, nb,
                                                             ops._stream()), [dx]))(out(m, k)))


@pytest.mark.parametrize('m,k,n', [(768, 100, 36), (768, 16, 1)])
def test_dense_bwd_filter(ops, lib, m, k, n):
    x, _, _, dz, p, out = dense(ops, m, k, n)
    exact(lib, lib.a3d_dense_bwd_filter_ws_bytes(m, k, n), True, lambda: list(ops.dense_bwd_filter(x, dz, out(k, n), out(n))),
          lambda ws, nb: (lambda dw, db: (lib.a3d_dense_bwd_filter(m, k, n, p(x), p(dz), p(dw), p(db), ws, nb, ops._stream()),
                                          [dw, db]))(out(k, n), out(n)))
