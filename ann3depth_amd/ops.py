"""Operator layer: the TF ops ann3depth's model functions instantiate, as calls into liba3d.so on torch tensors.

PyTorch only owns memory and streams here.  Every function enqueues HIP kernels on the current stream through the
C ABI (include/a3d.h) and returns without synchronising.  Layouts are TensorFlow's (NHWC / HWIO / [in,out]).
"""
import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import ConvDesc, check

ACT = {None: 0, 'relu': 1, 'sigmoid': 2}
PREC = {'fp32': 0, 'f32': 0, 'bf16x3': 1, 'bf16': 2, 'fp32w': 3}      # 'fp32w': A3D_PREC_F32_WINOGRAD


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Workspace:
    """Scratch for split-K slabs and partial reductions.  One per stream; grows on demand (never inside a graph
    capture: call reserve() with the largest need first)."""

    def __init__(self):
        self.buf = None

    def reserve(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'workspace of {nbytes} bytes must be reserved before graph capture')
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return self.buf

    def get(self, nbytes, device):
        buf = self.reserve(nbytes, device)
        return ctypes.c_void_p(buf.data_ptr()), buf.numel()


_WS = {}


def _ws():
    """The workspace of the current stream (kernels of different streams may run concurrently)."""
    key = torch.cuda.current_stream().cuda_stream
    w = _WS.get(key)
    if w is None:
        w = _WS[key] = Workspace()
    return w


def drop_workspace(stream_handle):
    """Forget the workspace of a stream that is being destroyed (its split-K scratch goes back to the allocator, and a
    later stream that happens to get the same handle value starts with a workspace of its own)."""
    _WS.pop(stream_handle, None)


def same_pad(in_size, k, stride):
    out = -(-in_size // stride)
    pad = max((out - 1) * stride + k - in_size, 0)
    return out, pad // 2


STORE_X, STORE_W, STORE_Y = 1, 2, 4      # a3d_conv_desc.storage bits: which tensors are bf16 in memory


HINT_SHARE_CU = 1                    # a3d_conv_desc.hints
HINT_W_PREPARED = 2


class PreparedFilter:
    """The filter of a few-channel forward in the layout its kernel reads (a3d_conv2d_fwd_prepare_filter), kept beside the
    stored filter so that the repack runs when the weights change instead of on every call.  desc: the descriptor the forward
    uses WITHOUT the hint; .desc_prepared is the same descriptor with A3D_HINT_W_PREPARED, .buf the prepared copy.
    which='bwd_d': the filter a3d_conv2d_bwd_data reads (precision 'fp32w': the transform of the flipped taps); 'bwd_d_wino1d':
    the one conv2d_bwd_data_wino1d reads (include/a3d_wino1d.h)."""

    def __init__(self, desc, device, which='fwd'):
        lib = _lib.load()
        self.stem = {'fwd': 'a3d_conv2d_fwd', 'bwd_d': 'a3dw_conv2d_bwd_data', 'bwd_d_wino1d': 'a3dl_conv2d_bwd_data'}[which]
        nbytes = getattr(lib, self.stem + '_prepared_filter_bytes')(ctypes.byref(desc))
        self.ok = nbytes > 0
        self.desc = desc
        if self.ok:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.desc_prepared = ConvDesc.from_buffer_copy(desc)
            self.desc_prepared.hints = desc.hints | HINT_W_PREPARED

    def refresh(self, w):
        name = self.stem + '_prepare_filter'
        check(getattr(_lib.load(), name)(ctypes.byref(self.desc), _ptr(w), _ptr(self.buf), self.buf.numel(), _stream()), name)


def conv_desc(n, h, w, c, k, r, s, stride, padding, ldx=None, ldy=None, precision='fp32', storage=0, hints=0):
    """Descriptor of tf.layers.conv2d(x[n,h,w,c], k, (r,s), (stride,stride), padding).  precision selects the
    arithmetic of the contraction: 'fp32' (exact, default), 'bf16x3' (split operands), 'bf16', or 'fp32w' (fp32 through
    Winograd F(2x2,3x3) where the layer is a stride-1 3x3 one, 'fp32' elsewhere)."""
    padding = padding.upper()
    if padding == 'SAME':
        ho, pt = same_pad(h, r, stride)
        wo, pl = same_pad(w, s, stride)
    elif padding == 'VALID':
        ho, pt = (h - r) // stride + 1, 0
        wo, pl = (w - s) // stride + 1, 0
    else:
        raise ValueError(padding)
    return ConvDesc(n=n, h=h, w=w, c=c, k=k, r=r, s=s, stride=stride, pad_t=pt, pad_l=pl, ho=ho, wo=wo,
                    ldx=ldx or c, ldy=ldy or k, precision=PREC[precision], storage=storage, hints=hints)


def second_output(t, cols=None, step=1, offset=0, ld=None):
    """a3d_second_output for tensor t: element (row, col < cols) of the launch's output also goes to
    t.flat[(row * ld + col) * step + offset], in t's type (float32 or bfloat16).  Default: t as a [rows, ld] matrix."""
    if t is None:
        return None
    ld = t.shape[-1] if ld is None else ld
    o = _lib.SecondOutput(t.data_ptr(), ld, step, offset, int(t.dtype == torch.bfloat16), ld if cols is None else cols)
    o._keep = t
    return o


def _o2(out2):
    return None if out2 is None else ctypes.byref(out2)


def conv2d_fwd(d, x, w, bias, y, act=None, out2=None):
    lib = _lib.load()
    ws, n = _ws().get(lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(d)), x.device)
    if out2 is not None:
        check(lib.a3d_conv2d_fwd_ex2(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), ACT[act], _o2(out2), ws, n, _stream()),
              'a3d_conv2d_fwd_ex2')
        return y
    check(lib.a3d_conv2d_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), ACT[act], ws, n, _stream()),
          'a3d_conv2d_fwd')
    return y


def conv2d_pool_fwd(d, x, w, bias, y_pooled, act='relu', argmax=None):
    """maxpool2x2(act(conv2d(x) + bias)) in one kernel; y_pooled [n, ho//2, wo//2, >= k] (last dim = pixel stride).
    argmax: optional uint8 [n, ho//2, wo//2, k], receives the window position of each maximum (for maxpool2x2_bwd_idx)."""
    lib = _lib.load()
    ws, n = _ws().get(lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(d)), x.device)
    check(lib.a3d_conv2d_pool_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(y_pooled), y_pooled.shape[-1],
                                  _ptr(argmax), ACT[act], ws, n, _stream()), 'a3d_conv2d_pool_fwd')
    return y_pooled


def maxpool2x2_bwd_idx(argmax, y_pooled, dy, dx, relu_mask=True):
    """MaxPoolGrad (+ ReluGrad) from the argmax positions and pooled values of conv2d_pool_fwd; dx [n,h,w,c] dense,
    y_pooled / dy: last dim = pixel stride (>= c)."""
    n, h, w, c = dx.shape
    if y_pooled.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16:      # bf16 storage throughout (conv2d_1 of config 5)
        assert dy.dtype == torch.bfloat16
        name = 'a3d_maxpool2x2_bwd_idx_bf16s'
    elif y_pooled.dtype == torch.bfloat16:       # bf16 storage: pooled values and dy bf16, dx float32
        assert dy.dtype == torch.bfloat16 and dx.dtype == torch.float32
        name = 'a3d_maxpool2x2_bwd_idx_bf16'
    else:
        name = 'a3d_maxpool2x2_bwd_idx'
    check(getattr(_lib.load(), name)(n, h, w, c, _ptr(argmax), _ptr(y_pooled), y_pooled.shape[-1], _ptr(dy), dy.shape[-1],
                                     _ptr(dx), int(relu_mask), _stream()), name)
    return dx


def copy_channel(src, c_src, dst, c_dst):
    """dst[..., c_dst] = src[..., c_src] (same pixel count; last dims are the pixel strides)."""
    npix = src.numel() // src.shape[-1]
    assert dst.numel() // dst.shape[-1] == npix
    fn = _lib.load().a3d_copy_channel_bf16 if dst.dtype == torch.bfloat16 else _lib.load().a3d_copy_channel
    check(fn(npix, _ptr(src), src.shape[-1], c_src, _ptr(dst), dst.shape[-1], c_dst, _stream()), 'a3d_copy_channel')
    return dst


def conv2d_bwd_data(d, dz, w, dx, relu_mask=None):
    lib = _lib.load()
    ws, n = _ws().get(lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(d)), dz.device)
    check(lib.a3d_conv2d_bwd_data(ctypes.byref(d), _ptr(dz), _ptr(w), _ptr(dx), _ptr(relu_mask), ws, n, _stream()),
          'a3d_conv2d_bwd_data')
    return dx


def conv2d_bwd_filter(d, x, dz, dw, db=None):
    lib = _lib.load()
    ws, n = _ws().get(lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)), x.device)
    check(lib.a3d_conv2d_bwd_filter(ctypes.byref(d), _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), ws, n, _stream()),
          'a3d_conv2d_bwd_filter')
    return dw, db


def conv2d_bwd_filter_wino(d, x, dz, dw, db=None):
    """The filter and bias gradient through Winograd F(2x2,3x3) in fp32 (include/a3d_wino_grad.h) where d is a stride-1 3x3
    layer of float32 tensors; for any other descriptor the library runs conv2d_bwd_filter's kernels."""
    lib = _lib.load()
    ws, n = _ws().get(lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)), x.device)
    check(lib.a3dwg_conv2d_bwd_filter(ctypes.byref(d), _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), ws, n, _stream()),
          'a3dwg_conv2d_bwd_filter')
    return dw, db


def conv2d_bwd_data_wino1d(d, dz, w, dx, relu_mask=None):
    """The input gradient through 1-D Winograd F(4,5) along the width in fp32 (include/a3d_wino1d.h) where d is a stride-1 layer
    of float32 tensors with a window 5 wide; for any other descriptor the library runs conv2d_bwd_data's kernels.  w: the filter,
    or its prepared transform (PreparedFilter(..., 'bwd_d_wino1d')) when d.hints says so."""
    lib = _lib.load()
    ws, n = _ws().get(lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d)), dz.device)
    check(lib.a3dl_conv2d_bwd_data(ctypes.byref(d), _ptr(dz), _ptr(w), _ptr(dx), _ptr(relu_mask), ws, n, _stream()),
          'a3dl_conv2d_bwd_data')
    return dx


def conv2d_bwd_filter_wino1d(d, x, dz, dw, db=None):
    """The filter and bias gradient through the same identity; descriptors as conv2d_bwd_data_wino1d's."""
    lib = _lib.load()
    ws, n = _ws().get(lib.a3dl_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)), x.device)
    check(lib.a3dl_conv2d_bwd_filter(ctypes.byref(d), _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), ws, n, _stream()),
          'a3dl_conv2d_bwd_filter')
    return dw, db


def conv2d_bwd_wino(d, x, dz, w, dw, db, dx, relu_mask=None, pool=None):
    """Filter, bias and input gradient of a stride-1 3x3 layer of float32 tensors through Winograd F(2x2,3x3) as one chain of
    three launches (include/a3d_wino_bwd.h): the bits of conv2d_bwd_filter_wino followed by conv2d_bwd_data under 'fp32w'.
    w: the filter, or its prepared bwd-data transform when d.hints says so.  pool = (argmax, y_pooled): dx is then the UNPOOLED
    gradient [n, h2, w2, c], what maxpool2x2_bwd_idx(relu_mask=True) writes from the layer's own dx.  For any other descriptor the
    library runs the two calls."""
    lib = _lib.load()
    prepared = int(bool(d.hints & HINT_W_PREPARED))
    ws, n = _ws().get(lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(d), prepared, int(pool is not None)), x.device)
    pp = None
    if pool is not None:
        argmax, y = pool
        pp = ctypes.byref(_lib.WinoBwdPool(_ptr(argmax), _ptr(y), y.shape[-1], dx.shape[1], dx.shape[2]))
    check(lib.a3dwb_conv2d_bwd(ctypes.byref(d), _ptr(x), _ptr(dz), _ptr(w), _ptr(dw), _ptr(db), _ptr(dx), _ptr(relu_mask), pp,
                               ws, n, _stream()), 'a3dwb_conv2d_bwd')
    return dw, db, dx


def conv2d_bwd_filter_pooled_supported(d):
    return _lib.load().a3d_conv2d_bwd_filter_pooled_ws_bytes(ctypes.byref(d)) > 0


def conv2d_bwd_filter_pooled(d, x, dpool, pooled, argmax, dw, db=None):
    """Filter and bias gradient of a conv -> ReLU -> 2x2 max pool block from the gradient of the POOLED map: MaxPoolGrad (by the
    recorded window positions) and ReluGrad (pooled > 0; pooled=None: none) happen while the kernel stages its operand."""
    lib = _lib.load()
    ws, n = _ws().get(lib.a3d_conv2d_bwd_filter_pooled_ws_bytes(ctypes.byref(d)), x.device)
    assert pooled is None or (pooled.dtype == dpool.dtype and pooled.shape[-1] == dpool.shape[-1])
    check(lib.a3d_conv2d_bwd_filter_pooled(ctypes.byref(d), _ptr(x), _ptr(dpool), dpool.shape[-1], _ptr(pooled), _ptr(argmax),
                                           argmax.shape[-1], int(dpool.dtype == torch.bfloat16), _ptr(dw), _ptr(db), ws, n,
                                           _stream()), 'a3d_conv2d_bwd_filter_pooled')
    return dw, db


_BOTH_STATE = {}


def conv2d_bwd_both_supported(d):
    return bool(_lib.load().a3d_conv2d_bwd_both_supported(ctypes.byref(d)))


def conv2d_bwd_both(d, x, dz, w, dw, db, dx, relu_mask=True):
    """Filter gradient, bias gradient and input gradient (times x > 0 if relu_mask) of a single-output-channel conv in one
    pass over x (a3d_conv2d_bwd_both); dx may be a bfloat16 tensor.  The launch's arrival counters live in a small zeroed
    buffer per stream (every call leaves it zero)."""
    lib = _lib.load()
    key = (torch.cuda.current_stream().cuda_stream, x.device)
    state = _BOTH_STATE.get(key)
    if state is None:
        state = _BOTH_STATE[key] = torch.zeros(64, dtype=torch.int32, device=x.device)
    ws, n = _ws().get(lib.a3d_conv2d_bwd_both_ws_bytes(ctypes.byref(d)), x.device)
    check(lib.a3d_conv2d_bwd_both(ctypes.byref(d), _ptr(x), _ptr(dz), _ptr(w), _ptr(dw), _ptr(db), _ptr(dx), dx.shape[-1],
                                  int(dx.dtype == torch.bfloat16), int(bool(relu_mask)), _ptr(state), ws, n, _stream()),
          'a3d_conv2d_bwd_both')
    return dw, db, dx


def dense_fwd(x, w, bias, y, act=None, drop_keep=None):
    m, k = x.shape
    n = w.shape[1]
    lib = _lib.load()
    ws, nb = _ws().get(lib.a3d_dense_fwd_ws_bytes(m, k, n), x.device)
    check(lib.a3d_dense_fwd(m, k, n, _ptr(x), _ptr(w), _ptr(bias), _ptr(y), ACT[act], _ptr(drop_keep), ws, nb,
                            _stream()), 'a3d_dense_fwd')
    return y


def dense_bwd_data(dz, w, dx, mask=None, scale=1.0, mask_act='relu'):
    """dx = dz @ w^T, optionally times the activation gradient of the layer below given its output `mask`."""
    m, n = dz.shape
    k = w.shape[0]
    lib = _lib.load()
    ws, nb = _ws().get(lib.a3d_dense_bwd_data_ws_bytes(m, k, n), dz.device)
    check(lib.a3d_dense_bwd_data(m, k, n, _ptr(dz), _ptr(w), _ptr(dx), _ptr(mask), ACT[mask_act], scale, ws, nb,
                                 _stream()),
          'a3d_dense_bwd_data')
    return dx


def dense_bwd_filter(x, dz, dw, db=None):
    m, k = x.shape
    n = dz.shape[1]
    lib = _lib.load()
    ws, nb = _ws().get(lib.a3d_dense_bwd_filter_ws_bytes(m, k, n), x.device)
    check(lib.a3d_dense_bwd_filter(m, k, n, _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), ws, nb, _stream()),
          'a3d_dense_bwd_filter')
    return dw, db


def maxpool2x2_fwd(x, y, extra=None):
    """y[..., :c] = max_pool(x); if extra is given, y[..., c] = extra (fused concat).  y's last dim is its pixel
    stride."""
    n, h, w, c = x.shape
    check(_lib.load().a3d_maxpool2x2_fwd(n, h, w, c, _ptr(x), _ptr(y), y.shape[-1], _ptr(extra), _stream()),
          'a3d_maxpool2x2_fwd')
    return y


def maxpool2x2_bwd(x, dy, dx, relu_mask=True):
    """dy's last dim is its pixel stride (>= c): only its first c channels are read."""
    n, h, w, c = x.shape
    check(_lib.load().a3d_maxpool2x2_bwd(n, h, w, c, _ptr(x), _ptr(dy), dy.shape[-1], _ptr(dx), int(relu_mask),
                                         _stream()), 'a3d_maxpool2x2_bwd')
    return dx


def _pair_args(x0, y0, x1=None, y1=None):
    """(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1): what the _ex, warp and validity-aware entry
    points all begin with.  x1 None: no second tensor, zeros and null pointers."""
    def one(x, y):
        if x is None:
            return 0, None, 0, 0, 0, None
        return x.shape[3], _ptr(x), int(x.dtype == torch.uint8), y.shape[1], y.shape[2], _ptr(y)
    return tuple(x0.shape[:3]) + one(x0, y0) + one(x1, y1)


def resize_bilinear_tf1(x, y):
    """x float32, or uint8 pixel values k of a converter-written record (the kernel reads fl(fl(fl(k/255) - .5) + .5))."""
    n, h, w, c = x.shape
    if x.dtype == torch.uint8:
        check(_lib.load().a3d_resize_bilinear_tf1_ex(*_pair_args(x, y), _stream()), 'a3d_resize_bilinear_tf1_ex')
        return y
    check(_lib.load().a3d_resize_bilinear_tf1(n, h, w, c, _ptr(x), y.shape[1], y.shape[2], _ptr(y), _stream()),
          'a3d_resize_bilinear_tf1')
    return y


def resize_bilinear_tf1_pair(x0, y0, x1, y1):
    """Both resizes of a step in one launch: x0 -> y0 and x1 -> y1, stored tensors of the same batch and size; each
    float32 or uint8 (see resize_bilinear_tf1)."""
    n, h, w, c0 = x0.shape
    assert x1.shape[:3] == (n, h, w)
    if x0.dtype == torch.uint8 or x1.dtype == torch.uint8:
        check(_lib.load().a3d_resize_bilinear_tf1_ex(*_pair_args(x0, y0, x1, y1), _stream()), 'a3d_resize_bilinear_tf1_ex')
        return
    check(_lib.load().a3d_resize_bilinear_tf1_pair(n, h, w, c0, _ptr(x0), y0.shape[1], y0.shape[2], _ptr(y0), x1.shape[3],
                                                   _ptr(x1), y1.shape[1], y1.shape[2], _ptr(y1), _stream()),
          'a3d_resize_bilinear_tf1_pair')


WARP_STRIDE = 12                     # A3D_WARP_STRIDE (include/a3d.h)


def _check_pair(who, x0, y0, x1, y1, table):
    """The argument checks of warp_bilinear_pair and the validity-aware pair launches (table None: a launch without one)."""
    if x0.dim() != 4 or y0.dim() != 4 or y0.shape[0] != x0.shape[0] or y0.shape[3] != x0.shape[3]:
        raise ValueError(f'{who}: {tuple(x0.shape)} -> {tuple(y0.shape)}')
    n, h, w, c0 = x0.shape
    if (x1 is None) != (y1 is None):
        raise ValueError(f'{who}: x1 and y1 go together')
    if x1 is not None and (x1.dim() != 4 or tuple(x1.shape[:3]) != (n, h, w) or y1.dim() != 4
                           or y1.shape[0] != n or y1.shape[3] != x1.shape[3]):
        raise ValueError(f'{who}: second tensor {tuple(x1.shape)} -> {tuple(y1.shape)} beside '
                         f'{tuple(x0.shape)}')
    if table is not None and (tuple(table.shape) != (n, WARP_STRIDE) or table.dtype != torch.float32):
        raise ValueError(f'{who}: table {tuple(table.shape)} {table.dtype}, want [{n}, {WARP_STRIDE}] float32')
    for name, t, dtypes in (('x0', x0, (torch.float32, torch.uint8)), ('y0', y0, (torch.float32,)),
                            ('x1', x1, (torch.float32, torch.uint8)), ('y1', y1, (torch.float32,)),
                            ('table', table, (torch.float32,))):
        if t is None:
            continue
        if t.dtype not in dtypes:
            raise ValueError(f'{who}: {name} is {t.dtype}')
        if not t.is_cuda or t.device != x0.device:
            raise ValueError(f'{who}: {name} is on {t.device}, x0 on {x0.device}')
        if not t.is_contiguous():
            raise ValueError(f'{who}: {name} is not contiguous')
    return n, h, w, c0


def warp_bilinear_pair(x0, y0, x1, y1, table):
    """resize_bilinear_tf1_pair through a per-image affine map and gains (a3d_warp_bilinear_pair): x0 -> y0 and, unless
    x1 is None, x1 -> y1.  x0 / x1 [n, h, w, c] float32 or uint8, y0 / y1 float32, table [n, 12] float32, all contiguous
    tensors of one device."""
    if table is None:
        raise ValueError('warp_bilinear_pair: no table')
    _check_pair('warp_bilinear_pair', x0, y0, x1, y1, table)
    check(_lib.load().a3d_warp_bilinear_pair(*_pair_args(x0, y0, x1, y1), _ptr(table), _stream()), 'a3d_warp_bilinear_pair')


def _valid_range(who, x1, min_depth, max_depth):
    if x1 is None:
        raise ValueError(f'{who}: the depth map x1 is required')
    lo, hi = float(min_depth), float(max_depth)
    if not lo <= hi:
        raise ValueError(f'{who}: min_depth {lo}, max_depth {hi}')
    return lo, hi


def resize_bilinear_tf1_pair_valid(x0, y0, x1, y1, min_depth=0., max_depth=float('inf')):
    """NON-REFERENCE: resize_bilinear_tf1_pair for a depth map x1 with holes (a3dx_resize_bilinear_tf1_valid): an element of
    y1 whose counting taps are not all finite and in (min_depth, max_depth] is NaN, every other bit of y0 and y1 is the
    plain launch's.  Tensors as warp_bilinear_pair's."""
    who = 'resize_bilinear_tf1_pair_valid'
    lo, hi = _valid_range(who, x1, min_depth, max_depth)
    _check_pair(who, x0, y0, x1, y1, None)
    check(_lib.load().a3dx_resize_bilinear_tf1_valid(*_pair_args(x0, y0, x1, y1), lo, hi, _stream()),
          'a3dx_resize_bilinear_tf1_valid')


def resize_bilinear_tf1_valid(x, y, min_depth=0., max_depth=float('inf'), scratch=None):
    """NON-REFERENCE: the depth map x alone (stored at another size than its image).  The entry point's tensor 0 is then x
    itself, resized to one pixel per image into `scratch` ([n, 1, 1, c] float32, allocated here when None)."""
    if scratch is None:
        scratch = torch.empty((x.shape[0], 1, 1, x.shape[3]), device=x.device)
    resize_bilinear_tf1_pair_valid(x, scratch, x, y, min_depth, max_depth)
    return y


def warp_bilinear_pair_valid(x0, y0, x1, y1, table, min_depth=0., max_depth=float('inf')):
    """NON-REFERENCE: warp_bilinear_pair for a depth map x1 with holes (a3dx_warp_bilinear_pair_valid); the thresholds are
    compared with the stored depth, before the table's depth gain."""
    who = 'warp_bilinear_pair_valid'
    if table is None:
        raise ValueError(f'{who}: no table')
    lo, hi = _valid_range(who, x1, min_depth, max_depth)
    _check_pair(who, x0, y0, x1, y1, table)
    check(_lib.load().a3dx_warp_bilinear_pair_valid(*_pair_args(x0, y0, x1, y1), _ptr(table), lo, hi, _stream()),
          'a3dx_warp_bilinear_pair_valid')


def extract_patches(x, k, stride, y):
    n, h, w, c = x.shape
    check(_lib.load().a3d_extract_patches(n, h, w, c, _ptr(x), k, stride, _ptr(y), _stream()), 'a3d_extract_patches')
    return y


SILOG_PARTS = 8                      # A3D_SILOG_PARTS (include/a3d.h)


def _loss_ws_floats(k, b):
    """Floats of a loss workspace: the ticket, k words per sample, k per block (A3D_SILOG_WS_FLOATS and its siblings)."""
    return k * b + 1 + k * b * SILOG_PARTS


def _ssi_ws_floats(b):
    """A3DI_WS_FLOATS(b): the ticket and a pad, four words per sample, ten per block (four of them float64 pairs)."""
    return 4 * b + 2 + 10 * b * SILOG_PARTS


def _ld16(dout16):
    """The pitch argument that goes with an optional bf16 copy of the gradient."""
    return 0 if dout16 is None else dout16.shape[-1]


# What a loss launch set passes between (b, ...) and the buffers, with its checks: ((the sizes after b), (the arguments between tgt
# and the buffers)) from who's out, tgt and the caller's own arguments.
def _plain_args(who, out, tgt):
    return (out.numel() // out.shape[0],), ()


def _grad_loss_args(who, out, tgt, h, w, masked, grad_weight):
    b = out.shape[0]
    assert out.numel() == b * h * w, f'{who}: out holds {out.numel()} values, not {b} x {h} x {w}'
    grad_weight = float(grad_weight)
    if not grad_weight >= 0:
        raise ValueError(f'{who}: grad_weight {grad_weight!r} must be a number >= 0')
    return (h, w), (int(bool(masked)), grad_weight)


def _berhu_args(who, out, tgt, masked, fraction):
    assert out.numel() == tgt.numel(), f'{who}: out holds {out.numel()} values, tgt {tgt.numel()}'
    fraction = float(fraction)
    if not 0 < fraction <= 1:
        raise ValueError(f'{who}: fraction {fraction!r} must lie in (0, 1]')
    return (out.numel() // out.shape[0],), (int(bool(masked)), fraction)


def _ssi_args(who, out, tgt, masked):
    assert out.numel() == tgt.numel(), f'{who}: out holds {out.numel()} values, tgt {tgt.numel()}'
    return (out.numel() // out.shape[0],), (int(bool(masked)),)


# The five loss launch sets, by the name their public functions <name>_ws, <name>_loss_fwd and <name>_loss_bwd carry: the forward
# and backward entry points, the workspace in floats for a batch of b, the floats a forward writes, and the arguments above.
_LossLaunch = collections.namedtuple('_LossLaunch', 'fwd bwd ws_floats writes args')
_LOSSES = {
    'silog': _LossLaunch('a3d_silog_loss_fwd', 'a3d_silog_loss_bwd_ex', lambda b: _loss_ws_floats(2, b), 1, _plain_args),
    'silog_masked': _LossLaunch('a3dx_silog_masked_loss_fwd', 'a3dx_silog_masked_loss_bwd_ex', lambda b: _loss_ws_floats(3, b), 2,
                                _plain_args),
    'silog_grad': _LossLaunch('a3dg_silog_grad_loss_fwd', 'a3dg_silog_grad_loss_bwd_ex', lambda b: _loss_ws_floats(5, b), 4,
                              _grad_loss_args),
    'berhu': _LossLaunch('a3dh_berhu_loss_fwd', 'a3dh_berhu_loss_bwd_ex', lambda b: _loss_ws_floats(3, b), 4, _berhu_args),
    'ssi': _LossLaunch('a3di_ssi_loss_fwd', 'a3di_ssi_loss_bwd_ex', _ssi_ws_floats, 4, _ssi_args),
}


def _loss_ws(name, b, device):
    """The workspace of one launch set for a batch of b (or any smaller one): zeros, since the ticket, its first word, must
    start at zero."""
    return torch.zeros(_LOSSES[name].ws_floats(b), device=device)


def _loss_fwd(name, out, tgt, loss, ws, *more):
    launch = _LOSSES[name]
    b = out.shape[0]
    dims, middle = launch.args(name + '_loss_fwd', out, tgt, *more)
    assert ws.numel() >= launch.ws_floats(b), \
        f'{name.split("_")[0]} workspace too small: allocate it with ops.{name}_ws(b, device)'
    if launch.writes > 1:
        assert loss.numel() >= launch.writes and loss.is_contiguous(), \
            f'{name}_loss_fwd writes {("two", "four")[launch.writes // 4]} floats'
    check(getattr(_lib.load(), launch.fwd)(b, *dims, _ptr(out), _ptr(tgt), *middle, _ptr(loss), _ptr(ws), _stream()), launch.fwd)
    return loss


def _loss_bwd(name, out, tgt, ws, dout, dout16, *more):
    launch = _LOSSES[name]
    dims, middle = launch.args(name + '_loss_bwd', out, tgt, *more)
    check(getattr(_lib.load(), launch.bwd)(out.shape[0], *dims, _ptr(out), _ptr(tgt), *middle, _ptr(ws), _ptr(dout), _ptr(dout16),
                                          _ld16(dout16), _stream()), launch.bwd)
    return dout


def silog_ws(b, device):
    """Workspace of silog_loss_fwd / _bwd: A3D_SILOG_WS_FLOATS(b) zeros (see _loss_ws)."""
    return _loss_ws('silog', b, device)


def silog_loss_fwd(out, tgt, loss, ws):
    return _loss_fwd('silog', out, tgt, loss, ws)


def silog_loss_bwd(out, tgt, ws, dout, dout16=None):
    """dout16: optional bfloat16 [b, ld >= npix], receives the same gradient (columns npix.. stay as they are: keep them zero)."""
    return _loss_bwd('silog', out, tgt, ws, dout, dout16)


def silog_masked_ws(b, device):
    """Workspace of silog_masked_loss_fwd / _bwd: A3DX_SILOG_MASKED_WS_FLOATS(b) zeros (see _loss_ws)."""
    return _loss_ws('silog_masked', b, device)


def silog_masked_loss_fwd(out, tgt, loss, ws):
    """NON-REFERENCE: the loss over the finite targets only (a3dx_silog_masked_loss_fwd).  loss: 2 floats, the loss and the
    fraction of valid target pixels."""
    return _loss_fwd('silog_masked', out, tgt, loss, ws)


def silog_masked_loss_bwd(out, tgt, ws, dout, dout16=None):
    """dout16 as silog_loss_bwd's."""
    return _loss_bwd('silog_masked', out, tgt, ws, dout, dout16)


def silog_grad_ws(b, device):
    """Workspace of silog_grad_loss_fwd / _bwd: A3DG_WS_FLOATS(b) zeros (see _loss_ws)."""
    return _loss_ws('silog_grad', b, device)


def silog_grad_loss_fwd(out, tgt, h, w, masked, grad_weight, loss, ws):
    """NON-REFERENCE: the scale-invariant loss plus grad_weight times the gradient-matching term of Eigen & Fergus 2015 over
    the horizontal and vertical neighbour pairs of the h x w grid (a3dg_silog_grad_loss_fwd).  masked: only finite targets
    count, as in silog_masked_loss_fwd.  loss: 4 floats — the total, the valid fraction, the silog part, the gradient part."""
    return _loss_fwd('silog_grad', out, tgt, loss, ws, h, w, masked, grad_weight)


def silog_grad_loss_bwd(out, tgt, h, w, masked, grad_weight, ws, dout, dout16=None):
    """dout16 as silog_loss_bwd's.  masked and grad_weight as in the forward call that filled ws."""
    return _loss_bwd('silog_grad', out, tgt, ws, dout, dout16, h, w, masked, grad_weight)


def berhu_ws(b, device):
    """Workspace of berhu_loss_fwd / _bwd: A3DH_WS_FLOATS(b) zeros (see _loss_ws)."""
    return _loss_ws('berhu', b, device)


def berhu_loss_fwd(out, tgt, masked, fraction, loss, ws):
    """NON-REFERENCE: the reverse Huber loss of Laina et al. 2016 on linear depth, with the threshold fraction x the largest
    error of each sample (a3dh_berhu_loss_fwd, two launches).  masked: only finite targets count, as in silog_masked_loss_fwd.
    loss: 4 floats — the loss, the valid fraction, the mean threshold, the share of the counting pixels that are quadratic."""
    return _loss_fwd('berhu', out, tgt, loss, ws, masked, fraction)


def berhu_loss_bwd(out, tgt, masked, fraction, ws, dout, dout16=None):
    """dout16 as silog_loss_bwd's.  masked and fraction as in the forward call that filled ws."""
    return _loss_bwd('berhu', out, tgt, ws, dout, dout16, masked, fraction)


def ssi_ws(b, device):
    """Workspace of ssi_loss_fwd / _bwd: A3DI_WS_FLOATS(b) zeros (see _loss_ws).  Word 2 + 4 i + {0, 1, 2, 3} holds sample i's
    scale, shift, count and flag (0 fitted, 1 degenerate, 2 poisoned) after a forward call."""
    return _loss_ws('ssi', b, device)


def ssi_loss_fwd(out, tgt, masked, loss, ws):
    """NON-REFERENCE: the least-squares scale-and-shift-invariant loss of Ranftl et al. 2020 on linear depth: per sample the
    squared error left after the best scale and shift of the output (a3di_ssi_loss_fwd, two launches).  masked: only finite
    targets count, as in silog_masked_loss_fwd.  loss: 4 floats — the loss, the valid fraction, the mean scale, the mean shift."""
    return _loss_fwd('ssi', out, tgt, loss, ws, masked)


def ssi_loss_bwd(out, tgt, masked, ws, dout, dout16=None):
    """dout16 as silog_loss_bwd's.  masked as in the forward call that filled ws."""
    return _loss_bwd('ssi', out, tgt, ws, dout, dout16, masked)


METRIC_COLUMNS = ('n', 'abs_rel', 'sq_rel', 'sq', 'log', 'log_sq', 'log10', 'delta1', 'delta2', 'delta3', 'nonfinite')
# A3D_METRIC_* (include/a3d.h): the per-image sums of a3d_depth_metrics, in this column order


def _depth_pair(what, pred, target):
    """The argument checks depth_metrics and depth_align share: (n, ph, pw, th, tw)."""
    n = pred.shape[0]
    if target.shape[0] != n:
        raise ValueError(f'{what}: {n} predictions, {target.shape[0]} targets')
    if pred.dtype != torch.float32 or target.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f'{what}: pred float32, target float32 or uint8')
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise ValueError(f'{what}: contiguous tensors only')
    ph, pw = pred.shape[1], pred.shape[2]
    th, tw = target.shape[1], target.shape[2]
    if pred[0].numel() != ph * pw or target[0].numel() != th * tw:
        raise ValueError(f'{what}: one channel only')
    return n, ph, pw, th, tw


def _coef_ok(what, coef, n, device):
    if coef.dtype != torch.float32 or not coef.is_contiguous() or tuple(coef.shape) != (n, 2) or coef.device != device:
        raise ValueError(f'{what}: coef is float32 [{n}, 2], contiguous, on the tensors\' device')


def depth_metrics(pred, target, *, min_depth=0., max_depth=float('inf'), clamp_lo=1e-3, clamp_hi=float('inf'), rows=None,
                  coef=None):
    """Per-image error sums of Eigen et al. 2014, section 4: pred [n, ph, pw(, 1)] float32 on the model grid; target
    [n, th, tw(, 1)] float32 or the uint8 pixel values of a converter-written record.  A target of another size than the
    prediction is compared at its own pixels, the prediction sampled there as ResizeBilinear (align_corners=False) would
    resample it.  Returns float64 [n, 11] (`rows`, or a new tensor) with the columns of METRIC_COLUMNS; see
    summarize_depth_metrics for the metrics.  Stream-ordered, no synchronisation.
    coef (NON-REFERENCE, include/a3d_align.h): float32 [n, 2] (s, b) per image, as depth_align returns them; the sampled
    prediction p is judged as fl(fl(s p) + b).  None: the plain a3d_depth_metrics."""
    n, ph, pw, th, tw = _depth_pair('depth_metrics', pred, target)
    if rows is None:
        rows = torch.empty((n, len(METRIC_COLUMNS)), dtype=torch.float64, device=pred.device)
    assert rows.dtype == torch.float64 and rows.is_contiguous() and rows.shape[0] >= n and rows.shape[1] == len(METRIC_COLUMNS)
    lib = _lib.load()
    need = lib.a3d_depth_metrics_ws_bytes(n, th, tw)
    ws, cap = _ws().get(need, pred.device)
    if coef is None:
        check(lib.a3d_depth_metrics(n, ph, pw, _ptr(pred), th, tw, _ptr(target), int(target.dtype == torch.uint8), min_depth,
                                    max_depth, clamp_lo, clamp_hi, _ptr(rows), ws, cap, _stream()), 'a3d_depth_metrics')
        return rows
    _coef_ok('depth_metrics', coef, n, pred.device)
    check(lib.a3da_depth_metrics_aligned(n, ph, pw, _ptr(pred), th, tw, _ptr(target), int(target.dtype == torch.uint8),
                                         min_depth, max_depth, clamp_lo, clamp_hi, _ptr(coef), _ptr(rows), ws, cap, _stream()),
          'a3da_depth_metrics_aligned')
    return rows


ALIGN_MODES = ('median', 'scale', 'affine')      # A3DA_MEDIAN, A3DA_SCALE, A3DA_AFFINE (include/a3d_align.h), in this order


def depth_align(pred, target, mode, *, min_depth=0., max_depth=float('inf')):
    """NON-REFERENCE (include/a3d_align.h).  Per image, the scale and shift that align pred to target over the pixels
    depth_metrics sums over (valid target, finite sampled prediction): mode 'median' (s = med t / med p, lower medians),
    'scale' (least squares, b = 0) or 'affine' (least squares).  pred / target as depth_metrics takes them.  Returns
    (coef float32 [n, 2], count int32 [n], status int32 [n]); an image that cannot be aligned has coef (1, 0) and status 1.
    Stream-ordered, no synchronisation."""
    if mode not in ALIGN_MODES:
        raise ValueError(f'depth_align: mode {mode!r} is none of {ALIGN_MODES}')
    n, ph, pw, th, tw = _depth_pair('depth_align', pred, target)
    coef = torch.empty((n, 2), dtype=torch.float32, device=pred.device)
    count = torch.empty(n, dtype=torch.int32, device=pred.device)
    status = torch.empty(n, dtype=torch.int32, device=pred.device)
    lib = _lib.load()
    m = ALIGN_MODES.index(mode)
    need = lib.a3da_depth_align_ws_bytes(n, th, tw, m)
    ws, cap = _ws().get(need, pred.device)
    check(lib.a3da_depth_align(n, ph, pw, _ptr(pred), th, tw, _ptr(target), int(target.dtype == torch.uint8), min_depth,
                               max_depth, m, _ptr(coef), _ptr(count), _ptr(status), ws, cap, _stream()), 'a3da_depth_align')
    return coef, count, status


def affine_apply(x, coef, out=None):
    """NON-REFERENCE (include/a3d_align.h): out[i] = fl(fl(s_i x[i]) + b_i) for x float32 [n, ...] and coef [n, 2] (s, b) per
    image; out may be x (None: a new tensor).  Stream-ordered."""
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 2 or x[0].numel() == 0:
        raise ValueError('affine_apply: x is float32 [n, ...], contiguous')
    n = x.shape[0]
    _coef_ok('affine_apply', coef, n, x.device)
    if out is None:
        out = torch.empty_like(x)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape != x.shape or out.device != x.device:
        raise ValueError('affine_apply: out has x\'s shape, dtype and device')
    check(_lib.load().a3da_affine_apply(n, x[0].numel(), _ptr(x), _ptr(coef), _ptr(out), _stream()), 'a3da_affine_apply')
    return out


def summarize_depth_metrics(rows):
    """The metrics of Eigen et al. 2014, Table 1, from depth_metrics rows (any number of batches stacked), on the host in
    float64.  With q the clamped prediction, t the target and N the valid pixels of ALL images:
      abs_rel  = sum |q - t| / t / N                sq_rel = sum (q - t)^2 / t / N
      rmse     = sqrt(sum (q - t)^2 / N)            rmse_log = sqrt(sum (ln q - ln t)^2 / N)
      log10    = sum |log10 q - log10 t| / N
      delta_k  = share of pixels with max(q / t, t / q) < 1.25^k, k = 1, 2, 3
      rmse_si  = sqrt(mean over the images with n > 0 of  sum d^2 / n - (sum d / n)^2),  d = ln q - ln t: eq. (1) with
                 lambda = 1, per image, as the paper reports its scale-invariant error
    and pixels = N, images = rows, images_without_valid_pixels, nonfinite = valid pixels whose prediction was not finite
    (left out of every other sum).  A metric over no pixels is NaN."""
    import numpy as np
    r = (rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)).astype(np.float64)
    r = r.reshape(-1, len(METRIC_COLUMNS))
    col = {c: r[:, i] for i, c in enumerate(METRIC_COLUMNS)}
    N = float(col['n'].sum())

    def mean(c):
        return float(col[c].sum()) / N if N > 0 else float('nan')
    have = col['n'] > 0
    nv = col['n'][have]
    per_image = col['log_sq'][have] / nv - np.square(col['log'][have] / nv) if have.any() else np.zeros(0)
    return {
        'abs_rel': mean('abs_rel'), 'sq_rel': mean('sq_rel'), 'rmse': float(np.sqrt(mean('sq'))),
        'rmse_log': float(np.sqrt(mean('log_sq'))), 'log10': mean('log10'),
        'rmse_si': float(np.sqrt(max(per_image.mean(), 0.0))) if per_image.size else float('nan'),
        'delta1': mean('delta1'), 'delta2': mean('delta2'), 'delta3': mean('delta3'),
        'pixels': int(N), 'images': int(r.shape[0]), 'images_without_valid_pixels': int((~have).sum()),
        'nonfinite': int(col['nonfinite'].sum()),
    }


def adam_apply_tf1(var, m, v, g, lr, beta1, beta2, eps, beta1_power, beta2_power, grad_scale=1.0, poisoned=None):
    """poisoned: optional int32[1] device tensor; bit 0 is set when the update turned an element of var or v non-finite."""
    if poisoned is not None:
        check(_lib.load().a3d_adam_apply_tf1_flag(var.numel(), _ptr(var), _ptr(m), _ptr(v), _ptr(g), lr, beta1, beta2, eps,
                                                  beta1_power, beta2_power, grad_scale, _ptr(poisoned), _stream()),
              'a3d_adam_apply_tf1_flag')
        return
    check(_lib.load().a3d_adam_apply_tf1(var.numel(), _ptr(var), _ptr(m), _ptr(v), _ptr(g), lr, beta1, beta2, eps,
                                         beta1_power, beta2_power, grad_scale, _stream()), 'a3d_adam_apply_tf1')


def dense_bwd_filter_adam_tf1(x, dz, var_w, m_w, v_w, var_b, m_b, v_b, lr, beta1, beta2, beta1_power, beta2_power,
                              grad_scale=1.0, precision='fp32'):
    """dense_bwd_filter + ApplyAdam(beta2 = 1) of one dense layer in one pass; the gradient is not materialised.
    precision 'bf16': x and dz rounded to bf16 for the contraction (batches above 32 rows; config 5)."""
    m, k = x.shape
    n = dz.shape[1]
    check(_lib.load().a3d_dense_bwd_filter_adam_tf1_ex(m, k, n, _ptr(x), _ptr(dz), _ptr(var_w), _ptr(m_w), _ptr(v_w),
                                                       _ptr(var_b), _ptr(m_b), _ptr(v_b), lr, beta1, beta2, beta1_power,
                                                       beta2_power, grad_scale, PREC[precision], _stream()),
          'a3d_dense_bwd_filter_adam_tf1_ex')


def with_storage(d, storage):
    """Copy of a conv descriptor with other storage bits (forward / bwd-data / bwd-filter mark different tensors)."""
    e = ConvDesc()
    ctypes.pointer(e)[0] = d
    e.storage = storage
    return e


def _dense_ws(lib, m, k, n, precision, storage, device):
    d = conv_desc(m, 1, 1, k, n, 1, 1, 1, 'VALID', precision=precision, storage=storage)
    need = max(lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(d)), lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(d)))
    return _ws().get(need, device)


def dense_fwd_ex(x, w, bias, y, act=None, drop_keep=None, precision='fp32', storage=0, out2=None, n=None):
    """dense_fwd with the arithmetic / weight storage of BASELINE config 5 (w may be the layer's bf16 copy).  n: the GEMM's
    column count where it is wider than y (w padded to whole 16-byte pieces): y then receives its own y.shape[1] columns at its
    own pitch; out2: a3d_second_output (second_output())."""
    m, k = x.shape
    ncols = y.shape[1]
    n = ncols if n is None else n
    lib = _lib.load()
    ws, nb = _dense_ws(lib, m, k, n, precision, storage, x.device)
    check(lib.a3d_dense_fwd_ex2(m, k, n, _ptr(x), _ptr(w), _ptr(bias), _ptr(y), ncols, ncols, ACT[act], _ptr(drop_keep),
                                PREC[precision], storage, _o2(out2), ws, nb, _stream()), 'a3d_dense_fwd_ex2')
    return y


def dense_bwd_data_ex(dz, w, dx, mask=None, mask_act='relu', scale=1.0, precision='fp32', storage=0, out2=None):
    m, n = dz.shape
    k = dx.shape[1]
    lib = _lib.load()
    ws, nb = _dense_ws(lib, m, k, n, precision, storage, dz.device)
    check(lib.a3d_dense_bwd_data_ex2(m, k, n, _ptr(dz), _ptr(w), _ptr(dx), _ptr(mask), ACT[mask_act], scale, PREC[precision],
                                     storage, _o2(out2), ws, nb, _stream()), 'a3d_dense_bwd_data_ex2')
    return dx


def pad_channels_bf16(src, dst):
    """float32 [..., c] -> bfloat16 [..., 4], missing channels zero."""
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and dst.shape[-1] == 4 and src.shape[:-1] == dst.shape[:-1]
    check(_lib.load().a3d_pad_channels_bf16(src.numel() // src.shape[-1], src.shape[-1], _ptr(src), 4, _ptr(dst), _stream()),
          'a3d_pad_channels_bf16')
    return dst


def cast_rows(src, dst, cols=None):
    """dst[r, :cols] = src[r, :cols] (float32 / bfloat16 on either side), dst[r, cols:] = 0: 2-D tensors whose last
    dimensions are their row pitches."""
    rows = src.shape[0]
    cols = cols if cols is not None else min(src.shape[1], dst.shape[1])
    assert dst.shape[0] == rows and src.dim() == dst.dim() == 2 and src.is_contiguous() and dst.is_contiguous()
    check(_lib.load().a3d_cast_rows(rows, cols, _ptr(src), src.shape[1], int(src.dtype == torch.bfloat16), _ptr(dst),
                                    dst.shape[1], int(dst.dtype == torch.bfloat16), _stream()), 'a3d_cast_rows')
    return dst


def cast_bf16(src, dst):
    """float32 -> bfloat16 or back, by dst's dtype (round to nearest even)."""
    assert src.numel() == dst.numel() and {src.dtype, dst.dtype} == {torch.float32, torch.bfloat16}
    check(_lib.load().a3d_cast_bf16(src.numel(), _ptr(src), _ptr(dst), int(dst.dtype == torch.bfloat16), _stream()),
          'a3d_cast_bf16')
    return dst


def maxpool2x2_fwd_bf16(x, y, extra=None, c=None):
    """bf16 tensors; x's and y's last dims are their pixel strides, c (default: x's) the channels pooled."""
    n, h, w, ldx = x.shape
    check(_lib.load().a3d_maxpool2x2_fwd_bf16(n, h, w, c or ldx, _ptr(x), ldx, _ptr(y), y.shape[-1], _ptr(extra), _stream()),
          'a3d_maxpool2x2_fwd_bf16')
    return y


def maxpool2x2_bwd_bf16(x, dy, dx, relu_mask=True, c=None):
    n, h, w, ldx = x.shape
    assert dx.shape == x.shape
    check(_lib.load().a3d_maxpool2x2_bwd_bf16(n, h, w, c or ldx, _ptr(x), ldx, _ptr(dy), dy.shape[-1], _ptr(dx),
                                              int(relu_mask), _stream()), 'a3d_maxpool2x2_bwd_bf16')
    return dx


def sgd_apply(var, g, lr):
    """tf.train.GradientDescentOptimizer (src/models.py:198)."""
    check(_lib.load().a3d_sgd_apply(var.numel(), _ptr(var), _ptr(g), lr, _stream()), 'a3d_sgd_apply')


def sgd_apply_floor(var, g, lr, floor=0.0):
    """NON-REFERENCE (a3dp_sgd_apply_floor): sgd_apply's step, then no element below `floor`; a NaN stays a NaN.  var, g:
    float32 tensors of one size."""
    if var.numel() == 0 or g.numel() != var.numel():
        raise ValueError(f'sgd_apply_floor: var {tuple(var.shape)} and g {tuple(g.shape)} must hold the same number of values')
    if var.dtype != torch.float32 or g.dtype != torch.float32:
        raise TypeError('sgd_apply_floor: var, g float32')
    if not (var.is_contiguous() and g.is_contiguous()):
        raise ValueError('sgd_apply_floor: contiguous tensors only')
    if g.device != var.device:
        raise ValueError('sgd_apply_floor: all tensors on one device')
    check(_lib.load().a3dp_sgd_apply_floor(var.numel(), _ptr(var), _ptr(g), lr, floor, _stream()), 'a3dp_sgd_apply_floor')


def _check_momentum(who, f32, names):
    """TypeError unless every tensor is float32; ValueError unless all are contiguous and on one device."""
    if any(t.dtype != torch.float32 for t in f32):
        raise TypeError(f'{who}: {names} float32')
    if not all(t.is_contiguous() for t in f32):
        raise ValueError(f'{who}: contiguous tensors only')
    if any(t.device != f32[0].device for t in f32):
        raise ValueError(f'{who}: all tensors on one device')


def momentum_apply(var, accum, g, lr, momentum, grad_scale=1.0):
    """NON-REFERENCE (a3do_momentum_apply): TF 1.3's MomentumOptimizer step without Nesterov, every operation rounded to float32
    on its own: g' = g * grad_scale (skipped at 1), accum = accum * momentum + g', var = var - lr * accum.  var, accum, g:
    float32 tensors of one size, starting on 16-byte boundaries."""
    if var.numel() == 0 or accum.numel() != var.numel() or g.numel() != var.numel():
        raise ValueError(f'momentum_apply: var {tuple(var.shape)}, accum {tuple(accum.shape)} and g {tuple(g.shape)} must hold '
                         f'the same number of values')
    _check_momentum('momentum_apply', (var, accum, g), 'var, accum, g')
    check(_lib.load().a3do_momentum_apply(var.numel(), _ptr(var), _ptr(accum), _ptr(g), lr, momentum, grad_scale, _stream()),
          'a3do_momentum_apply')


def dense_bwd_filter_momentum(x, dz, var_w, accum_w, var_b, accum_b, lr, momentum, grad_scale=1.0):
    """NON-REFERENCE (a3do_dense_bwd_filter_momentum): dense_bwd_filter + momentum_apply of one dense layer's kernel and bias in
    one launch, bit for bit the two calls; the gradient is not materialised.  x [m, k], dz [m, n] with m <= 64, var_w and
    accum_w [k, n]; var_b and accum_b [n], or both None."""
    if x.dim() != 2 or dz.dim() != 2 or x.shape[0] != dz.shape[0]:
        raise ValueError(f'dense_bwd_filter_momentum: x {tuple(x.shape)} and dz {tuple(dz.shape)} are [m, k] and [m, n]')
    m, k = x.shape
    n = dz.shape[1]
    if tuple(var_w.shape) != (k, n) or tuple(accum_w.shape) != (k, n):
        raise ValueError(f'dense_bwd_filter_momentum: var_w {tuple(var_w.shape)} and accum_w {tuple(accum_w.shape)} must be '
                         f'[{k}, {n}]')
    if (var_b is None) != (accum_b is None):
        raise ValueError('dense_bwd_filter_momentum: var_b and accum_b come as a pair or not at all')
    bias = () if var_b is None else (var_b, accum_b)
    if any(t.numel() != n for t in bias):
        raise ValueError(f'dense_bwd_filter_momentum: var_b and accum_b must hold {n} values')
    _check_momentum('dense_bwd_filter_momentum', (x, dz, var_w, accum_w) + bias, 'x, dz, var_w, accum_w, var_b, accum_b')
    check(_lib.load().a3do_dense_bwd_filter_momentum(m, k, n, _ptr(x), _ptr(dz), _ptr(var_w), _ptr(accum_w), _ptr(var_b),
                                                     _ptr(accum_b), lr, momentum, grad_scale, _stream()),
          'a3do_dense_bwd_filter_momentum')


# ---- gradient clipping by global norm, per optimizer group (NON-REFERENCE, include/a3d_clip.h) ----
ClipState = collections.namedtuple('ClipState', 'sumsq norm scale skip skipped')


def clip_ctl(device):
    """A control block of grad_norm_scale and the *_ctl applies: 32 zeroed bytes, as four int64 words."""
    return torch.zeros(_lib.CLIP_CTL_BYTES // 8, dtype=torch.int64, device=device)


def clip_read(ctl):
    """The control block on the host, one copy: ClipState(sumsq float64, norm float32, scale float32, skip, skipped)."""
    import numpy as np
    raw = ctl.cpu().numpy().tobytes()
    f = np.frombuffer(raw, np.float32)
    u = np.frombuffer(raw, np.uint32)
    return ClipState(float(np.frombuffer(raw, np.float64)[0]), f[2], f[3], int(u[4]), int(u[5]))


def grad_norm_ws(count, device):
    """Workspace of grad_norm_scale for up to `count` elements: a3dn_grad_norm_ws_bytes zeros (the arrival ticket, which every
    launch leaves at 0 again, and one float64 per block)."""
    return torch.zeros(_lib.load().a3dn_grad_norm_ws_bytes(int(count)) // 8, dtype=torch.int64, device=device)


def _check_ctl(who, ctl, like):
    if ctl.dtype != torch.int64 or ctl.numel() * 8 != _lib.CLIP_CTL_BYTES or not ctl.is_contiguous():
        raise TypeError(f'{who}: ctl is a control block of clip_ctl()')
    if ctl.device != like.device:
        raise ValueError(f'{who}: all tensors on one device')


def grad_norm_scale(g, grad_scale, clip_norm, ctl, ws):
    """NON-REFERENCE (a3dn_grad_norm_scale): one launch that leaves in ctl the float64 sum of squares S of g, the norm
    n = |grad_scale| sqrt(S), scale = grad_scale (n <= clip_norm) or grad_scale * clip_norm / n, and skip = 1 with scale = 0
    where S is not finite.  g: a float32 tensor starting on a 16-byte boundary; clip_norm > 0, inf allowed."""
    if g.numel() == 0:
        raise ValueError('grad_norm_scale: g holds no values')
    _check_momentum('grad_norm_scale', (g,), 'g')
    _check_ctl('grad_norm_scale', ctl, g)
    if ws.dtype != torch.int64 or not ws.is_contiguous() or ws.device != g.device:
        raise TypeError('grad_norm_scale: ws is a workspace of grad_norm_ws() on the device of g')
    grad_scale, clip_norm = float(grad_scale), float(clip_norm)
    if not (math.isfinite(grad_scale) and grad_scale != 0):
        raise ValueError(f'grad_norm_scale: grad_scale {grad_scale!r} must be finite and not 0')
    if not clip_norm > 0:
        raise ValueError(f'grad_norm_scale: clip_norm {clip_norm!r} must be > 0 (inf: measure and skip only)')
    check(_lib.load().a3dn_grad_norm_scale(g.numel(), _ptr(g), grad_scale, clip_norm, _ptr(ctl), _ptr(ws), ws.numel() * 8,
                                           _stream()), 'a3dn_grad_norm_scale')


def momentum_apply_ctl(var, accum, g, lr, momentum, ctl):
    """NON-REFERENCE (a3dn_momentum_apply_ctl): momentum_apply with grad_scale read from ctl on the device; nothing is written
    where ctl says skip."""
    if var.numel() == 0 or accum.numel() != var.numel() or g.numel() != var.numel():
        raise ValueError(f'momentum_apply_ctl: var {tuple(var.shape)}, accum {tuple(accum.shape)} and g {tuple(g.shape)} must '
                         f'hold the same number of values')
    _check_momentum('momentum_apply_ctl', (var, accum, g), 'var, accum, g')
    _check_ctl('momentum_apply_ctl', ctl, var)
    check(_lib.load().a3dn_momentum_apply_ctl(var.numel(), _ptr(var), _ptr(accum), _ptr(g), lr, momentum, _ptr(ctl), _stream()),
          'a3dn_momentum_apply_ctl')


def adam_apply_tf1_ctl(var, m, v, g, lr, beta1, beta2, eps, beta1_power, beta2_power, ctl, poisoned=None):
    """NON-REFERENCE (a3dn_adam_apply_tf1_ctl): adam_apply_tf1 with grad_scale read from ctl on the device; nothing is written,
    `poisoned` included, where ctl says skip."""
    if var.numel() == 0 or any(t.numel() != var.numel() for t in (m, v, g)):
        raise ValueError('adam_apply_tf1_ctl: var, m, v and g must hold the same number of values')
    _check_momentum('adam_apply_tf1_ctl', (var, m, v, g), 'var, m, v, g')
    _check_ctl('adam_apply_tf1_ctl', ctl, var)
    check(_lib.load().a3dn_adam_apply_tf1_ctl(var.numel(), _ptr(var), _ptr(m), _ptr(v), _ptr(g), lr, beta1, beta2, eps,
                                              beta1_power, beta2_power, _ptr(ctl), _ptr(poisoned), _stream()),
          'a3dn_adam_apply_tf1_ctl')


def sgd_apply_ctl(var, g, lr, ctl, floor=None):
    """NON-REFERENCE (a3dn_sgd_apply_ctl; with a floor a3dn_sgd_apply_floor_ctl): sgd_apply / sgd_apply_floor at the rate
    fl32(lr * scale), the product formed on the device from ctl; nothing is written where ctl says skip."""
    if var.numel() == 0 or g.numel() != var.numel():
        raise ValueError(f'sgd_apply_ctl: var {tuple(var.shape)} and g {tuple(g.shape)} must hold the same number of values')
    _check_momentum('sgd_apply_ctl', (var, g), 'var, g')
    _check_ctl('sgd_apply_ctl', ctl, var)
    if floor is None:
        check(_lib.load().a3dn_sgd_apply_ctl(var.numel(), _ptr(var), _ptr(g), lr, _ptr(ctl), _stream()), 'a3dn_sgd_apply_ctl')
    else:
        check(_lib.load().a3dn_sgd_apply_floor_ctl(var.numel(), _ptr(var), _ptr(g), lr, floor, _ptr(ctl), _stream()),
              'a3dn_sgd_apply_floor_ctl')


def superpixel_mean(x, sp, out=None):
    """[n,h,w,c] -> [n,(h/sp)*(w/sp),c] block means (src/models.py:110,132)."""
    n, h, w, c = x.shape
    out = out if out is not None else torch.empty((n, (h // sp) * (w // sp), c), dtype=torch.float32, device=x.device)
    check(_lib.load().a3d_superpixel_mean(n, h, w, c, _ptr(x), sp, _ptr(out), _stream()), 'a3d_superpixel_mean')
    return out


def _check_operands(who, f32, i32, names):
    """TypeError unless the tensors of f32 are float32 and those of i32 int32; ValueError unless all are contiguous and on
    one device."""
    if any(t.dtype != torch.float32 for t in f32) or any(t.dtype != torch.int32 for t in i32):
        raise TypeError(f'{who}: {names}')
    if not all(t.is_contiguous() for t in (*f32, *i32)):
        raise ValueError(f'{who}: contiguous tensors only')
    if any(t.device != f32[0].device for t in (*f32, *i32)):
        raise ValueError(f'{who}: all tensors on one device')


def _check_superpixels(who, x, sp, channels, max_sp=None):
    """(n, h, w, P) of a non-empty image batch x [n, h, w, channels] cut into P superpixels of edge sp, or ValueError."""
    if (x.dim() != 4 or x.shape[3] != channels or sp <= 0 or (max_sp is not None and sp > max_sp) or x.shape[1] % sp
            or x.shape[2] % sp or x.numel() == 0):
        raise ValueError(f'{who}: x {tuple(x.shape)} is not a non-empty [n, h, w, {channels}] with h, w multiples of '
                         f'sp = {sp}' + (f' <= {max_sp}' if max_sp is not None else ''))
    n, h, w, _ = x.shape
    return n, h, w, (h // sp) * (w // sp)


def superpixel_hist(x, sp, out=None):
    """color_histogram of every superpixel (src/models.py:95-100): [n,h,w,3] -> [n,P,256]."""
    n, h, w, nsp = _check_superpixels('superpixel_hist', x, sp, 3)
    out = out if out is not None else torch.empty((n, nsp, 256), dtype=torch.float32, device=x.device)
    check(_lib.load().a3d_superpixel_hist(n, h, w, _ptr(x), sp, _ptr(out), _stream()), 'a3d_superpixel_hist')
    return out


TEXTURE_MAX_SP = 53      # A3DT_MAX_SP: the texture similarity's sum of squared count differences stays below 2^24


def superpixel_lbp_hist(x, sp, out=None):
    """NON-REFERENCE (a3dt_superpixel_lbp_hist): local-binary-pattern histogram of every superpixel, [n,h,w,3] float32 ->
    [n,P,256] float32 integer counts (each superpixel's sum to sp * sp).  Neighbours are read from the image, across
    superpixel borders, clamped at the image border; sp <= 53."""
    n, h, w, nsp = _check_superpixels('superpixel_lbp_hist', x, sp, 3, TEXTURE_MAX_SP)
    out = out if out is not None else torch.empty((n, nsp, 256), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (n, nsp, 256):
        raise ValueError(f'superpixel_lbp_hist: out {tuple(out.shape)} for x {tuple(x.shape)}, sp {sp} must be '
                         f'{(n, nsp, 256)}')
    _check_operands('superpixel_lbp_hist', (x, out), (), 'x, out float32')
    check(_lib.load().a3dt_superpixel_lbp_hist(n, h, w, _ptr(x), sp, _ptr(out), _stream()), 'a3dt_superpixel_lbp_hist')
    return out


def _pair_similarity(who, x, sp, hists, left, right, dense_w, dense_b, gamma, max_sp=None):
    """pair_similarity (hists: the colour histograms) and pair_similarity3 (and the LBP histograms): one similarity from
    the image and one from each of hists, all [n,P,256]."""
    n, h, w, nsp = _check_superpixels(who, x, sp, 3, max_sp)
    q, k = left.numel(), 1 + len(hists)
    if (q == 0 or right.numel() != q or any(tuple(t.shape) != (n, nsp, 256) for t in hists) or dense_w.numel() != k
            or dense_b.numel() != 1):
        raise ValueError(f'{who}: x {tuple(x.shape)}, sp {sp}, histograms {[tuple(t.shape) for t in hists]}, {q} / '
                         f'{right.numel()} pair indices, dense kernel {tuple(dense_w.shape)}, bias {tuple(dense_b.shape)}')
    _check_operands(who, (x, *hists, dense_w, dense_b), (left, right),
                    'x, hist, lbp_hist, dense_w, dense_b float32; left, right int32')
    sims = torch.empty((n, q, k), dtype=torch.float32, device=x.device)
    r = torch.empty((n, q), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    fn, name = (lib.a3d_pair_similarity, 'a3d_pair_similarity') if k == 2 else (lib.a3dt_pair_similarity3,
                                                                                'a3dt_pair_similarity3')
    check(fn(n, h, w, _ptr(x), sp, *(_ptr(t) for t in hists), _ptr(left), _ptr(right), q, _ptr(dense_w), _ptr(dense_b),
             gamma, _ptr(sims), _ptr(r), _stream()), name)
    return sims, r


def pair_similarity(x, sp, hist, left, right, dense_w, dense_b, gamma=1.0):
    """pairwise_part (src/models.py:108-127): returns (sims [n,Q,2], r [n,Q]).  x [n,h,w,3], hist [n,P,256] float32;
    left, right [Q] int32; dense_w 2 and dense_b 1 float32 values.  A pair with an index outside [0, P) gets NaN."""
    return _pair_similarity('pair_similarity', x, sp, (hist,), left, right, dense_w, dense_b, gamma)


def pair_similarity3(x, sp, hist, lbp_hist, left, right, dense_w, dense_b, gamma=1.0):
    """NON-REFERENCE (a3dt_pair_similarity3): pair_similarity with the texture similarity of the LBP histograms as the
    third: returns (sims [n,Q,3], r [n,Q]); sims[..., :2] are pair_similarity's bits.  x [n,h,w,3], hist and lbp_hist
    [n,P,256] float32; left, right [Q] int32; dense_w 3 and dense_b 1 float32 values.  A pair with an index outside
    [0, P) gets NaN."""
    return _pair_similarity('pair_similarity3', x, sp, (hist, lbp_hist), left, right, dense_w, dense_b, gamma,
                            TEXTURE_MAX_SP)


def _check_crf(who, z, r, left, right, others):
    """(n, P) of a CRF call, or ValueError / TypeError: z [n,P], r [n,Q] and every tensor of `others` [n,P] float32; left,
    right [Q] int32, Q > 0; all contiguous and on one device."""
    if z.dim() != 2 or r.dim() != 2:
        raise ValueError(f'{who}: z {tuple(z.shape)} and r {tuple(r.shape)} must be [n, P] and [n, Q]')
    n, nsp = z.shape[0], z.shape[1]
    if (n == 0 or r.shape[0] != n or left.numel() == 0 or r.shape[1] != left.numel() or left.numel() != right.numel()
            or any(tuple(t.shape) != (n, nsp) for t in others)):
        raise ValueError(f'{who}: z {tuple(z.shape)}, {[tuple(t.shape) for t in others]}, r {tuple(r.shape)}, '
                         f'{left.numel()} / {right.numel()} pair indices')
    _check_operands(who, (z, r, *others), (left, right), 'z, y, r, mu float32; left, right int32')
    return n, nsp


def _crf_outputs(z, r, pair_grad):
    """What every CRF objective writes: (per-image [n], mean [1], dz [n,P], dr [n,Q] or None without pair_grad)."""
    n, nsp = z.shape
    return (torch.empty((n,), dtype=torch.float32, device=z.device), torch.empty((1,), dtype=torch.float32, device=z.device),
            torch.empty((n, nsp), dtype=torch.float32, device=z.device), torch.empty_like(r) if pair_grad else None)


def _crf_loss(who, z, y, r, left, right, eps, pair_grad):
    n, nsp = _check_crf(who, z, r, left, right, (y,))
    per, mean, dz, dr = _crf_outputs(z, r, pair_grad)
    lib = _lib.load()
    args = (n, nsp, _ptr(z), _ptr(y), _ptr(r), _ptr(left), _ptr(right), left.numel(), eps, _ptr(per), _ptr(mean), _ptr(dz))
    if pair_grad:
        check(lib.a3dp_crf_loss_grad(*args, _ptr(dr), _stream()), 'a3dp_crf_loss_grad')
        return mean, per, dz, dr
    check(lib.a3d_crf_loss(*args, _stream()), 'a3d_crf_loss')
    return mean, per, dz


def crf_loss(z, y, r, left, right, eps=1e-7):
    """loss_part (src/models.py:129-177): returns (mean loss [1], per-image loss [n], d mean / d z [n,P]).  z, y [n,P],
    r [n,Q] float32; left, right [Q] int32.  A pair index outside [0, P) turns every loss and all of dz into NaN."""
    return _crf_loss('crf_loss', z, y, r, left, right, eps, False)


def crf_loss_grad(z, y, r, left, right, eps=1e-7):
    """NON-REFERENCE (a3dp_crf_loss_grad): crf_loss with the CRF matrix no longer a constant: returns (mean loss [1],
    per-image loss [n], d mean / d z [n,P], d mean / d r [n,Q]), the first three the bits crf_loss returns.  A pair index
    outside [0, P) turns all of it into NaN; a pair that a later pair overwrote has a gradient of +0."""
    return _crf_loss('crf_loss_grad', z, y, r, left, right, eps, True)


def pair_dense_bwd(sims, dr, dw, db):
    """NON-REFERENCE (a3dp_pair_dense_bwd): backward of the pairwise dense layer K -> 1.  sims [n,Q,K], dr [n,Q] float32 ->
    dw (K values) = sum dr * sims, db (1 value) = sum dr, written in place (views of a gradient buffer); 1 <= K <= 8.  One
    block, a fixed order: the same bits on every run."""
    if sims.dim() != 3 or dr.dim() != 2 or tuple(sims.shape[:2]) != tuple(dr.shape) or dr.numel() == 0:
        raise ValueError(f'pair_dense_bwd: sims {tuple(sims.shape)} and dr {tuple(dr.shape)} must be [n, Q, K] and [n, Q]')
    k = sims.shape[2]
    if not 1 <= k <= 8 or dw.numel() != k or db.numel() != 1:
        raise ValueError(f'pair_dense_bwd: {k} similarities per pair (1 .. 8), dw {tuple(dw.shape)}, db {tuple(db.shape)}')
    _check_operands('pair_dense_bwd', (sims, dr, dw, db), (), 'sims, dr, dw, db float32')
    check(_lib.load().a3dp_pair_dense_bwd(dr.shape[0], dr.shape[1], k, _ptr(sims), _ptr(dr), _ptr(dw), _ptr(db), _stream()),
          'a3dp_pair_dense_bwd')
    return dw, db


def crf_map(z, r, left, right, y=None, status=None):
    """The field's MAP depths y = A^-1 z, A = I + D - R from the pair weights r (a3d_crf_map): z [n,P], r [n,Q] ->
    (y [n,P] float32, status [n] int32; 1 where the image's system was singular or not finite and its row of y is NaN)."""
    y = y if y is not None else torch.empty_like(z)
    n, nsp = _check_crf('crf_map', z, r, left, right, (y,))
    status = status if status is not None else torch.empty((n,), dtype=torch.int32, device=z.device)
    if status.dtype != torch.int32:
        raise TypeError('crf_map: y float32, status int32')
    if status.numel() != n or not status.is_contiguous() or status.device != z.device:
        raise ValueError(f'crf_map: status {tuple(status.shape)} on {status.device} for {n} images on {z.device}')
    check(_lib.load().a3d_crf_map(n, nsp, _ptr(z), _ptr(r), _ptr(left), _ptr(right), left.numel(), _ptr(y), _ptr(status),
                                  _stream()), 'a3d_crf_map')
    return y, status


def superpixel_mean_valid(x, sp, min_count=0, out=None, count=None):
    """NON-REFERENCE (a3dv_superpixel_mean_valid): superpixel_mean of a one-channel map with holes.  x [n,h,w,1] float32
    with NaN (or an infinity) where nothing was measured -> (y [n,P] float32, count [n,P] int32): per superpixel the number
    of finite pixels and their mean, NaN where fewer than max(1, min_count) are finite.  With every pixel finite y is
    superpixel_mean's bits."""
    n, h, w, nsp = _check_superpixels('superpixel_mean_valid', x, sp, 1)
    if min_count < 0:
        raise ValueError(f'superpixel_mean_valid: min_count {min_count}')
    out = out if out is not None else torch.empty((n, nsp), dtype=torch.float32, device=x.device)
    count = count if count is not None else torch.empty((n, nsp), dtype=torch.int32, device=x.device)
    if out.numel() != n * nsp or count.numel() != out.numel():
        raise ValueError(f'superpixel_mean_valid: out {tuple(out.shape)}, count {tuple(count.shape)} for {(n, nsp)}')
    _check_operands('superpixel_mean_valid', (x, out), (count,), 'x, out float32; count int32')
    check(_lib.load().a3dv_superpixel_mean_valid(n, h, w, _ptr(x), sp, int(min_count), _ptr(out), _ptr(count), _stream()),
          'a3dv_superpixel_mean_valid')
    return out, count


def crf_loss_observed(z, y, r, left, right, pair_grad=True):
    """NON-REFERENCE (a3dv_crf_loss_observed): the CRF's negative log-likelihood of the superpixels whose target is finite,
    the others integrated out: returns (mean [1], per-image [n], d mean / d z [n,P], d mean / d r [n,Q] or None without
    pair_grad, nobs [n] int32, status [n] int32).  z, y [n,P] (y NaN where there is no target), r [n,Q] float32; left,
    right [Q] int32.  An image without a target has loss 0 and zero gradients; one whose A is not positive is NaN with
    status 1; a pair index outside [0, P) turns all of it into NaN."""
    n, nsp = _check_crf('crf_loss_observed', z, r, left, right, (y,))
    per, mean, dz, dr = _crf_outputs(z, r, pair_grad)
    nobs = torch.empty((n,), dtype=torch.int32, device=z.device)
    status = torch.empty((n,), dtype=torch.int32, device=z.device)
    check(_lib.load().a3dv_crf_loss_observed(n, nsp, _ptr(z), _ptr(y), _ptr(r), _ptr(left), _ptr(right), left.numel(),
                                             _ptr(per), _ptr(mean), _ptr(dz), _ptr(dr), _ptr(nobs), _ptr(status),
                                             _stream()), 'a3dv_crf_loss_observed')
    return mean, per, dz, dr, nobs, status


BAND_MAX_SP, BAND_MAX_BAND = 768, 32         # A3DB_MAX_SP, A3DB_MAX_BAND


def pair_band(left, right):
    """max |l - r| over the pairs (host integer sequences of one length, not empty): the `band` of crf_band_nll and
    crf_band_map, which cannot look at the device's lists."""
    left, right = [int(v) for v in left], [int(v) for v in right]
    if not left or len(left) != len(right):
        raise ValueError(f'pair_band: {len(left)} / {len(right)} pair indices')
    return max(abs(a - b) for a, b in zip(left, right))


def _check_band(who, z, r, left, right, band, others):
    """_check_crf, then the banded kernels' limits."""
    n, nsp = _check_crf(who, z, r, left, right, others)
    if not 1 <= nsp <= BAND_MAX_SP or not 1 <= int(band) <= BAND_MAX_BAND:
        raise ValueError(f'{who}: {nsp} superpixels (1 .. {BAND_MAX_SP}), band {band} (1 .. {BAND_MAX_BAND})')
    return n, nsp


def crf_band_nll(z, y, r, left, right, band, pair_grad=True, want_mu=False):
    """NON-REFERENCE (a3db_crf_band_nll): the CRF's negative log-likelihood e^T A e - log det A / 2 + P log(pi) / 2 of a
    banded A (every pair |l - r| <= band = pair_band(left, right)), up to 768 superpixels: returns (mean [1], per-image
    [n], d mean / d z [n,P], d mean / d r [n,Q] or None without pair_grad, mu = A^-1 z [n,P] or None without want_mu,
    status [n] int32).  z, y [n,P], r [n,Q] float32; left, right [Q] int32.  An image whose A is not positive is NaN with
    status 1; a pair index outside [0, P) or farther apart than band turns all of it into NaN."""
    n, nsp = _check_band('crf_band_nll', z, r, left, right, band, (y,))
    per, mean, dz, dr = _crf_outputs(z, r, pair_grad)
    mu = torch.empty((n, nsp), dtype=torch.float32, device=z.device) if want_mu else None
    status = torch.empty((n,), dtype=torch.int32, device=z.device)
    check(_lib.load().a3db_crf_band_nll(n, nsp, int(band), _ptr(z), _ptr(y), _ptr(r), _ptr(left), _ptr(right), left.numel(),
                                        _ptr(per), _ptr(mean), _ptr(dz), _ptr(dr), _ptr(mu), _ptr(status), _stream()),
          'a3db_crf_band_nll')
    return mean, per, dz, dr, mu, status


def crf_band_map(z, r, left, right, band, mu=None, status=None):
    """NON-REFERENCE (a3db_crf_band_map): the field's MAP depths mu = A^-1 z of a banded A, as crf_map for up to 768
    superpixels: z [n,P], r [n,Q] -> (mu [n,P] float32, status [n] int32; 1 where A was not positive or the solution not
    finite and the row of mu is NaN)."""
    mu = mu if mu is not None else torch.empty_like(z)
    n, nsp = _check_band('crf_band_map', z, r, left, right, band, (mu,))
    status = status if status is not None else torch.empty((n,), dtype=torch.int32, device=z.device)
    if status.dtype != torch.int32 or status.numel() != n or not status.is_contiguous() or status.device != z.device:
        raise ValueError(f'crf_band_map: status {tuple(status.shape)} {status.dtype} for {n} images')
    check(_lib.load().a3db_crf_band_map(n, nsp, int(band), _ptr(z), _ptr(r), _ptr(left), _ptr(right), left.numel(), _ptr(mu),
                                        _ptr(status), _stream()), 'a3db_crf_band_map')
    return mu, status


def crf_band_posterior(z, y, r, left, right, band, want_var=True, mean=None, var=None):
    """NON-REFERENCE (a3dc_crf_band_posterior): the field's mean and variance per superpixel given the superpixels whose y
    is finite (y None: none is), A banded as for crf_band_nll: returns (mean [n,P], var [n,P] or None without want_var,
    nobs [n] int32, status [n] int32).  z, y [n,P], r [n,Q] float32; left, right [Q] int32.  On an observed superpixel mean
    is y's bits and var +0; on the others the conditional mean A_MM^-1 (z_M - A_MO y_O) and 1/2 diag A_MM^-1.  With nothing
    observed mean is crf_band_map's mu bit for bit.  An image whose system is not positive is NaN with status 1; a pair
    index outside [0, P) or farther apart than band turns all of it into NaN.  mean, var: buffers to write into."""
    mean = mean if mean is not None else torch.empty_like(z)
    if var is not None and not want_var:
        raise ValueError('crf_band_posterior: a var buffer without want_var')
    if want_var and var is None:
        var = torch.empty_like(z)
    others = tuple(t for t in (y, mean, var) if t is not None)
    if any(not isinstance(t, torch.Tensor) for t in others):
        raise TypeError('crf_band_posterior: y, mean, var are tensors (y may be None)')
    n, nsp = _check_band('crf_band_posterior', z, r, left, right, band, others)
    nobs = torch.empty((n,), dtype=torch.int32, device=z.device)
    status = torch.empty((n,), dtype=torch.int32, device=z.device)
    check(_lib.load().a3dc_crf_band_posterior(n, nsp, int(band), _ptr(z), _ptr(y), _ptr(r), _ptr(left), _ptr(right),
                                              left.numel(), _ptr(mean), _ptr(var), _ptr(nobs), _ptr(status), _stream()),
          'a3dc_crf_band_posterior')
    return mean, var, nobs, status


FCSP_MAX_SP = 64       # A3DF_MAX_SP: one lane of a wave per window pixel, 2 KiB of LDS for a block's counts


class FcspMap:
    """NON-REFERENCE (include/a3d_fcsp.h): the validated pixel-to-cell tables of superpixel pooling on the device.  ymap [H],
    xmap [W] (host integer sequences): image row y belongs to feature row ymap[y] of a [h, w] map, column x to xmap[x];
    superpixels of edge sp.  Holds ymap, xmap (int32 device tensors) and H, W, h, w, sp.  ValueError for tables of the wrong
    length (H, W positive multiples of sp, 0 < sp <= 64), out of range, or decreasing."""

    def __init__(self, ymap, xmap, h, w, sp, device='cuda', H=None, W=None):
        import numpy as np
        ya, xa = np.asarray(ymap), np.asarray(xmap)
        h, w, sp = int(h), int(w), int(sp)
        if not 0 < sp <= FCSP_MAX_SP or h <= 0 or w <= 0:
            raise ValueError(f'FcspMap: h {h}, w {w}, sp {sp}: a positive map and a superpixel edge in 1 .. {FCSP_MAX_SP}')
        for name, a, want in (('ymap', ya, H), ('xmap', xa, W)):
            if a.ndim != 1 or a.size == 0 or a.size % sp or a.dtype.kind not in 'iu' or (want is not None and a.size != want):
                raise ValueError(f'FcspMap: {name} of shape {a.shape}, {a.dtype} is not one integer per image '
                                 f'{"row" if name == "ymap" else "column"}'
                                 + (f' ({want})' if want is not None else '') + f', a positive multiple of sp = {sp}')
        for name, a, lim in (('ymap', ya, h), ('xmap', xa, w)):
            if a.min() < 0 or a.max() >= lim:
                raise ValueError(f'FcspMap: {name} has entries outside [0, {lim})')
            if (np.diff(a.astype(np.int64)) < 0).any():
                raise ValueError(f'FcspMap: {name} decreases')
        self.H, self.W, self.h, self.w, self.sp = int(ya.size), int(xa.size), h, w, sp
        self.S = (self.H // sp) * (self.W // sp)
        self.ymap = torch.from_numpy(np.ascontiguousarray(ya, np.int32)).to(device)
        self.xmap = torch.from_numpy(np.ascontiguousarray(xa, np.int32)).to(device)


def _fcsp_args(who, feat, tables, pooled, channels):
    """(n, h, w, C, ld, H, W, sp, ymap, xmap, S, ldp) of a pooling call.  feat [n,h,w,ld], pooled [n,S,ldp] or None (then
    [n,S,C] is the shape to allocate); tables: an FcspMap, or (ymap, xmap, sp) device tables taken as they are."""
    if isinstance(tables, FcspMap):
        ymap, xmap, sp = tables.ymap, tables.xmap, tables.sp
        if feat.dim() == 4 and tuple(feat.shape[1:3]) != (tables.h, tables.w):
            raise ValueError(f'{who}: a map of {tuple(feat.shape[1:3])} cells, tables made for {(tables.h, tables.w)}')
    else:
        ymap, xmap, sp = tables
    if feat.dim() != 4 or feat.numel() == 0:
        raise ValueError(f'{who}: feature map {tuple(feat.shape)} is not a non-empty [n, h, w, ld]')
    n, h, w, ld = feat.shape
    C = ld if channels is None else int(channels)
    H, W = ymap.numel(), xmap.numel()
    if not 0 < sp <= FCSP_MAX_SP or H == 0 or W == 0 or H % sp or W % sp or not 0 < C <= ld:
        raise ValueError(f'{who}: tables of {H} and {W} entries, sp {sp} (<= {FCSP_MAX_SP}), {C} channels of {ld}')
    S = (H // sp) * (W // sp)
    if pooled is not None and (pooled.dim() != 3 or tuple(pooled.shape[:2]) != (n, S) or pooled.shape[2] < C):
        raise ValueError(f'{who}: pooled {tuple(pooled.shape)} for {n} images, {S} superpixels, {C} channels')
    ts = [t for t in (feat, pooled) if t is not None]
    if any(t.dtype != torch.float32 for t in ts) or ymap.dtype != torch.int32 or xmap.dtype != torch.int32:
        raise TypeError(f'{who}: feature map and pooled rows float32; tables int32')
    if not all(t.is_contiguous() for t in ts + [ymap, xmap]):
        raise ValueError(f'{who}: contiguous tensors only')
    if any(t.device != feat.device for t in ts + [ymap, xmap]):
        raise ValueError(f'{who}: all tensors on one device')
    return n, h, w, C, ld, H, W, sp, ymap, xmap, S, (C if pooled is None else pooled.shape[2])


def superpixel_pool_fwd(feat, tables, pooled=None, channels=None):
    """NON-REFERENCE (a3df_superpixel_pool_fwd): the mean of the feature map, upsampled by the tables, over every
    superpixel: feat [n,h,w,ld] float32 -> pooled [n,S,ldp]; only the first `channels` (default all) of a pixel are read and
    written.  Cells are summed in ascending (i, j) with integer weights, zero weights skipped, one division by sp * sp."""
    n, h, w, C, ld, H, W, sp, ymap, xmap, S, ldp = _fcsp_args('superpixel_pool_fwd', feat, tables, pooled, channels)
    if pooled is None:
        pooled = torch.empty((n, S, C), dtype=torch.float32, device=feat.device)
    check(_lib.load().a3df_superpixel_pool_fwd(n, h, w, C, _ptr(feat), ld, H, W, sp, _ptr(ymap), _ptr(xmap), _ptr(pooled),
                                               ldp, _stream()), 'a3df_superpixel_pool_fwd')
    return pooled


def superpixel_pool_bwd(dpooled, tables, dfeat, channels=None):
    """NON-REFERENCE (a3df_superpixel_pool_bwd): the transpose, dpooled [n,S,ldp] -> dfeat [n,h,w,ld], a gather; every
    element of dfeat[..., :channels] is written (+0 where no pixel maps to the cell)."""
    n, h, w, C, ld, H, W, sp, ymap, xmap, S, ldp = _fcsp_args('superpixel_pool_bwd', dfeat, tables, dpooled, channels)
    check(_lib.load().a3df_superpixel_pool_bwd(n, h, w, C, _ptr(dpooled), ldp, H, W, sp, _ptr(ymap), _ptr(xmap), _ptr(dfeat),
                                               ld, _stream()), 'a3df_superpixel_pool_bwd')
    return dfeat


SLIC_MAX_SP = 64               # A3DS_MAX_SP
SLIC_MAX_CELLS = 4096          # A3DS_MAX_CELLS: the label pooling's forward keeps one count per cell of the map in LDS
SLIC_MAX_SUPERPIXELS = 768     # A3DS_MAX_SUPERPIXELS: its backward one per superpixel of an image


def _slic_image(who, x, sp, channels, labels=None, coords=False):
    """(n, H, W, S) of a label call on a non-empty image batch x [n,H,W,channels] float32 with labels [n,H,W] int32 (when
    given), or ValueError / TypeError.  channels: an int, or None for 1 .. 4.  coords: the call forms coordinate means."""
    sp = int(sp)
    ok = x.dim() == 4 and x.numel() > 0 and 0 < sp <= SLIC_MAX_SP and x.shape[1] % sp == 0 and x.shape[2] % sp == 0
    if not ok or (x.shape[3] != channels if channels is not None else not 1 <= x.shape[3] <= 4):
        raise ValueError(f'{who}: x {tuple(x.shape)} is not a non-empty [n, H, W, {channels or "1 .. 4"}] with H, W multiples '
                         f'of sp = {sp} <= {SLIC_MAX_SP}')
    n, H, W, _ = x.shape
    if coords and 9 * sp * sp * max(H, W) >= 1 << 24:
        raise ValueError(f'{who}: 9 sp^2 max(H, W) = {9 * sp * sp * max(H, W)} reaches 2^24 (H {H}, W {W}, sp {sp}): the '
                         f'coordinate sums would not be exact in float32')
    if labels is not None and tuple(labels.shape) != (n, H, W):
        raise ValueError(f'{who}: labels {tuple(labels.shape)} for x {tuple(x.shape)} must be {(n, H, W)}')
    return n, H, W, (H // sp) * (W // sp)


def _slic_out(who, name, t, shape, dtype, device):
    """The output tensor `t`, allocated when None, or ValueError unless it has the shape."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{who}: {name} {tuple(t.shape)} must be {tuple(shape)}')
    return t


def _slic_compactness(who, compactness):
    compactness = float(compactness)
    if not 0 <= compactness < float('inf'):
        raise ValueError(f'{who}: compactness {compactness} is negative or not finite')
    return compactness


def label_mean(x, sp, labels, mean=None, count=None):
    """NON-REFERENCE (a3ds_label_mean): x [n,H,W,c] float32 (c in 1 .. 4), labels [n,H,W] int32 -> (mean [n,S,c] float32,
    count [n,S] int32) over the pixels that count for every superpixel (label s, and s among the pixel's 3 x 3 candidates);
    NaN where count is 0."""
    n, H, W, S = _slic_image('label_mean', x, sp, None, labels)
    c = x.shape[3]
    mean = _slic_out('label_mean', 'mean', mean, (n, S, c), torch.float32, x.device)
    count = _slic_out('label_mean', 'count', count, (n, S), torch.int32, x.device)
    _check_operands('label_mean', (x, mean), (labels, count), 'x, mean float32; labels, count int32')
    check(_lib.load().a3ds_label_mean(n, H, W, c, _ptr(x), int(sp), _ptr(labels), _ptr(mean), _ptr(count), _stream()),
          'a3ds_label_mean')
    return mean, count


def label_hist(x, sp, labels, out=None):
    """NON-REFERENCE (a3ds_label_hist): superpixel_hist over the pixels that count for every superpixel of a label map:
    x [n,H,W,3] float32, labels [n,H,W] int32 -> [n,S,256] float32 integer counts."""
    n, H, W, S = _slic_image('label_hist', x, sp, 3, labels)
    out = _slic_out('label_hist', 'out', out, (n, S, 256), torch.float32, x.device)
    _check_operands('label_hist', (x, out), (labels,), 'x, out float32; labels int32')
    check(_lib.load().a3ds_label_hist(n, H, W, _ptr(x), int(sp), _ptr(labels), _ptr(out), _stream()), 'a3ds_label_hist')
    return out


def slic_update(x, sp, labels, centres, count=None):
    """NON-REFERENCE (a3ds_slic_update): the centres (ybar, xbar, c0, c1, c2) of a segmentation, written into centres
    [n,S,5] (in/out: the row of a superpixel without pixels is left alone); returns (centres, count [n,S] int32)."""
    n, H, W, S = _slic_image('slic_update', x, sp, 3, labels, coords=True)
    centres = _slic_out('slic_update', 'centres', centres, (n, S, 5), torch.float32, x.device)
    count = _slic_out('slic_update', 'count', count, (n, S), torch.int32, x.device)
    _check_operands('slic_update', (x, centres), (labels, count), 'x, centres float32; labels, count int32')
    check(_lib.load().a3ds_slic_update(n, H, W, _ptr(x), int(sp), _ptr(labels), _ptr(centres), _ptr(count), _stream()),
          'a3ds_slic_update')
    return centres, count


def slic_assign(x, sp, centres, compactness, labels=None):
    """NON-REFERENCE (a3ds_slic_assign): every pixel to the nearest of the up to nine centres around its home cell, in
    colour plus (compactness / sp)^2 times position; ties to the lowest index, NaN distances skipped, the anchor pixel of
    every cell kept.  x [n,H,W,3], centres [n,S,5] float32 -> labels [n,H,W] int32."""
    n, H, W, S = _slic_image('slic_assign', x, sp, 3, labels, coords=True)
    compactness = _slic_compactness('slic_assign', compactness)
    if tuple(centres.shape) != (n, S, 5):
        raise ValueError(f'slic_assign: centres {tuple(centres.shape)} must be {(n, S, 5)}')
    labels = _slic_out('slic_assign', 'labels', labels, (n, H, W), torch.int32, x.device)
    _check_operands('slic_assign', (x, centres), (labels,), 'x, centres float32; labels int32')
    check(_lib.load().a3ds_slic_assign(n, H, W, _ptr(x), int(sp), _ptr(centres), compactness, _ptr(labels), _stream()),
          'a3ds_slic_assign')
    return labels


def slic_segment(x, sp, iters=5, compactness=0.1, labels=None, centres=None, count=None):
    """NON-REFERENCE (a3ds_slic_segment): grid labels, slic_update, then iters x (slic_assign, slic_update): x [n,H,W,3]
    float32 -> (labels [n,H,W] int32, centres [n,S,5] float32, count [n,S] int32).  iters = 0 gives the grid."""
    n, H, W, S = _slic_image('slic_segment', x, sp, 3, labels, coords=True)
    compactness = _slic_compactness('slic_segment', compactness)
    if int(iters) != iters or iters < 0:
        raise ValueError(f'slic_segment: iters {iters} is not a non-negative integer')
    labels = _slic_out('slic_segment', 'labels', labels, (n, H, W), torch.int32, x.device)
    centres = _slic_out('slic_segment', 'centres', centres, (n, S, 5), torch.float32, x.device)
    count = _slic_out('slic_segment', 'count', count, (n, S), torch.int32, x.device)
    _check_operands('slic_segment', (x, centres), (labels, count), 'x, centres float32; labels, count int32')
    check(_lib.load().a3ds_slic_segment(n, H, W, _ptr(x), int(sp), int(iters), compactness, _ptr(labels), _ptr(centres),
                                        _ptr(count), _stream()), 'a3ds_slic_segment')
    return labels, centres, count


def label_pair_similarity(mean3, hist, count, left, right, dense_w, dense_b, gamma=1.0):
    """NON-REFERENCE (a3ds_pair_similarity): the paper's colour and histogram similarities from label statistics, and the
    pairwise dense layer: mean3 [n,S,3], hist [n,S,256] float32, count [n,S] int32, left, right [Q] int32, dense_w 2 and
    dense_b 1 float32 values -> (sims [n,Q,2], r [n,Q]).  A pair with an index outside [0, S) gets NaN."""
    who = 'label_pair_similarity'
    q = left.numel()
    if (mean3.dim() != 3 or mean3.shape[2] != 3 or mean3.numel() == 0 or tuple(hist.shape) != (*mean3.shape[:2], 256)
            or tuple(count.shape) != tuple(mean3.shape[:2]) or q == 0 or right.numel() != q or dense_w.numel() != 2
            or dense_b.numel() != 1):
        raise ValueError(f'{who}: mean3 {tuple(mean3.shape)}, hist {tuple(hist.shape)}, count {tuple(count.shape)}, {q} / '
                         f'{right.numel()} pair indices, dense kernel {tuple(dense_w.shape)}, bias {tuple(dense_b.shape)}')
    _check_operands(who, (mean3, hist, dense_w, dense_b), (count, left, right),
                    'mean3, hist, dense_w, dense_b float32; count, left, right int32')
    n, S, _ = mean3.shape
    sims = torch.empty((n, q, 2), dtype=torch.float32, device=mean3.device)
    r = torch.empty((n, q), dtype=torch.float32, device=mean3.device)
    check(_lib.load().a3ds_pair_similarity(n, S, _ptr(mean3), _ptr(hist), _ptr(count), _ptr(left), _ptr(right), q,
                                           _ptr(dense_w), _ptr(dense_b), gamma, _ptr(sims), _ptr(r), _stream()),
          'a3ds_pair_similarity')
    return sims, r


def _label_pool_args(who, feat, tables, labels, count, pooled, channels):
    """_fcsp_args plus the label map and counts of a3ds_label_pool_*: labels [n,H,W], count [n,S] int32."""
    args = _fcsp_args(who, feat, tables, pooled, channels)
    n, h, w, _, _, H, W, _, _, _, S, _ = args
    if h * w > SLIC_MAX_CELLS or S > SLIC_MAX_SUPERPIXELS:
        raise ValueError(f'{who}: a map of {h * w} cells (at most {SLIC_MAX_CELLS}), {S} superpixels (at most '
                         f'{SLIC_MAX_SUPERPIXELS})')
    if tuple(labels.shape) != (n, H, W) or tuple(count.shape) != (n, S):
        raise ValueError(f'{who}: labels {tuple(labels.shape)}, count {tuple(count.shape)} must be {(n, H, W)}, {(n, S)}')
    _check_operands(who, (feat,), (labels, count), 'labels, count int32')
    return args


def label_pool_fwd(feat, tables, labels, count, pooled=None, channels=None):
    """NON-REFERENCE (a3ds_label_pool_fwd): superpixel_pool_fwd over the superpixels of a label map: the mean of the
    upsampled feature map over the pixels that count for each, divided by count [n,S]; +0 where count is 0."""
    n, h, w, C, ld, H, W, sp, ymap, xmap, S, ldp = _label_pool_args('label_pool_fwd', feat, tables, labels, count, pooled,
                                                                    channels)
    if pooled is None:
        pooled = torch.empty((n, S, C), dtype=torch.float32, device=feat.device)
    check(_lib.load().a3ds_label_pool_fwd(n, h, w, C, _ptr(feat), ld, H, W, sp, _ptr(ymap), _ptr(xmap), _ptr(labels),
                                          _ptr(count), _ptr(pooled), ldp, _stream()), 'a3ds_label_pool_fwd')
    return pooled


def label_pool_bwd(dpooled, tables, labels, count, dfeat, channels=None):
    """NON-REFERENCE (a3ds_label_pool_bwd): the exact transpose, dpooled [n,S,ldp] -> dfeat [n,h,w,ld]; every element of
    dfeat[..., :channels] is written."""
    n, h, w, C, ld, H, W, sp, ymap, xmap, S, ldp = _label_pool_args('label_pool_bwd', dfeat, tables, labels, count, dpooled,
                                                                    channels)
    check(_lib.load().a3ds_label_pool_bwd(n, h, w, C, _ptr(dpooled), ldp, H, W, sp, _ptr(ymap), _ptr(xmap), _ptr(labels),
                                          _ptr(count), _ptr(dfeat), ld, _stream()), 'a3ds_label_pool_bwd')
    return dfeat


def paint_labels(values, labels):
    """values [n,S] -> [n,H,W]: every pixel gets the value of its label (labels [n,H,W] int32, all in [0, S): a
    segmentation of slic_segment).  Plumbing, a torch.gather; not on the training path."""
    if values.dim() != 2 or labels.dim() != 3 or labels.shape[0] != values.shape[0]:
        raise ValueError(f'paint_labels: values {tuple(values.shape)}, labels {tuple(labels.shape)}')
    return torch.gather(values, 1, labels.reshape(labels.shape[0], -1).long()).reshape(labels.shape)


UPSAMPLE_MAX_RADIUS = 4      # A3DU_MAX_RADIUS: 81 cells per output pixel
UPSAMPLE_GRID = (240, 320)   # the grid DCNF's superpixels are cut from (models.DCNF_IMG_H, DCNF_IMG_W)


def upsample_tables(gh, gw, H, W, kind, sp=None):
    """The four host tables of a3du_joint_bilateral_upsample for a gh x gw prediction and an H x W image: (cy [H], cx [W]
    float32, ay [gh], ax [gw] int32), computed in float64 and cast.  Both kinds relate two sizes as resize_bilinear_tf1
    does: pixel u of a size S sits at pixel u * H / S of a size H (no half-pixel shift).

    kind='corner' (msdn): the targets were made by that resize, so cell i stands for relative position i / gh:
        cy[y] = y * gh / H,  ay[i] = clamp(floor(i * H / gh + 1/2), 0, H - 1).
    kind='block' (dcnf): cell R is the mean of rows [R sp, (R + 1) sp) of the 240 x 320 grid; with u = y * 240 / H
        cy[y] = (u + 1/2) / sp - 1/2,  ay[R] = clamp(floor((R + 1/2) * sp * H / 240), 0, H - 1),
    the image row in the middle of the rows [R sp H / 240, (R + 1) sp H / 240) the block covers, the later of the two
    when the middle falls between rows (H = 240: 20, 60, ..; H = 480: 40, 120, ..).  Carrying the grid's middle row
    (R + 1/2) sp - 1/2 through the legacy mapping instead gives the earlier one there (39, 119, .. at H = 480); both are
    half a pixel from the middle.  The same along x with 320."""
    import numpy as np
    gh, gw, H, W = int(gh), int(gw), int(H), int(W)
    if min(gh, gw, H, W) <= 0:
        raise ValueError(f'upsample_tables: a {gh} x {gw} grid and a {H} x {W} image must be positive')
    if kind == 'corner':
        if sp is not None:
            raise ValueError(f"upsample_tables: sp = {sp!r} goes with kind='block'")
        c = [np.arange(S, dtype=np.float64) * g / S for g, S in ((gh, H), (gw, W))]
        a = [np.floor(np.arange(g, dtype=np.float64) * S / g + 0.5) for g, S in ((gh, H), (gw, W))]
    elif kind == 'block':
        G = UPSAMPLE_GRID
        if sp is None or int(sp) <= 0 or G[0] % int(sp) or G[1] % int(sp) or (gh, gw) != (G[0] // int(sp), G[1] // int(sp)):
            raise ValueError(f"upsample_tables: kind='block' is a {G[0]} x {G[1]} grid cut into superpixels of edge sp; "
                             f'sp = {sp!r} does not give {gh} x {gw} cells')
        sp = int(sp)
        c = [(np.arange(S, dtype=np.float64) * g / S + 0.5) / sp - 0.5 for g, S in zip(G, (H, W))]
        a = [np.floor((np.arange(n, dtype=np.float64) + 0.5) * sp * S / g) for n, g, S in zip((gh, gw), G, (H, W))]
    else:
        raise ValueError(f"upsample_tables: kind {kind!r}: 'corner' or 'block'")
    ay, ax = (np.clip(t, 0, S - 1).astype(np.int32) for t, S in zip(a, (H, W)))
    return c[0].astype(np.float32), c[1].astype(np.float32), ay, ax


class UpsampleMap:
    """NON-REFERENCE (include/a3d_upsample.h): the tables of joint_bilateral_upsample on the device, built once per pair of
    sizes (upsample_tables).  Holds cy, cx (float32), ay, ax (int32) and gh, gw, H, W, kind, sp.  device='cpu' builds them
    without a GPU (for inspection; the launch refuses them)."""

    def __init__(self, gh, gw, H, W, kind, sp=None, device='cuda'):
        cy, cx, ay, ax = upsample_tables(gh, gw, H, W, kind, sp)
        self.gh, self.gw, self.H, self.W, self.kind, self.sp = int(gh), int(gw), int(H), int(W), kind, sp
        self.cy, self.cx, self.ay, self.ax = (torch.from_numpy(t).to(device) for t in (cy, cx, ay, ax))


# The defaults are choices, not derivations: sigma_space is in cells (1: the neighbouring cell weighs e^-1/2), sigma_range
# in colour units of [0, 1] (0.1: a step of a quarter of the range in one channel is worth e^-3).  Whether they are good
# on NYU has not been shown: no run on a data set stands behind them.
UPSAMPLE_RADIUS, UPSAMPLE_SIGMA_SPACE, UPSAMPLE_SIGMA_RANGE = 2, 1.0, 0.1


def upsample_params(radius, sigma_space, sigma_range):
    """(R, inv2ss, inv2sr) as a3du_joint_bilateral_upsample takes them, or ValueError: an integer radius in 1 .. 4; sigmas
    > 0, inf allowed (inv = 0: that term is off), whose 1 / (2 sigma^2) is finite in float32."""
    import numpy as np
    if int(radius) != radius or not 1 <= int(radius) <= UPSAMPLE_MAX_RADIUS:
        raise ValueError(f'joint_bilateral_upsample: radius {radius!r} is not an integer in 1 .. {UPSAMPLE_MAX_RADIUS}')
    inv = []
    for name, s in (('sigma_space', sigma_space), ('sigma_range', sigma_range)):
        s = float(s)
        if not s > 0:
            raise ValueError(f'joint_bilateral_upsample: {name} {s!r} must be > 0 (inf switches the term off)')
        with np.errstate(over='ignore'):
            v = float(np.float32(0.0 if s == float('inf') else 1.0 / (2.0 * s * s)))
        if not v < float('inf'):
            raise ValueError(f'joint_bilateral_upsample: 1 / (2 {name}^2) with {name} = {s!r} is not finite in float32')
        inv.append(v)
    return int(radius), inv[0], inv[1]


def joint_bilateral_upsample(depth, guide, tables, radius=UPSAMPLE_RADIUS, sigma_space=UPSAMPLE_SIGMA_SPACE,
                             sigma_range=UPSAMPLE_SIGMA_RANGE, out=None):
    """NON-REFERENCE (a3du_joint_bilateral_upsample): depth [n, gh, gw] float32 -> out [n, H, W] float32 under guide
    [n, H, W, 3], float32 or the uint8 pixel values k (read as fl(k / 255)); tables: an UpsampleMap of these sizes.  Every
    output pixel is the weighted mean of the finite cells within `radius` of it, w = exp(-dist^2 / (2 sigma_space^2)
    - |colour difference|^2 / (2 sigma_range^2)), clamped to their range; NaN where no cell counts.  sigma_range=inf:
    distance only.  Stream-ordered, no synchronisation."""
    who = 'joint_bilateral_upsample'
    R, inv2ss, inv2sr = upsample_params(radius, sigma_space, sigma_range)
    if not isinstance(tables, UpsampleMap):
        raise TypeError(f'{who}: tables must be an ops.UpsampleMap')
    if depth.dim() != 3 or guide.dim() != 4 or depth.numel() == 0 or guide.shape[3] != 3 or guide.shape[0] != depth.shape[0]:
        raise ValueError(f'{who}: depth {tuple(depth.shape)} and guide {tuple(guide.shape)} must be a non-empty [n, gh, gw] '
                         f'and [n, H, W, 3]')
    n = depth.shape[0]
    if tuple(depth.shape[1:]) != (tables.gh, tables.gw) or tuple(guide.shape[1:3]) != (tables.H, tables.W):
        raise ValueError(f'{who}: depth {tuple(depth.shape)}, guide {tuple(guide.shape)}; tables made for '
                         f'{(tables.gh, tables.gw)} -> {(tables.H, tables.W)}')
    if out is not None and tuple(out.shape) != (n, tables.H, tables.W):
        raise ValueError(f'{who}: out {tuple(out.shape)} must be {(n, tables.H, tables.W)}')
    if depth.dtype != torch.float32 or guide.dtype not in (torch.float32, torch.uint8) or (
            out is not None and out.dtype != torch.float32):
        raise TypeError(f'{who}: depth and out float32; guide float32 or uint8')
    ts = [t for t in (depth, guide, out, tables.cy, tables.cx, tables.ay, tables.ax) if t is not None]
    if not all(t.is_contiguous() for t in ts):
        raise ValueError(f'{who}: contiguous tensors only')
    if not depth.is_cuda or any(t.device != depth.device for t in ts):
        raise ValueError(f'{who}: all tensors on one GPU; ' + ', '.join(sorted({str(t.device) for t in ts})))
    if out is None:
        out = torch.empty((n, tables.H, tables.W), dtype=torch.float32, device=depth.device)
    check(_lib.load().a3du_joint_bilateral_upsample(n, tables.gh, tables.gw, _ptr(depth), tables.H, tables.W, _ptr(guide),
                                                    int(guide.dtype == torch.uint8), _ptr(tables.cy), _ptr(tables.cx),
                                                    _ptr(tables.ay), _ptr(tables.ax), R, inv2ss, inv2sr, _ptr(out), _stream()),
          'a3du_joint_bilateral_upsample')
    return out


class JointUpsampler:
    """joint_bilateral_upsample with fixed parameters for predictions of one model, whatever sizes come: kind / sp as
    upsample_tables takes them (msdn: 'corner'; dcnf: 'block' and the replica's superpixel edge); the tables of every
    pair of sizes are built once and kept.  ValueError at construction for parameters the launch would refuse."""

    def __init__(self, kind, sp=None, radius=UPSAMPLE_RADIUS, sigma_space=UPSAMPLE_SIGMA_SPACE,
                 sigma_range=UPSAMPLE_SIGMA_RANGE):
        upsample_params(radius, sigma_space, sigma_range)
        self.kind, self.sp = kind, sp
        self.radius, self.sigma_space, self.sigma_range = int(radius), float(sigma_space), float(sigma_range)
        self.tables = {}

    def __call__(self, depth, guide, out=None):
        key = (tuple(depth.shape[1:3]), tuple(guide.shape[1:3]), depth.device)
        tables = self.tables.get(key)
        if tables is None:
            tables = self.tables[key] = UpsampleMap(*key[0], *key[1], self.kind, self.sp, device=depth.device)
        return joint_bilateral_upsample(depth, guide, tables, self.radius, self.sigma_space, self.sigma_range, out)


def dropout_keep_mask(keep, seed, step, rate=0.5):
    """Fill the uint8 tensor `keep` with the Bernoulli(1-rate) keep mask of training step `step`."""
    check(_lib.load().a3d_dropout_keep_mask(keep.numel(), seed, step, rate, _ptr(keep), _stream()),
          'a3d_dropout_keep_mask')
    return keep
