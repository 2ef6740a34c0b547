"""The extension header include/a3d_clip.h, the library's a3dn_* exports and _lib.CLIP_SIGNATURES name the same entry points, as
tests/test_abi_optim.py holds include/a3d_optim.h to its exports and bindings; bad arguments are refused before any launch (no
GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3dn_grad_norm_ws_bytes', 'a3dn_grad_norm_scale', 'a3dn_momentum_apply_ctl', 'a3dn_adam_apply_tf1_ctl',
         'a3dn_sgd_apply_ctl', 'a3dn_sgd_apply_floor_ctl'}


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dn_', NAMES)
    for words in ('NON-REFERENCE', 'per optimizer group', 'tf.clip_by_global_norm', 'S = sum of (double)g[i] * (double)g[i] in float64',
                  'n = |gs| * sqrt(S) in float64', 'skipped iff S is not finite', 'scale = 0, skip = 1, skipped += 1',
                  'rounded once', 'scale = gs, the same bits, if n <= C', 'it may be +inf while n is finite, and that is not a skip',
                  'On skip it writes nothing: not var, not a slot,', 'scale == 1 multiplies nothing',
                  "Adam's beta powers", 'and global_step move on a skipped step too', 'every refusal comes before any launch',
                  'stream-ordered', 'offset 20  uint32    skipped', 'reserved, never written', 'floating-point atomics',
                  'no block waits for another', 'no trip count depends on a value', 'the same bits on every run',
                  'lr = fl32(lr * scale), one float32 product formed on the device', 'A3D_EWORKSPACE', 'A3D_EINVAL'):
        assert words in text, words
    macros = dict(re.findall(r'#define (A3DN_[A-Z_]+) (\d+)', code))
    assert macros == {'A3DN_CTL_BYTES': str(_lib.CLIP_CTL_BYTES), 'A3DN_BLOCK_ELEMS': str(_lib.CLIP_BLOCK_ELEMS),
                      'A3DN_MAX_BLOCKS': str(_lib.CLIP_MAX_BLOCKS)}
    # the _ctl forms are the existing rules with grad_scale replaced by the control block
    P, sig = ctypes.c_void_p, _lib.CLIP_SIGNATURES
    mom = _lib.OPTIM_SIGNATURES['a3do_momentum_apply'][1]
    assert sig['a3dn_momentum_apply_ctl'][1] == mom[:6] + [P] + mom[7:] and mom[6] is ctypes.c_float
    adam = _lib.SIGNATURES['a3d_adam_apply_tf1_flag'][1]
    assert sig['a3dn_adam_apply_tf1_ctl'][1] == adam[:11] + [P] + adam[12:] and adam[11] is ctypes.c_float
    sgd = _lib.SIGNATURES['a3d_sgd_apply'][1]
    assert sig['a3dn_sgd_apply_ctl'][1] == sgd[:-1] + [P] + sgd[-1:]
    floor = _lib.PAIR_SIGNATURES['a3dp_sgd_apply_floor'][1]
    assert sig['a3dn_sgd_apply_floor_ctl'][1] == floor[:-1] + [P] + floor[-1:]


def test_workspace_bytes_follow_the_grid():
    lib = _lib.load()
    block, cap = _lib.CLIP_BLOCK_ELEMS, _lib.CLIP_MAX_BLOCKS
    for count, blocks in ((1, 1), (3, 1), (block, 1), (block + 3, 1), (block + 4, 2), (cap * block, cap), (cap * block + 5, cap),
                          (1 << 27, cap)):
        assert lib.a3dn_grad_norm_ws_bytes(count) == -(-(8 + 8 * blocks) // 256) * 256, count


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: the refusal must come first, each with words of its own."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 14)
    p = (ctypes.addressof(buf) + 15) & ~15
    inf, nan = float('inf'), float('nan')

    def norm(count=8, g=p, gs=1.0, clip=1.0, ctl=p + 256, ws=p + 512, nb=8192):
        return lib.a3dn_grad_norm_scale(count, g, gs, clip, ctl, ws, nb, None)

    def momentum(count=8, var=p, accum=p + 256, g=p + 512, ctl=p + 1024):
        return lib.a3dn_momentum_apply_ctl(count, var, accum, g, 0.1, 0.9, ctl, None)

    def adam(count=8, var=p, m=p + 256, v=p + 512, g=p + 768, ctl=p + 1024):
        return lib.a3dn_adam_apply_tf1_ctl(count, var, m, v, g, 0.1, 0.9, 0.999, 1e-8, 0.9, 0.999, ctl, None, None)

    def sgd(count=8, var=p, g=p + 256, ctl=p + 1024):
        return lib.a3dn_sgd_apply_ctl(count, var, g, 0.1, ctl, None)

    def floor(count=8, var=p, g=p + 256, ctl=p + 1024):
        return lib.a3dn_sgd_apply_floor_ctl(count, var, g, 0.1, 0.0, ctl, None)

    def refused(fn, why, code=-1, **kw):
        assert fn(**kw) == code, (fn.__name__, kw)
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        assert why in err.value, (fn.__name__, kw, err.value)

    for kw in ({'g': None}, {'ctl': None}, {'ws': None}):
        refused(norm, b'grad_norm_scale: bad arguments: a NULL pointer', **kw)
    refused(norm, b'grad_norm_scale: bad arguments: no elements', count=0)
    for kw in ({'g': p + 4}, {'g': p + 8}):
        refused(norm, b'the gradient must be 16-byte aligned', **kw)
    for kw in ({'ctl': p + 256 + 4}, {'ws': p + 512 + 4}):
        refused(norm, b'the control block and the workspace must be 8-byte aligned', **kw)
    for gs in (0.0, inf, -inf, nan):
        refused(norm, b'must be finite and not 0', gs=gs)
    for clip in (0.0, -1.0, -inf, nan):
        refused(norm, b'must be > 0', clip=clip)
    refused(norm, b'workspace bytes', code=-2, nb=lib.a3dn_grad_norm_ws_bytes(8) - 1)
    refused(norm, b'workspace bytes', code=-2, count=1 << 20, nb=lib.a3dn_grad_norm_ws_bytes(1 << 20) - 8)

    for kw in ({'var': None}, {'accum': None}, {'g': None}, {'count': 0}):
        refused(momentum, b'momentum_apply_ctl: bad arguments', **kw)
    for kw in ({'var': p + 4}, {'accum': p + 256 + 4}, {'g': p + 512 + 8}):
        refused(momentum, b'momentum_apply_ctl: buffers must be 16-byte aligned', **kw)
    for kw in ({'var': None}, {'m': None}, {'v': None}, {'g': None}, {'count': 0}):
        refused(adam, b'adam_ctl: bad arguments', **kw)
    for kw in ({'var': p + 4}, {'m': p + 256 + 4}, {'v': p + 512 + 4}, {'g': p + 768 + 8}):
        refused(adam, b'adam_ctl: buffers must be 16-byte aligned', **kw)
    for kw in ({'var': None}, {'g': None}, {'count': 0}):
        refused(sgd, b'sgd_ctl: bad arguments', **kw)
        refused(floor, b'sgd_floor_ctl: bad arguments', **kw)
    for fn, who in ((momentum, b'momentum_apply_ctl'), (adam, b'adam_ctl'), (sgd, b'sgd_ctl'), (floor, b'sgd_floor_ctl')):
        refused(fn, who + b': no control block', ctl=None)
        refused(fn, who + b': the control block must be 8-byte aligned', ctl=p + 1024 + 4)
