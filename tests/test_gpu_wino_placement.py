"""The Winograd surfaces and the fused momentum launch under hostile placement: the entries of tests/wino_placement.py (P.ENTRIES:
'fp32w' forward and bwd-data, a3dwg_conv2d_bwd_filter, a3dwb_conv2d_bwd plain / mask / pool, a3dl_conv2d_bwd_data and
a3dl_conv2d_bwd_filter, the three *_prepare_filter calls, a3do_dense_bwd_filter_momentum), called through the C entry points so
that an operand can start at any address.  csrc/wino.hip and csrc/wino1d.hip pick the 16-byte or the scalar transform kernel by
`aligned16(ptr)` of x, dz, dx, mask, the pool's y and the argmax bytes; torch's own allocations are 256-byte aligned, so the other
Winograd tests run the scalar kernels only where c % 4 != 0.  Four parts, with Placed, Workspace and the fault latch of
tests/test_gpu_exact_offgrid.py (a device error ends the module: nothing more is launched):

  B. the placement sweep (P.sweep): every operand a window of a NaN-filled allocation (argmax bytes 9; 64 elements in front, 67
     rows behind, NaN pad columns), each alone at +4 bytes, argmax at +1 too, the image-side operand at +8, all together, the
     workspace at +16 and +4.  Accepted: every output equals its reference over the WHOLE allocation (F(2x2,3x3): the float64
     oracle on ternary operands, no tolerance; F(4,5): the two bounds of tests/test_wino1d_cpu.py; momentum: the two-call form's
     bits) AND the on-grid launch bit for bit, inputs keep their bits, the product's timing record is the on-grid one.  Refused:
     A3D_EINVAL, the message names the operand, outputs hold their fill, and the pair is in P.REFUSED (from the headers).
  C. the dirty workspace: exactly the queried bytes of 0xFF (float32 NaN), 4096 guard bytes behind; the bits of the call on the
     roomy workspace of `ops`; and one workspace that serves the largest case, then the smallest (the bits of fresh zeros).
  D. one NaN (image 0, interior) and one +Inf (last image, border) in x or dz: non-finite where the geometry says they must be,
     the clean run's bits everywhere outside the windows that hold them (P.nonfinite_sets, checked on the CPU against the numpy
     restatements).

What the file bites on was checked with mutated copies of the sources, one change per build, bound through A3D_LIB (DESIGN.md
3.1m).  Two of the four made the tests named here fail and no other; two change no bit of any output, and the reason is given:
  `cq * 4 + e < c` dropped in wino_load_window<false> -> test_placement_f23[*-1x9x9x5x7xSAME] for fwd, fwd_prepared, the four
                                                        bwd_data entries and wb, wb_prepared, wb_mask, wb_prepared_mask (10), and
                                                        test_nonfinite_inputs_stay_in_their_window on that case for fwd, bwd_data and
                                                        wb, per call and prepared (8): the neighbouring pixel's channels and the NaN
                                                        behind the tensor reach V's pad columns, and NaN x 0 is NaN.  The filter
                                                        gradient alone stays exact: there V's pad columns are rows of the slabs
                                                        that wino_dw_item never reads
  transformed_filter accepting an off-grid U         -> all 31 test_placement_f23 / _f45 cases of the *_prepared* entries: U+4 and
                                                        `all` are accepted where P.REFUSED names U
  aligned16(mask) dropped from wino_output           -> none, and none can: the 16-byte kernel then loads the mask with 16-byte
                                                        global loads from a 4-byte aligned address, which gfx950 serves with the
                                                        same values; the host test guards speed, not results
  the pad-column store of wino1d_dz_kernel skipped   -> none, and none can: Z's pad columns lie on the product's N axis, so the
                                                        NaN bytes of a dirty workspace reach only slab and bias-partial columns
                                                        >= k, which wino1d_dw_kernel never reads"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import wino1d_ref as W1
import wino_placement as P
import wino_ref as W
from oracle import tf13_ops as T
from test_gpu_exact_offgrid import FAULTED, ROOMY, Placed, Workspace, launched, route, synchronize
from test_wino1d_cpu import RTOL_F32, rel_l2

pytestmark = pytest.mark.gpu

EINVAL = -1
F64 = np.float64
LAUNCHES = [0]


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


@pytest.fixture(autouse=True)
def no_launch_after_a_device_error():
    assert not FAULTED, f'not run: the device reported an error earlier ({FAULTED[0]})'


# ---------------------------------------------------------------------------------------------------------------- checks
class Exact:
    """the float64 reference, element for element"""

    def __init__(self, ref):
        self.ref = np.asarray(ref, F64)

    def check(self, inside, what):
        np.testing.assert_array_equal(inside, self.ref.reshape(inside.shape), err_msg=what)
        return None


class Bounded:
    """rel-L2 below RTOL_F32 and |got - ref| <= RTOL_F32 * scale element by element (tests/test_wino1d_cpu.py)"""

    def __init__(self, ref, scale):
        self.ref, self.scale = np.asarray(ref, F64), np.asarray(scale, F64)

    def check(self, inside, what):
        ref, scale = self.ref.reshape(inside.shape), self.scale.reshape(inside.shape)
        r = rel_l2(inside, ref)
        err = np.abs(inside - ref)
        worst = float((err / np.maximum(scale, 1e-300)).max())
        print(f'BOUND | {what} | rel-L2 {r:.3e} | worst element {worst / RTOL_F32:.4f} of its bound')
        assert r < RTOL_F32 and (err <= RTOL_F32 * scale).all(), (what, r, worst)
        return worst / RTOL_F32


class Bits:
    """the float32 bits of another launch"""

    def __init__(self, ref):
        self.ref = np.ascontiguousarray(ref, np.float32)

    def check(self, inside, what):
        got = inside.astype(np.float32)      # (it came from float32: exact)
        assert np.array_equal(got.view(np.uint32), self.ref.reshape(got.shape).view(np.uint32)), what
        return None


def whole(pl, cols, what):
    """the window's first `cols` columns as float64, after asserting that everything else of the allocation holds its fill"""
    a = pl.big.cpu().numpy().astype(F64) if pl.dtype == torch.uint8 else pl.big.float().cpu().numpy().astype(F64)
    win = a[pl.front:pl.front + pl.rows * pl.ld].reshape(pl.rows, pl.ld)
    inside = win[:, :cols].copy()
    win[:, :cols] = pl.fill
    assert bool((a == 9).all() if pl.dtype == torch.uint8 else np.isnan(a).all()), f'{what}: written outside its {cols} columns'
    return inside


class Job:
    """One entry on one case.  inputs {operand: (data, rows, ld, cols)}; outputs {operand: (rows, ld, cols, check or None)};
    inout {operand: (data, rows, ld, cols, check or None)}; call(placed, ws, ws_bytes); query() or None."""

    def __init__(self, entry, what, call, query, inputs, outputs, inout=None):
        self.entry, self.what, self.call, self.query = entry, what, call, query
        self.inputs, self.outputs, self.inout = inputs, outputs, inout or {}
        assert set(P.ENTRIES[entry].operands) == set(inputs) | set(outputs) | set(self.inout), entry

    def place(self, offs=None):
        offs = offs or {}
        pl = {}
        for o, v in {**self.inputs, **self.inout}.items():
            pl[o] = Placed(v[1], v[2], offs.get(o, 0), P.operand_type(self.entry, o), v[0], v[3])
        for o, (rows, ld, cols, _) in self.outputs.items():
            pl[o] = Placed(rows, ld, offs.get(o, 0), P.operand_type(self.entry, o))
        return pl

    def results(self):
        return {**self.outputs, **{o: v[1:] for o, v in self.inout.items()}}

    def bits(self, pl):
        return {o: pl[o].bits() for o in self.results()}


# ---------------------------------------------------------------------------------------------------------------- operands, references
@functools.lru_cache(maxsize=None)
def host_w(case):
    """the ternary operands of an F(2x2,3x3) case and their float64 results, computed once"""
    t = P.ternary_operands(case)
    padding = case[5]
    x, g, b, dz = (t[a].astype(F64) for a in ('x', 'w', 'bias', 'dz'))
    dw, db = T.conv2d_bwd_filter(x, dz, g.shape, 1, padding)
    return dict(t, y=T.conv2d_fwd(x, g, b, 1, padding, relu=True), dx=T.conv2d_bwd_data(dz, g, x.shape, 1, padding), dw=dw, db=db)


@functools.lru_cache(maxsize=None)
def host_l(case):
    """the normal operands of an F(4,5) case (W1.operands) and their float64 results and scales, computed once"""
    n, h, w, c, k, r, padding = case[:7]
    x, dz, wt, relu = W1.operands(case, 51)
    shape = (r, 5, c, k)
    ab = lambda a: np.abs(a).astype(F64)      # noqa: E731
    return dict(x=x, dz=dz, w=wt, mask=relu, dx=T.conv2d_bwd_data(dz.astype(F64), wt.astype(F64), (n, h, w, c), 1, padding),
                dx_scale=T.conv2d_bwd_data(ab(dz), ab(wt), (n, h, w, c), 1, padding),
                grads=T.conv2d_bwd_filter(x.astype(F64), dz.astype(F64), shape, 1, padding),
                scales=T.conv2d_bwd_filter(ab(x), ab(dz), shape, 1, padding))


def normal_operands(entry, case, seed=73):
    n, h, w, c, k, r, s, pt, pl, ho, wo = P.shapes(entry, case)
    rng = np.random.default_rng(seed)
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
    return dict(x=draw(n, h, w, c), dz=draw(n, ho, wo, k), w=(draw(r, s, c, k) / np.sqrt(r * s * c)).astype(np.float32), bias=draw(k),
                mask=draw(n, h, w, c))


def padded_planes(u, planes, rows, cols):
    """u [planes][rows][cols] -> flat [planes][pad4 rows][pad4 cols], zeros in the padding"""
    out = np.zeros((planes, W1.pad4(rows), W1.pad4(cols)), F64)
    out[:, :rows, :cols] = u.reshape(planes, rows, cols)
    return out.ravel()


def prepared_reference(entry, case, wt):
    """the prepared form of the filter as the headers define it -> a check over the floats the call writes"""
    n, h, w, c, k, r, s, pt, pl, ho, wo = P.shapes(entry, case)
    if entry == 'prepare_fwd':                     # U = G g G^T, sixteen [c][k] matrices
        return Exact(padded_planes(W.filter_transform(wt), 16, c, k))
    if entry == 'prepare_bwd_data':                # taps flipped, channels swapped: sixteen [k][c] matrices
        return Exact(padded_planes(W.filter_transform(wt[::-1, ::-1].transpose(0, 1, 3, 2)), 16, k, c))
    g = W1.as_array(W1.G, F64)                     # U[xi][r][k][c] = sum_s G[xi][s] w[R-1-r][4-s][c][k]
    flipped = wt[::-1, ::-1].transpose(1, 0, 3, 2).astype(F64)      # [s][r][k][c]
    u, scale = np.einsum('xs,srkc->xrkc', g, flipped), np.einsum('xs,srkc->xrkc', np.abs(g), np.abs(flipped))
    pad = lambda a: np.concatenate([padded_planes(a[:, i], 8, k, c).reshape(8, 1, -1) for i in range(r)], axis=1).ravel()      # noqa: E731
    return Bounded(pad(u), pad(scale))


def prepared_filter(ops, d, wt, which):
    """(descriptor with A3D_HINT_W_PREPARED, the prepared form as float32 values) written on the grid by the library"""
    pf = ops.PreparedFilter(d, torch.device('cuda'), which)
    assert pf.ok
    pf.refresh(torch.from_numpy(np.ascontiguousarray(wt)).cuda())
    synchronize('prepare_filter')
    return pf.desc_prepared, pf.buf.view(torch.float32).cpu().numpy()


def build(ops, lib, entry, case, data=None, ref=True, act='relu'):
    """the Job of an entry on a case.  data: the operands (default: ternary for F(2x2,3x3), W1.operands for F(4,5)); ref: attach
    the host references (needs the default operands)"""
    e = P.ENTRIES[entry]
    if entry == 'momentum':
        return momentum_job(ops, lib, case)
    pool = None
    if 'pool' in entry:
        case, h2, w2, ldp = pool = case
    n, h, w, c, k, r, s, pt, pl, ho, wo = P.shapes(entry, case)
    fam = e.family
    padding = case[5] if fam == 'w' else case[6]
    ldx, ldy = case[-2] or c, case[-1] or k
    assert data is None or not ref
    if data is not None:
        hs = data
    elif ref:
        hs = host_w(case) if fam == 'w' else host_l(case)
    else:
        hs = P.ternary_operands(case) if fam == 'w' else dict(zip(('x', 'dz', 'w', 'mask'), W1.operands(case, 51)))
    prepared = 'U' in e.operands
    wname = 'U' if prepared else 'w'
    plain = ops.conv_desc(n, h, w, c, k, r, s, 1, padding, ldx=ldx, ldy=ldy)
    d = ops.conv_desc(n, h, w, c, k, r, s, 1, padding, ldx=ldx, ldy=ldy, precision='fp32w') if fam == 'w' else plain
    st = ops._stream
    pix, opix, taps = n * h * w, n * ho * wo, r * s * c
    x_in, dz_in, m_in = (hs['x'], pix, ldx, c), (hs['dz'], opix, ldy, k), (hs['mask'], pix, ldx, c)
    w_in = (hs['w'], taps, k, k)
    what = f'{entry} {P.case_id(pool or case)}'
    on = lambda make: make() if ref else None      # noqa: E731  (a reference only where one is wanted)
    if entry.startswith(('prepare', 'l_prepare')):
        fn = getattr(lib, e.cname)
        nbytes = getattr(lib, e.cname.replace('prepare_filter', 'prepared_filter_bytes'))(ctypes.byref(d))
        assert nbytes > 0 and nbytes % 4 == 0
        written = (16 if fam == 'w' else 8 * r) * W1.pad4(c) * W1.pad4(k)
        assert written * 4 <= nbytes < written * 4 + 256
        return Job(entry, what, lambda q, ws, nb: fn(ctypes.byref(d), q['w'].ptr, q['prepared'].ptr, nbytes, st()), None, dict(w=w_in),
                   dict(prepared=(1, nbytes // 4, written, on(lambda: prepared_reference(entry, case, hs['w'])))))
    D = d
    if prepared:
        which = {'fwd_prepared': 'fwd'}.get(entry, 'bwd_d' if fam == 'w' else 'bwd_d_wino1d')
        D, u = prepared_filter(ops, d, hs['w'], which)
        w_in = (u, 1, u.size, u.size)
    B = ctypes.byref(D)
    masked = 'mask' in e.operands
    keep = (hs['mask'] > 0) if masked else 1.0
    if entry.startswith('fwd'):
        a = ops.ACT[act]
        y_ref = on(lambda: Exact(hs['y']))
        return Job(entry, what, lambda q, ws, nb: lib.a3d_conv2d_fwd(B, q['x'].ptr, q[wname].ptr, q['bias'].ptr, q['y'].ptr, a, ws, nb, st()),
                   lambda: lib.a3d_conv2d_fwd_ws_bytes(B), {'x': x_in, wname: w_in, 'bias': (hs['bias'], 1, k, k)}, dict(y=(opix, ldy, k, y_ref)))
    if 'bwd_data' in entry:
        fn, qn = (lib.a3d_conv2d_bwd_data, lib.a3d_conv2d_bwd_data_ws_bytes) if fam == 'w' else (lib.a3dl_conv2d_bwd_data, lib.a3dl_conv2d_bwd_data_ws_bytes)
        dx_ref = on(lambda: (Exact(hs['dx'] * keep) if fam == 'w' else Bounded(hs['dx'] * keep, hs['dx_scale'] * keep)))
        inputs = {'dz': dz_in, wname: w_in, **({'mask': m_in} if masked else {})}
        return Job(entry, what, lambda q, ws, nb: fn(B, q['dz'].ptr, q[wname].ptr, q['dx'].ptr, q['mask'].ptr if masked else None, ws, nb, st()),
                   lambda: qn(B), inputs, dict(dx=(pix, ldx, c, dx_ref)))
    if 'bwd_filter' in entry:
        fn, qn = (lib.a3dwg_conv2d_bwd_filter, lib.a3dwg_conv2d_bwd_filter_ws_bytes) if fam == 'w' else (lib.a3dl_conv2d_bwd_filter, lib.a3dl_conv2d_bwd_filter_ws_bytes)
        P0 = ctypes.byref(plain)
        has_db = 'db' in e.operands
        if fam == 'w':
            dw_ref, db_ref = on(lambda: Exact(hs['dw'])), on(lambda: Exact(hs['db']))
        else:
            dw_ref, db_ref = (on(lambda: Bounded(hs['grads'][i], hs['scales'][i])) for i in (0, 1))
        outputs = dict(dw=(taps, k, k, dw_ref), **(dict(db=(1, k, k, db_ref)) if has_db else {}))
        return Job(entry, what, lambda q, ws, nb: fn(P0, q['x'].ptr, q['dz'].ptr, q['dw'].ptr, q['db'].ptr if has_db else None, ws, nb, st()),
                   lambda: qn(P0), dict(x=x_in, dz=dz_in), outputs)
    assert entry.startswith('wb')
    inputs = {'x': x_in, 'dz': dz_in, wname: w_in, **({'mask': m_in} if masked else {})}
    dx_out = (pix, ldx, c, on(lambda: Exact(hs['dx'] * keep)))
    if pool:
        arg, py = P.pool_operands(pool)
        inputs.update(argmax=(arg, pix, c, c), pool_y=(py, pix, ldp or c, c))
        dx_out = (n * h2 * w2, c, c, on(lambda: Exact(P.unpool(hs['dx'], arg, py, h2, w2))))

    def call(q, ws, nb):
        pp = None
        if pool:
            q['_pool'] = _lib().WinoBwdPool(q['argmax'].t.data_ptr(), q['pool_y'].t.data_ptr(), ldp or c, h2, w2)
            pp = ctypes.byref(q['_pool'])
        return lib.a3dwb_conv2d_bwd(B, q['x'].ptr, q['dz'].ptr, q[wname].ptr, q['dw'].ptr, q['db'].ptr, q['dx'].ptr,
                                    q['mask'].ptr if masked else None, pp, ws, nb, st())
    return Job(entry, what, call, lambda: lib.a3dwb_conv2d_bwd_ws_bytes(B, int(prepared), int(bool(pool))), inputs,
               dict(dw=(taps, k, k, on(lambda: Exact(hs['dw']))), db=(1, k, k, on(lambda: Exact(hs['db']))), dx=dx_out))


def _lib():
    from ann3depth_amd import _lib
    return _lib


def momentum_job(ops, lib, shape, lr=0.1, mu=0.9, scale=0.125):
    """var_w, accum_w, var_b and accum_b against the bits of a3d_dense_bwd_filter into a scratch gradient followed by
    a3do_momentum_apply on kernel and bias, as tests/test_gpu_momentum.py holds the launch"""
    m, k, n = shape
    rng = np.random.default_rng(74)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    x, dz, state = draw(m, k), draw(m, n), [draw(k, n), draw(k, n), draw(n), draw(n)]
    dev = lambda a: torch.from_numpy(a.copy()).cuda()      # noqa: E731
    var_w, acc_w, var_b, acc_b = (dev(a) for a in state)
    dw, db = torch.empty((k, n), device='cuda'), torch.empty(n, device='cuda')
    ops.dense_bwd_filter(dev(x), dev(dz), dw, db)
    ops.momentum_apply(var_w, acc_w, dw, lr, mu, scale)
    ops.momentum_apply(var_b, acc_b, db, lr, mu, scale)
    synchronize('the two-call form')
    want = [t.cpu().numpy() for t in (var_w, acc_w, var_b, acc_b)]
    call = lambda q, ws, nb: lib.a3do_dense_bwd_filter_momentum(m, k, n, q['x'].ptr, q['dz'].ptr, q['var_w'].ptr, q['accum_w'].ptr,      # noqa: E731
                                                                q['var_b'].ptr, q['accum_b'].ptr, lr, mu, scale, ops._stream())
    inout = {o: (a, r, n, n, Bits(wt)) for o, a, r, wt in zip(('var_w', 'accum_w', 'var_b', 'accum_b'), state, (k, k, 1, 1), want)}
    return Job('momentum', f'momentum {shape}', call, None, dict(x=(x, m, k, k), dz=(dz, m, n, n)), {}, inout)


# ---------------------------------------------------------------------------------------------------------------- B: the sweep
def named(operand, message):
    return re.search(P.NAMED_AS.get(operand, rf'\b{operand}\b'), message) is not None


def record_key(recs):
    return [(r.mode, r.m, r.n, r.k, r.splitk) for r in recs]


def sweep(lib, job):
    e = P.ENTRIES[job.entry]
    q = int(job.query()) if e.ws else 0
    assert not e.ws or q > 0
    base = None
    for label, offs, ws_off in P.sweep(job.entry):
        assert not FAULTED, f'not run: the device reported an error earlier ({FAULTED[0]})'
        what = f'{e.cname} {job.what} [{label}]'
        pl = job.place(offs)
        roomy = Workspace(max(q, ROOMY), ws_off)
        args = roomy.args if e.ws else (None, 0)
        rc, recs = launched(lib, lambda: job.call(pl, *args), what)
        LAUNCHES[0] += 1
        bad = P.refused_operands(job.entry, offs, ws_off)
        for o in job.inputs:
            assert pl[o].untouched(), f'{what}: input {o} was written'
        if rc != 0:
            err = _lib().last_error()
            assert rc == EINVAL, f'{what}: returned {rc}: {err}'
            assert bad, f'{what}: refused ({err}), but the headers allow this placement'
            assert any(named(o, err) for o in bad), f'{what}: the message "{err}" names none of {bad}'
            assert not recs, what
            for o in job.outputs:
                assert pl[o].holds_fill(), f'{what}: refused, yet {o} was written'
            for o in job.inout:
                assert pl[o].untouched(), f'{what}: refused, yet {o} was written'
            print(f'ROUTE | {e.cname} | {job.what} | {label} | {route(base[0]) if base else "-"} | refused: {err}')
            continue
        assert not bad, f'{what}: accepted, but the headers let the entry point refuse {bad}'
        worst = [job.results()[o][3].check(whole(pl[o], job.results()[o][2], f'{what} {o}'), f'{what} {o}') for o in job.results()]
        assert roomy.tail_untouched(), what
        windows = {o: pl[o].t.view(torch.int32).clone() for o in job.results()}
        if base is None:
            assert label == 'on-grid'
            base = (recs, windows)
        for o in windows:
            assert torch.equal(windows[o], base[1][o]), f'{what}: {o} differs from the on-grid launch'
        assert record_key(recs) == record_key(base[0]), f'{what}: {route(base[0])} -> {route(recs)}'
        worst = [v for v in worst if v is not None]
        print(f'ROUTE | {e.cname} | {job.what} | {label} | {route(base[0])} | {route(recs)}' + (f' | worst {max(worst):.4f} of its bound' if worst else ''))
    print(f'LAUNCHES | {LAUNCHES[0]}')


F23 = [(e, c) for e, v in P.ENTRIES.items() if v.family == 'w' for c in P.cases(e)]
F45 = [(e, c) for e, v in P.ENTRIES.items() if v.family == 'l' for c in P.cases(e)]
ids = lambda v: P.case_id(v) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize('entry,case', F23, ids=ids)
def test_placement_f23(ops, lib, entry, case):
    """F(2x2,3x3): forward (bias + ReLU), bwd-data, the filter gradient, the chain and its pool form, per-call and prepared filter,
    and the two prepare calls — ternary operands, the float64 oracle element for element"""
    sweep(lib, build(ops, lib, entry, case))


@pytest.mark.parametrize('entry,case', F45, ids=ids)
def test_placement_f45(ops, lib, entry, case):
    """F(4,5): bwd-data, the filter gradient and the prepare call under the two bounds of tests/test_wino1d_cpu.py"""
    sweep(lib, build(ops, lib, entry, case))


@pytest.mark.parametrize('shape', P.MOMENTUM, ids=str)
def test_placement_momentum(ops, lib, shape):
    """a3do_dense_bwd_filter_momentum: "the tensors need 4-byte alignment only" — the two-call form's bits at every placement"""
    sweep(lib, build(ops, lib, 'momentum', shape))


# ---------------------------------------------------------------------------------------------------------------- C: the dirty workspace
WS_ENTRIES = [e for e, v in P.ENTRIES.items() if v.ws]


def run_on(job, ws, nbytes, what):
    pl = job.place()
    rc = job.call(pl, ws, nbytes)
    synchronize(what)
    assert rc == 0, f'{what}: {rc}: {_lib().last_error()}'
    for o in job.inputs:
        assert pl[o].untouched(), f'{what}: input {o} was written'
    return job.bits(pl)


def dirty(nbytes):
    ws = Workspace(nbytes, 0)
    ws.buf[:nbytes] = 0xFF      # float32 NaN, every byte
    return ws


@pytest.mark.parametrize('entry', WS_ENTRIES)
def test_dirty_workspace(ops, lib, entry):
    """exactly the queried bytes, every one 0xFF: a plane, pad column or slab read before it is written shows as NaN"""
    for case in P.dirty_cases(entry):
        job = build(ops, lib, entry, case, ref=False)
        q = int(job.query())
        what = f'{job.what} on {q} dirty bytes'
        ws, n = ops._ws().get(q, torch.device('cuda'))
        want = run_on(job, ws, n, job.what)
        tight = dirty(q)
        got = run_on(job, *tight.args, what)
        assert tight.tail_untouched(), f'{what}: wrote past the bytes its query named'
        for o in want:
            assert torch.equal(got[o], want[o]), f'{what}: {o} differs from the call on the roomy workspace'


@pytest.mark.parametrize('entry', WS_ENTRIES)
def test_workspace_dirty_by_history(ops, lib, entry):
    """one workspace serves the largest case and then the smallest: what the larger call left behind must not reach the smaller"""
    jobs = [build(ops, lib, entry, case, ref=False) for case in P.dirty_cases(entry)]
    sizes = [int(j.query()) for j in jobs]
    large, small = jobs[sizes.index(max(sizes))], jobs[sizes.index(min(sizes))]
    assert large is not small and max(sizes) > min(sizes)
    ws = dirty(max(sizes))
    run_on(large, *ws.args, large.what)
    got = run_on(small, *ws.args, f'{small.what} after {large.what}')
    assert ws.tail_untouched()
    zeros = torch.zeros(min(sizes), dtype=torch.uint8, device='cuda')
    want = run_on(small, ctypes.c_void_p(zeros.data_ptr()), min(sizes), small.what)
    for o in want:
        assert torch.equal(got[o], want[o]), f'{small.what} after {large.what}: {o} differs from the call on fresh zeros'


# ---------------------------------------------------------------------------------------------------------------- D: non-finite inputs
RUNS = [(e, c, o) for e in P.NONFINITE_ENTRIES for c in P.nonfinite_cases(e) for o in P.plant_operands(e)]


@pytest.mark.parametrize('entry,case,operand', RUNS, ids=ids)
def test_nonfinite_inputs_stay_in_their_window(ops, lib, entry, case, operand):
    """no activation, no mask (fmaxf swallows a NaN): non-finite where P.nonfinite_sets says must, the clean run's bits where it
    says clean — other tiles, images, channels and filters"""
    data = normal_operands(entry, case)
    clean_job = build(ops, lib, entry, case, data=data, ref=False, act=None)
    q = int(clean_job.query())
    ws, nb = ops._ws().get(q, torch.device('cuda'))
    clean = run_on(clean_job, ws, nb, clean_job.what)
    outs = clean_job.results()

    def array(bits, o, pl):
        rows, ld, cols, _ = outs[o]
        win = bits[o][pl[o].front:pl[o].front + rows * ld].view(rows, ld)[:, :cols]
        return win.cpu().numpy()
    probe = clean_job.place()
    for run in P.plants(entry, case, operand):
        sets = P.nonfinite_sets(entry, case, run)
        assert set(sets) == set(outs) and P.clean_share(sets) >= P.CLEAN_SHARE
        planted = {name: a.copy() for name, a in data.items()}
        for op, image, py, px, ch, value in run:
            planted[op][image, py, px, ch] = value
        job = build(ops, lib, entry, case, data=planted, ref=False, act=None)
        got = run_on(job, ws, nb, f'{job.what} {run}')
        for o, (must, may, keep) in sets.items():
            a, b = array(got, o, probe).reshape(must.shape), array(clean, o, probe).reshape(must.shape)
            finite = np.isfinite(a.view(np.float32))
            assert np.isfinite(b.view(np.float32)).all()
            assert not finite[must].any(), f'{job.what} {run}: {int(finite[must].sum())} outputs of {o} the element reaches are finite'
            leaked = keep & (a != b)
            assert not leaked.any(), f'{job.what} {run}: {o} changed outside the windows that hold the element at {np.argwhere(leaked)[:4].tolist()}'
            # around the tensor and in the pad columns nothing moved either
            outside = got[o].clone()
            rows, ld, cols, _ = outs[o]
            outside[probe[o].front:probe[o].front + rows * ld].view(rows, ld)[:, :cols] = 0
            inside = clean[o].clone()
            inside[probe[o].front:probe[o].front + rows * ld].view(rows, ld)[:, :cols] = 0
            assert torch.equal(outside, inside), f'{job.what} {run}: {o} written outside its window'
