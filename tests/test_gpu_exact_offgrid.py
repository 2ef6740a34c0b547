"""Every conv / dense entry point with its operands OFF the 16-byte grid, element by element.

The front end (csrc/igemm_host.hip) routes a call partly by `address & 15` of its operands: vector or scalar gathers, 16- / 8-byte
window runs, the LDS-DMA kernels, fewch / conv3 / the stencils, the vectorised split-K reduction.  torch's own allocations are
256-byte aligned, so the other tests only ever run the on-grid half of those decisions.  Here every pointer operand is carved
out of a larger allocation (NaN everywhere, bf16 NaN, argmax / keep bytes 9; 64 elements of guard in front, 67 guard rows
behind) so that it starts a chosen number of bytes past a 256-byte boundary — the helper asserts the address, a test can never
silently run on-grid — and the exact-integer cases of tests/exact_ops.py are swept per entry point (E.offgrid_sweep): each
operand alone at +4 bytes, the image-side operand at +8, all operands together (float32 +12, bf16 +2, uint8 +1), the workspace
at +16 and +4.

A launch either
  * is accepted: every output equals the float64 integer reference over its WHOLE allocation, inputs are bit for bit what they
    were, the timing record shows the route the code says an off-grid operand takes (avec / bvec 1, no LDS-DMA kernel, off fewch
    where x is off the grid; the same family where the kernel takes any 4-byte address), a `bf16` / `bf16x3` request is held
    to the reference of the arithmetic the record names (wide operands: the three differ), and the same call on EXACTLY the
    *_ws_bytes answer returns 0 too, leaves the 4096 bytes behind it alone and gives the same bits; or
  * is refused: A3D_EINVAL, a3d_last_error names the operand, every output still holds its fill — and the pair (entry point,
    operand) is in E.REFUSED, which is written from include/a3d.h's alignment paragraph.  A refusal outside that table fails, and
    so does an acceptance of something inside it.
Each accepted placement prints one `ROUTE |` line (entry, case, placement, on-grid route, off-grid route)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import exact_ops as E

pytestmark = pytest.mark.gpu

NAN = float('nan')
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
DTYPE = {'f32': F32, 'bf16': BF, 'u8': U8}
BITS = {F32: torch.int32, BF: torch.int16, U8: torch.uint8, torch.int32: torch.int32}
EINVAL, EWORKSPACE = -1, -2
FRONT, GUARD_ROWS = 64, 67
TAIL, FILL = 4096, 0xA5
ROOMY = 1 << 20          # ops.Workspace's smallest allocation
CONV3, FEWCH = (0, 2), (0, 4)
LAUNCHES = [0]
FAULTED = []            # a device error ends the module: nothing more is launched on a GPU that has faulted


@pytest.fixture(scope='module')
def ops():
    from ann3depth_amd import ops
    return ops


class Placed:
    """`rows` rows of pitch `ld` inside a larger allocation of the fill, starting `off` BYTES past a 256-byte boundary: FRONT
    elements (or more: up to that boundary) of guard in front, GUARD_ROWS rows behind.  data: [rows, cols] written into the view."""

    def __init__(self, rows, ld, off, typ='f32', data=None, cols=None):
        self.dtype = dtype = DTYPE[typ]
        esz = E.ELEMENT_BYTES[typ]
        assert off % esz == 0 and 0 <= off < 256
        self.fill = 9 if dtype == U8 else NAN
        front = (-(-FRONT * esz // 256) * 256 + off) // esz
        self.big = torch.full((front + (rows + GUARD_ROWS) * ld,), self.fill, dtype=dtype, device='cuda')
        self.front, self.rows, self.ld, self.off = front, rows, ld, off
        self.t = self.big[front:front + rows * ld]
        p = self.t.data_ptr()
        assert self.big.data_ptr() % 256 == 0 and front >= FRONT
        assert p & 15 == off & 15 and (p - off) % 256 == 0, f'operand at {p:#x}, wanted {off} bytes past a 256-byte boundary'
        self.before = None
        if data is not None:
            cols = ld if cols is None else cols
            d = torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint8 if dtype == U8 else np.float32).reshape(rows, cols)).cuda()
            self.t.view(rows, ld)[:, :cols] = d.to(dtype)
            self.before = self.bits()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def bits(self):
        return self.big.view(BITS[self.dtype]).clone()

    def untouched(self):
        return torch.equal(self.big.view(BITS[self.dtype]), self.before)

    def holds_fill(self):
        a = self.big.cpu().numpy() if self.dtype == U8 else self.big.float().cpu().numpy()
        return bool((a == 9).all() if self.dtype == U8 else np.isnan(a).all())

    def expect(self, ref, cols, what):
        """the WHOLE allocation: `ref` in the view's first `cols` columns, the fill everywhere else"""
        want = np.full((self.big.numel(),), 9.0 if self.dtype == U8 else np.nan, np.float64)
        win = want[self.front:self.front + self.rows * self.ld].reshape(self.rows, self.ld)
        win[:, :cols] = np.asarray(ref, np.float64).reshape(self.rows, cols)
        got = self.big.cpu().numpy().astype(np.float64) if self.dtype == U8 else self.big.float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(got, want, err_msg=what)


class Workspace:
    """nbytes of 0xA5 starting `off` bytes past a 256-byte boundary, TAIL more bytes behind them"""

    def __init__(self, nbytes, off):
        self.nbytes, self.off = int(nbytes), off
        self.buf = torch.full((off + self.nbytes + TAIL,), FILL, dtype=U8, device='cuda')
        assert self.buf.data_ptr() % 256 == 0

    @property
    def args(self):
        """(ws, ws_bytes); a query that answers 0 is served by (NULL, 0) while the workspace is on the grid"""
        if self.nbytes == 0 and self.off == 0:
            return None, 0
        return ctypes.c_void_p(self.buf.data_ptr() + self.off), self.nbytes

    def tail_untouched(self):
        return bool((self.buf[self.off + self.nbytes:] == FILL).all()) and bool((self.buf[:self.off] == FILL).all())


class Job:
    """One entry point on one case.  inputs: {operand: (data, rows, ld, cols)}; outputs: {operand: (rows, ld, cols, ref)} with ref an
    array, or {prec: array} where the arithmetic the record names decides; inout: {operand: (data, rows, ld, cols, ref)}.
    kind: 'fwd' | 'bwd_d' | 'bwd_f' | None (no GEMM behind it); A, B: the operands the GEMM gathers; plain: the GEMM axis whose
    padding shows a window-run form (forward: K, filter gradient: M)."""

    def __init__(self, entry, what, call, query, inputs, outputs, types=None, inout=None, kind=None, A=None, B=None, plain=0,
                 precision=0, has_ws=True, storage=0):
        self.entry, self.what, self.call, self.query = entry, what, call, query
        self.inputs, self.outputs, self.inout, self.types = inputs, outputs, inout or {}, types or {}
        self.kind, self.A, self.B, self.plain, self.precision, self.has_ws, self.storage = kind, A, B, plain, precision, has_ws, storage
        assert set(inputs) | set(outputs) | set(self.inout) == set(E.OFFGRID_ENTRIES[entry][1]), (entry, sorted(inputs), sorted(outputs))

    def place(self, offs):
        P = {}
        for o, (data, rows, ld, cols) in self.inputs.items():
            P[o] = Placed(rows, ld, offs.get(o, 0), E.operand_type(o, self.types), data, cols)
        for o, (rows, ld, cols, ref) in self.outputs.items():
            P[o] = Placed(rows, ld, offs.get(o, 0), E.operand_type(o, self.types))
        for o, (data, rows, ld, cols, ref) in self.inout.items():
            P[o] = Placed(rows, ld, offs.get(o, 0), E.operand_type(o, self.types), data, cols)
        return P

    def results(self):
        return {**self.outputs, **{o: v[1:] for o, v in self.inout.items()}}


def synchronize(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        FAULTED.append(f'{what}: {e}')
        raise


def launched(lib, fn, what=''):
    """runs fn with every launch bracketed -> (its return value, its timing records)"""
    from ann3depth_amd import _lib
    lib.a3d_timing_select(None)
    lib.a3d_timing_enable(1)
    try:
        rc = fn()
        synchronize(what)
    finally:
        lib.a3d_timing_enable(0)
    arr = (_lib.TimingRecord * 64)()
    return rc, [arr[i] for i in range(lib.a3d_timing_collect(arr, 64))]


def route(recs):
    """the launches of a call as the record shows them; none: the stencils and dense.hip's streaming kernels carry no record"""
    if not recs:
        return 'no record'
    fam = {(0, 1): 'igemm-glds', (0, 2): 'conv3', (2, 2): 'conv3b', (0, 4): 'fewch', (2, 4): 'fewch16', (2, 3): 'ring'}
    return ' + '.join(sorted({f'{fam.get((r.prec, r.lds_dma), "igemm" + ("", "-bf16x3", "-bf16")[r.prec])} {r.bm}x{r.bn} a{r.avec} b{r.bvec}'
                              f' M{r.m}' + (f' split{r.splitk}' if r.splitk > 1 else '') for r in recs}))


def families(recs):
    return {(r.prec, r.lds_dma) for r in recs}


def check_route(job, label, offs, recs, base):
    """the off-grid launch left the on-grid route where the code says it does, and stayed on it where the kernel takes any address"""
    what = f'{job.what} {label}: {route(base)} -> {route(recs)}'
    for r in recs:
        assert r.prec in (job.precision, 0), what
        assert r.prec == 0 or (r.avec == 4 and r.bvec == 4) or r.lds_dma in (2, 4), what      # bf16 arithmetic takes 16-byte operands only
    if job.kind is None or not base:
        return
    a_off, b_off = job.A in offs, job.B in offs
    if families(base) == {CONV3}:                  # conv3.hip gathers x float by float and repacks w: any 4-byte address
        assert families(recs) == {CONV3}, what
    elif families(base) == {FEWCH}:
        if 'x' in offs:                            # fewch stages rows of x in 16-byte pieces: the generic kernel's window runs take over
            assert recs and FEWCH not in families(recs), what
            for r in recs:
                assert r.avec == 2 and r.m != job.plain, what      # 8-byte runs from any 4-byte address, the padded filter gradient
        else:
            assert families(recs) == {FEWCH}, what
    else:
        assert recs, what
        for r in recs:
            run = (r.k if job.kind == 'fwd' else r.m) != job.plain and job.kind != 'bwd_d'
            if a_off:
                assert r.avec == 1 or (run and r.avec == 2 and (offs[job.A] % 8 == 0 or job.kind == 'bwd_f')), what
            if b_off:
                assert r.bvec == 1 or (run and job.kind == 'fwd'), what      # the forward's padded filter copy lies in the workspace
            if a_off or b_off:
                assert r.lds_dma == 0 and r.prec == 0, what
        if not a_off and not b_off and not job.storage:
            assert route(recs) == route(base), what


def sweep(lib, job):
    from ann3depth_amd import _lib
    cname = E.OFFGRID_ENTRIES[job.entry][0]
    q = int(job.query()) if job.has_ws else 0
    base = None
    assert not FAULTED, f'not run: the device reported an error earlier ({FAULTED[0]})'
    for label, offs, ws_off in E.offgrid_sweep(job.entry, job.types, ws=job.has_ws):
        what = f'{cname} {job.what} [{label}]'
        P = job.place(offs)
        roomy = Workspace(max(q, ROOMY), ws_off)
        rc, recs = launched(lib, lambda: job.call(P, *roomy.args), what)
        LAUNCHES[0] += 1
        bad = E.refused_operands(job.entry, offs, ws_off, job.types)
        for o in job.inputs:
            assert P[o].untouched(), f'{what}: input {o} was written'
        if rc != 0:
            err = _lib.last_error()
            assert rc == EINVAL, f'{what}: returned {rc}: {err}'
            assert bad, f'{what}: refused ({err}), but include/a3d.h allows this placement'
            assert any(re.search(rf'\b{o}\b', err) for o in bad), f'{what}: the message "{err}" names none of {bad}'
            assert not recs, what
            for o in job.outputs:
                assert P[o].holds_fill(), f'{what}: refused, yet {o} was written'
            for o in job.inout:
                assert P[o].untouched(), f'{what}: refused, yet {o} was written'
            print(f'ROUTE | {cname} | {job.what} | {label} | {route(base)} | refused: {err}')
            continue
        assert not bad, f'{what}: accepted, but include/a3d.h lets the entry point refuse {bad}'
        if base is None:
            assert label == 'on-grid'
            base = recs
        precs = {r.prec for r in recs} or {0}
        assert len(precs) == 1, what
        for o, (rows, ld, cols, ref) in job.results().items():
            P[o].expect(ref[precs.copy().pop()] if isinstance(ref, dict) else ref, cols, f'{what} {o}')
        assert roomy.tail_untouched(), what
        check_route(job, label, offs, recs, base)
        print(f'ROUTE | {cname} | {job.what} | {label} | {route(base)} | {route(recs)}')
        if not job.has_ws:
            continue
        # the same call on EXACTLY the bytes the query names
        P2 = job.place(offs)
        tight = Workspace(q, ws_off)
        rc2 = job.call(P2, *tight.args)
        synchronize(what)
        LAUNCHES[0] += 1
        assert rc2 != EWORKSPACE, f'{what}: the query answers {q} bytes, the launch wants more: {_lib.last_error()}'
        assert rc2 == 0, f'{what} on {q} workspace bytes: {rc2}: {_lib.last_error()}'
        assert tight.tail_untouched(), f'{what}: wrote past the {q} bytes its query named'
        for o in job.results():
            assert torch.equal(P2[o].bits(), P[o].bits()), f'{what}: {o} differs between the roomy and the exact workspace'
    print(f'LAUNCHES | {LAUNCHES[0]}')


# ---------------------------------------------------------------------------------------------------------------- conv jobs
def conv_job(ops, lib, entry, case, precision='fp32', stored=False, ld=None, cs=None, refs=None, tag=''):
    """refs: {prec: ConvCase view} for bf16 arithmetic on float32 tensors"""
    n, h, w, c, k, ks, st, pad = case
    cs = cs or E.conv_case(*case)
    refs = refs or {0: cs}
    S = ops.STORE_X | ops.STORE_W | ops.STORE_Y
    storage = {False: 0, 'conv2d_fwd': S, 'conv2d_bwd_data': S, 'conv2d_bwd_data_mask': S, 'conv2d_bwd_filter': ops.STORE_X | ops.STORE_Y,
               'conv2d_bwd_filter_db': ops.STORE_X | ops.STORE_Y}[stored and entry]
    d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, ldy=ld, precision=precision, storage=storage)
    D, ldy, act = ctypes.byref(d), d.ldy, ops.ACT['relu']
    assert (d.ho, d.wo) == (cs.ho, cs.wo)
    pix, opix, taps = n * h * w, n * cs.ho * cs.wo, ks * ks * c
    s = ops._stream
    by = lambda f: {p: f(v) for p, v in refs.items()} if len(refs) > 1 else f(refs[0])
    b16 = lambda *names: {o: 'bf16' for o in names} if stored else {}
    common = dict(precision=ops.PREC[precision], storage=storage)
    what = f'{case}' + (f' {precision}' if precision != 'fp32' else '') + (' bf16 tensors' if stored else '') + tag
    x_in, w_in, b_in, dz_in = (cs.x, pix, c, c), (cs.w, taps, k, k), (cs.b, 1, k, k), (cs.dz, opix, k, k)
    if entry == 'conv2d_fwd':
        return Job(entry, what, lambda P, ws, nb: lib.a3d_conv2d_fwd(D, P['x'].ptr, P['w'].ptr, P['bias'].ptr, P['y'].ptr, act, ws, nb, s()),
                   lambda: lib.a3d_conv2d_fwd_ws_bytes(D), dict(x=x_in, w=w_in, bias=b_in),
                   dict(y=(opix, ldy, k, by(lambda v: np.maximum(v.y, 0)))), b16('x', 'w', 'y'), kind='fwd', A='x', B='w', plain=taps, **common)
    if entry == 'conv2d_pool_fwd':
        prow = n * (cs.ho // 2) * (cs.wo // 2)
        pooled, arg = E.pool_reference(np.maximum(cs.y, 0))
        return Job(entry, what, lambda P, ws, nb: lib.a3d_conv2d_pool_fwd(D, P['x'].ptr, P['w'].ptr, P['bias'].ptr, P['y'].ptr, ldy,
                                                                         P['argmax'].ptr, act, ws, nb, s()),
                   lambda: lib.a3d_conv2d_fwd_ws_bytes(D), dict(x=x_in, w=w_in, bias=b_in),
                   dict(y=(prow, ldy, k, pooled), argmax=(prow, k, k, arg)), kind='fwd', A='x', B='w', plain=taps, **common)
    if entry in ('conv2d_bwd_data', 'conv2d_bwd_data_mask'):
        mask = entry.endswith('mask')
        inputs = dict(dz=dz_in, w=w_in, **(dict(mask=(cs.x, pix, c, c)) if mask else {}))
        return Job(entry, what, lambda P, ws, nb: lib.a3d_conv2d_bwd_data(D, P['dz'].ptr, P['w'].ptr, P['dx'].ptr,
                                                                         P['mask'].ptr if mask else None, ws, nb, s()),
                   lambda: lib.a3d_conv2d_bwd_data_ws_bytes(D), inputs,
                   dict(dx=(pix, c, c, by(lambda v: v.dx * (cs.x > 0) if mask else v.dx))), b16('dz', 'w', 'dx', 'mask'),
                   kind='bwd_d', A='dz', B='w', **common)
    assert entry in ('conv2d_bwd_filter', 'conv2d_bwd_filter_db')
    db = entry.endswith('db')
    outputs = dict(dw=(taps, k, k, by(lambda v: v.dw)), **(dict(db=(1, k, k, cs.db)) if db else {}))
    return Job(entry, what, lambda P, ws, nb: lib.a3d_conv2d_bwd_filter(D, P['x'].ptr, P['dz'].ptr, P['dw'].ptr, P['db'].ptr if db else None,
                                                                       ws, nb, s()),
               lambda: lib.a3d_conv2d_bwd_filter_ws_bytes(D), dict(x=x_in, dz=dz_in), outputs, b16('x', 'dz'),
               kind='bwd_f', A='x', B='dz', plain=taps, **common)


CONV_ENTRIES = ('conv2d_fwd', 'conv2d_bwd_data', 'conv2d_bwd_data_mask', 'conv2d_bwd_filter', 'conv2d_bwd_filter_db')


@pytest.mark.parametrize('entry', CONV_ENTRIES)
@pytest.mark.parametrize('case', E.OFFGRID_GENERIC + E.OFFGRID_STRIDED + E.OFFGRID_FEW_CHANNEL, ids=str)
def test_conv_fp32(ops, lib, case, entry):
    """generic fp32 GEMM at vec4-capable shapes, strided bwd-data as one launch, conv3 / window runs / fewch"""
    sweep(lib, conv_job(ops, lib, entry, case))


def lds_dma_forward_case(ops, lib):
    """the smallest E.GENERIC case whose on-grid forward record has lds_dma == 1 (igemm_glds.h)"""
    for case in sorted(E.OFFGRID_GLDS_FROM, key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4] * c[5] ** 2):
        n, h, w, c, k, ks, st, pad = case
        d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad)
        x, wt = torch.zeros((n, h, w, c), device='cuda'), torch.zeros((ks, ks, c, k), device='cuda')
        y = torch.empty((n, d.ho, d.wo, k), device='cuda')
        _, recs = launched(lib, lambda: ops.conv2d_fwd(d, x, wt, None, y, 'relu') is None)
        if recs and all(r.lds_dma == 1 and r.prec == 0 for r in recs):
            return case
    return None


def test_forward_on_the_lds_dma_staged_kernel():
    """igemm_glds.h stages its tiles with 16-byte global_load_lds and has no scalar-gather form: an x or w off the grid must run
    the register-staged twin (needs_twin, igemm_plan.cc).  The shipped planner never gives a forward to that kernel on its own
    (igemm_cfgs.h rates configurations 9 / 10 at 1.10 / 1.00 against 1.15 / 1.05 for their twins 7 / 8, so the cost model always
    prefers the twin: no E.GENERIC case, nor any other, has an on-grid record with lds_dma == 1), so the route is reached the way
    tests/exact_forced_worker.py reaches it: a child process with A3D_TUNING=1 and configuration 9 pinned.  There the worker takes
    the smallest E.GENERIC case whose on-grid record has lds_dma == 1, asserts that, sweeps it and the multi-tile case of
    E.OFFGRID_GENERIC, and this test asserts from the printed routes that every placement with x or w off the grid has 0."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    env.update(A3D_TUNING='1', A3D_FORCE_CFG='9')
    r = subprocess.run([sys.executable, os.path.join(root, 'tests', 'offgrid_glds_worker.py')], env=env, capture_output=True, text=True,
                       timeout=300, cwd=root)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln.split(' | ') for ln in r.stdout.splitlines() if ln.startswith('ROUTE |')]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith('verified ')]
    assert len(done) == 2 and lines, r.stdout[-2000:]
    LAUNCHES[0] += int([ln for ln in r.stdout.splitlines() if ln.startswith('LAUNCHES |')][-1].split(' | ')[1])
    for _, cname, what, label, base, got in lines:
        assert 'igemm-glds' in base, (what, label, base)
        assert got.startswith('refused') == (label == 'ws+4'), (what, label, got)
        assert got.startswith('refused') or ('igemm-glds' in got) == (label not in ('x+4', 'w+4', 'x+8', 'all')), (what, label, got)


@pytest.mark.parametrize('case', E.OFFGRID_POOL, ids=str)
def test_fused_pool_with_argmax(ops, lib, case):
    ld = {4: 12, 200: 208, 63: 64}[case[4]]      # the GUARD cases' pitches; the 63 filters in 16-byte rows
    sweep(lib, conv_job(ops, lib, 'conv2d_pool_fwd', case, ld=ld))


@pytest.mark.parametrize('entry', ('conv2d_fwd', 'conv2d_bwd_data_mask', 'conv2d_bwd_filter_db'))
@pytest.mark.parametrize('case', E.OFFGRID_BF16_STORED, ids=str)
def test_conv_on_bf16_stored_tensors(ops, lib, case, entry):
    """a bf16 tensor off the 16-byte grid is refused; the float32 operands beside it (bias, dw, db) may lie anywhere"""
    sweep(lib, conv_job(ops, lib, entry, case, precision='bf16', stored=True, cs=E.conv_case(*case).bf16('y', 'dx')))


# (direction, the operands it reads): each wide operand in each direction that reads it
ARITH_READS = [('conv2d_fwd', 'x'), ('conv2d_fwd', 'w'), ('conv2d_bwd_data', 'dz'), ('conv2d_bwd_data', 'w'), ('conv2d_bwd_filter_db', 'x'),
               ('conv2d_bwd_filter_db', 'dz')]


@pytest.mark.parametrize('precision', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('entry,wide', ARITH_READS)
@pytest.mark.parametrize('case', E.OFFGRID_BF16_ARITH, ids=str)
def test_bf16_arithmetic_on_float32_tensors(ops, lib, case, entry, wide, precision):
    """an off-grid float32 operand runs the request in fp32: never less exact than asked, and the record says so"""
    cs = dict(E.wide_variants(case))[wide]
    sweep(lib, conv_job(ops, lib, entry, case, precision=precision, cs=cs, refs={0: cs, 1: cs.arith_bf16x3, 2: cs.arith_bf16},
                        tag=f' {wide} wide'))


# ---------------------------------------------------------------------------------------------------------------- few-channel, stencil
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', E.OFFGRID_POOLED_BWDF, ids=str)
def test_filter_gradient_from_the_pooled_map(ops, lib, case, dtype):
    cs = E.pooled_bwdf_case(*case)
    n, h, w, c, k, ks, st, ld, lda = case
    d = ops.conv_desc(n, h, w, c, k, ks, ks, st, 'VALID')
    D = ctypes.byref(d)
    prow, taps = n * (cs.ho // 2) * (cs.wo // 2), ks * ks * c
    call = lambda P, ws, nb: lib.a3d_conv2d_bwd_filter_pooled(D, P['x'].ptr, P['dpool'].ptr, ld, P['pooled'].ptr, P['argmax'].ptr, lda,
                                                              int(dtype == 'bf16'), P['dw'].ptr, P['db'].ptr, ws, nb, ops._stream())
    sweep(lib, Job('conv2d_bwd_filter_pooled', f'{case} {dtype} pooled tensors', call, lambda: lib.a3d_conv2d_bwd_filter_pooled_ws_bytes(D),
                   dict(x=(cs.x, n * h * w, c, c), dpool=(cs.dpool, prow, ld, ld), pooled=(cs.pooled, prow, ld, ld),
                        argmax=(cs.arg, prow, lda, lda)),
                   dict(dw=(taps, k, k, cs.dw), db=(1, k, k, cs.db)), {'dpool': dtype, 'pooled': dtype}, kind='bwd_f', A='x', B='dpool',
                   plain=taps))


@pytest.mark.parametrize('dx16', [False, True], ids=['f32-dx', 'bf16-dx'])
@pytest.mark.parametrize('case', E.OFFGRID_BOTH, ids=str)
def test_one_filter_backward_in_one_pass(ops, lib, case, dx16):
    cs = E.both_case(*case)
    n, h, w, c, pad, ldx, lddx = case
    d = ops.conv_desc(n, h, w, c, 1, 5, 5, 1, pad, ldx=ldx)
    D = ctypes.byref(d)
    opix = cs.y.shape[0] * cs.y.shape[1] * cs.y.shape[2]
    state = torch.zeros(64, dtype=torch.int32, device='cuda')

    def call(P, ws, nb):
        rc = lib.a3d_conv2d_bwd_both(D, P['x'].ptr, P['dz'].ptr, P['w'].ptr, P['dw'].ptr, P['db'].ptr, P['dx'].ptr, lddx, int(dx16), 1,
                                     ctypes.c_void_p(state.data_ptr()), ws, nb, ops._stream())
        assert not state.any(), 'the arrival counters did not come back to zero'
        return rc
    sweep(lib, Job('conv2d_bwd_both', f'{case} {"bf16" if dx16 else "f32"} dx', call, lambda: lib.a3d_conv2d_bwd_both_ws_bytes(D),
                   dict(x=(cs.xbuf, n * h * w, ldx, ldx), dz=(cs.dz, opix, 1, 1), w=(cs.w, 25 * c, 1, 1)),
                   dict(dw=(25 * c, 1, 1, cs.dw), db=(1, 1, 1, cs.db), dx=(n * h * w, lddx, c, cs.dx * (cs.x > 0))),
                   {'dx': 'bf16'} if dx16 else {}))


def stencil_job(ops, lib, entry, case):
    cs = E.both_case(*case)
    n, h, w, c, pad, ldx, lddx = case
    d = ops.conv_desc(n, h, w, c, 1, 5, 5, 1, pad, ldx=ldx)
    D = ctypes.byref(d)
    opix = cs.y.shape[0] * cs.y.shape[1] * cs.y.shape[2]
    x_in, w_in = (cs.xbuf, n * h * w, ldx, ldx), (cs.w, 25 * c, 1, 1)
    if entry == 'conv2d_fwd':
        return Job(entry, f'{case} one filter', lambda P, ws, nb: lib.a3d_conv2d_fwd(D, P['x'].ptr, P['w'].ptr, P['bias'].ptr, P['y'].ptr,
                                                                                    ops.ACT['relu'], ws, nb, ops._stream()),
                   lambda: lib.a3d_conv2d_fwd_ws_bytes(D), dict(x=x_in, w=w_in, bias=(cs.b, 1, 1, 1)),
                   dict(y=(opix, 1, 1, np.maximum(cs.y, 0))))
    return Job(entry, f'{case} one filter', lambda P, ws, nb: lib.a3d_conv2d_bwd_filter(D, P['x'].ptr, P['dz'].ptr, P['dw'].ptr, P['db'].ptr,
                                                                                       ws, nb, ops._stream()),
               lambda: lib.a3d_conv2d_bwd_filter_ws_bytes(D), dict(x=x_in, dz=(cs.dz, opix, 1, 1)),
               dict(dw=(25 * c, 1, 1, cs.dw), db=(1, 1, 1, cs.db)))


@pytest.mark.parametrize('entry,case', [('conv2d_fwd', c) for c in E.OFFGRID_BOTH_FWD] + [('conv2d_bwd_filter_db', c) for c in E.OFFGRID_BOTH_BWD_F],
                         ids=str)
def test_one_filter_stencils(ops, lib, entry, case):
    """the MFMA stencil wants x and w on the grid, the lane-per-channel one takes any address: no record, equality is the check"""
    sweep(lib, stencil_job(ops, lib, entry, case))


# ---------------------------------------------------------------------------------------------------------------- dense
def dense_job(ops, lib, entry, shape, stored=False):
    m, k, n = shape
    cs = E.dense_case(m, k, n)
    s, relu = ops._stream, ops.ACT['relu']
    what = f'{shape}' + (' bf16 tensors' if stored else '')
    x_in, w_in, dz_in = (cs.x, m, k, k), (cs.w, k, n, n), (cs.dz, m, n, n)
    if entry in ('dense_fwd', 'dense_fwd_ex'):
        if stored:
            cs.bf16()
            st = ops.STORE_W | ops.STORE_X
            d = ops.conv_desc(m, 1, 1, k, n, 1, 1, 1, 'VALID', precision='bf16', storage=st)
            call = lambda P, ws, nb: lib.a3d_dense_fwd_ex(m, k, n, P['x'].ptr, P['w'].ptr, P['bias'].ptr, P['y'].ptr, relu,
                                                          P['drop_keep'].ptr, 2, st, ws, nb, s())
            query = lambda: max(lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(d)), lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(d)))
        else:
            call = lambda P, ws, nb: lib.a3d_dense_fwd(m, k, n, P['x'].ptr, P['w'].ptr, P['bias'].ptr, P['y'].ptr, relu, P['drop_keep'].ptr,
                                                       ws, nb, s())
            query = lambda: lib.a3d_dense_fwd_ws_bytes(m, k, n)
        return Job(entry, what, call, query, dict(x=x_in, w=w_in, bias=(cs.b, 1, n, n), drop_keep=(cs.keep, m, n, n)),
                   dict(y=(m, n, n, 2.0 * np.maximum(cs.y, 0) * cs.keep)), {'x': 'bf16', 'w': 'bf16'} if stored else {},
                   kind='fwd', A='x', B='w', plain=k, precision=2 if stored else 0, storage=int(stored))
    if entry in ('dense_bwd_data', 'dense_bwd_data_ex'):
        if stored:
            cs.bf16()
            st = ops.STORE_W | ops.STORE_X | ops.STORE_Y
            d = ops.conv_desc(m, 1, 1, k, n, 1, 1, 1, 'VALID', precision='bf16', storage=st)
            call = lambda P, ws, nb: lib.a3d_dense_bwd_data_ex(m, k, n, P['dz'].ptr, P['w'].ptr, P['dx'].ptr, P['mask'].ptr, relu, 2.0, 2, st,
                                                               ws, nb, s())
            query = lambda: max(lib.a3d_conv2d_fwd_ws_bytes(ctypes.byref(d)), lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(d)))
        else:
            call = lambda P, ws, nb: lib.a3d_dense_bwd_data(m, k, n, P['dz'].ptr, P['w'].ptr, P['dx'].ptr, P['mask'].ptr, relu, 2.0, ws, nb, s())
            query = lambda: lib.a3d_dense_bwd_data_ws_bytes(m, k, n)
        return Job(entry, what, call, query, dict(dz=dz_in, w=w_in, mask=x_in), dict(dx=(m, k, k, 2.0 * cs.dx * (cs.x > 0))),
                   {o: 'bf16' for o in ('dz', 'w', 'dx', 'mask')} if stored else {}, kind='bwd_d', A='dz', B='w',
                   precision=2 if stored else 0, storage=int(stored))
    assert entry == 'dense_bwd_filter'
    return Job(entry, what, lambda P, ws, nb: lib.a3d_dense_bwd_filter(m, k, n, P['x'].ptr, P['dz'].ptr, P['dw'].ptr, P['db'].ptr, ws, nb, s()),
               lambda: lib.a3d_dense_bwd_filter_ws_bytes(m, k, n), dict(x=x_in, dz=dz_in), dict(dw=(k, n, n, cs.dw), db=(1, n, n, cs.db)),
               kind='bwd_f', A='x', B='dz', plain=k)


@pytest.mark.parametrize('entry', ('dense_fwd', 'dense_bwd_data', 'dense_bwd_filter'))
@pytest.mark.parametrize('shape', E.OFFGRID_DENSE, ids=str)
def test_dense_fp32(ops, lib, shape, entry):
    """relu + dropout, bwd-data with mask and scale 2, the filter gradient; (5, 1028, 1031): dense.hip's streaming forward on-grid,
    the generic plan behind it for an x off the grid"""
    sweep(lib, dense_job(ops, lib, entry, shape))


@pytest.mark.parametrize('entry', ('dense_fwd_ex', 'dense_bwd_data_ex'))
@pytest.mark.parametrize('shape', E.OFFGRID_DENSE_BF16, ids=str)
def test_dense_ex_on_bf16_tensors(ops, lib, shape, entry):
    sweep(lib, dense_job(ops, lib, entry, shape, stored=True))


@pytest.mark.parametrize('shape', E.OFFGRID_DENSE_ADAM, ids=str)
def test_fused_dense_filter_gradient_and_adam(ops, lib, shape):
    """each of var_w, m_w, v_w, dz and x alone off the grid.  beta1 = 0 on a zero m slot: m becomes the gradient itself; alpha = 0
    leaves var and v (0.25 everywhere) as they were, guards included"""
    m, k, n = shape
    cs = E.dense_case(m, k, n)
    quarter = np.full((k, n), 0.25)
    call = lambda P, ws, nb: lib.a3d_dense_bwd_filter_adam_tf1(m, k, n, P['x'].ptr, P['dz'].ptr, P['var_w'].ptr, P['m_w'].ptr, P['v_w'].ptr,
                                                               None, None, None, 0.1, 0.0, 1.0, 0.0, 1.0, 1.0, ops._stream())
    sweep(lib, Job('dense_bwd_filter_adam_tf1', f'{shape}', call, None, dict(x=(cs.x, m, k, k), dz=(cs.dz, m, n, n)), {},
                   inout=dict(var_w=(quarter, k, n, n, quarter), m_w=(np.zeros((k, n)), k, n, n, cs.dw), v_w=(quarter, k, n, n, quarter)),
                   has_ws=False))
