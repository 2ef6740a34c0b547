"""Child process of test_gpu_dense_exact.py: the rows of tests/dense_cases.py, element by element, each held to its own route line.

    python tests/exact_dense_worker.py GROUP        (a key of dense_cases.GROUPS)

Run with A3D_TUNING=1 A3D_PLAN_LOG=1: every launch of ann3depth_amd/csrc/dense.hip then prints one `a3d dense:` line on stderr.
The process reads its own stderr: a launch whose line does not show the row's expected entry point, shape, kernel with its template
arguments, grid and splits / span / gpb is a MISMATCH — a row that silently lands on another kernel would prove nothing.  Every
output lies in a NaN-filled allocation with guard elements in front and guard rows behind, and the WHOLE allocation must equal
the float64 reference (integer operands: no tolerance).  The sigmoid rows are held to the float64 sigmoid of the exact
pre-activation within 8 x the largest error of the numpy float32 restatement, at least one ulp of the output.  The rows of
dense_cases.REPEATED also run three times from the same slots (the same bits each time), and those of dense_cases.POISONED (the
repeated ones and one row of each Adam form outside the stream kernels) once on a poisoned gradient.

stdout: `ROUTE | ...` per verified launch, `SIGMOID | ...` figures, `MISMATCH ...` per failure, then `verified N launches`; exit
status 1 on any failure.  A device error ends the process at once: nothing more is launched on a GPU that has faulted."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dense_cases as D  # noqa: E402
import exact_ops as E  # noqa: E402
from ann3depth_amd import _lib, ops  # noqa: E402

LINE = re.compile(r'a3d dense: (\S+) m (\d+) k (\d+) n (\d+) -> (\S+) grid (\d+)x(\d+)(?: splits (\d+) span (\d+))?(?: gpb (\d+))?')
NAN = float('nan')
FRONT, GUARD_ROWS = 64, 67


class RouteLog:
    """this process's stderr, in a file it can read back"""

    def __init__(self):
        self.file = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        sys.stderr.flush()
        os.dup2(self.file.fileno(), 2)
        self.pos = 0

    def new_routes(self):
        size = os.fstat(self.file.fileno()).st_size
        text = os.pread(self.file.fileno(), size - self.pos, self.pos).decode(errors='replace')
        self.pos = size
        out = []
        for g in LINE.finditer(text):
            r = dict(site=g.group(1), shape=tuple(map(int, g.group(2, 3, 4))), kernel=g.group(5), grid=(int(g.group(6)), int(g.group(7))))
            r.update({f: int(v) for f, v in zip(('splits', 'span', 'gpb'), g.group(8, 9, 10)) if v is not None})
            out.append(r)
        return out

    def close(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        size = os.fstat(self.file.fileno()).st_size
        other = [ln for ln in os.pread(self.file.fileno(), size, 0).decode(errors='replace').splitlines() if not ln.startswith('a3d dense:')]
        sys.stderr.write('\n'.join(other[-40:]) + ('\n' if other else ''))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def exact32(ref):
    """the float64 reference as float32, having asserted that nothing is rounded"""
    r32 = np.asarray(ref, np.float64).astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref, equal_nan=True), 'the reference is not exact in float32'
    return r32


class Guarded:
    """rows x cols of float32 inside a NaN-filled allocation: FRONT elements of guard in front (and `off` bytes more: the tensor
    then starts that far off the 256-byte grid), GUARD_ROWS rows behind"""

    def __init__(self, rows, cols, fill=None, off=0):
        assert off % 4 == 0 and 0 <= off < 256
        self.rows, self.cols, self.front = rows, cols, FRONT + off // 4
        self.big = torch.full((self.front + (rows + GUARD_ROWS) * cols,), NAN, device='cuda')
        self.t = self.big[self.front:self.front + rows * cols].view(rows, cols)
        assert self.big.data_ptr() % 256 == 0 and (self.t.data_ptr() - off) % 256 == 0
        if fill is not None:
            self.t.copy_(fill) if torch.is_tensor(fill) else self.t.fill_(fill)

    def expected(self, ref):
        want = torch.full_like(self.big, NAN)
        want[self.front:self.front + self.rows * self.cols] = (ref if torch.is_tensor(ref) else dev(exact32(ref))).reshape(-1)
        return want

    def differs(self, ref, within=None):
        """None if the WHOLE allocation holds `ref` (NaN where ref has NaN) and NaN around it, else where it first differs.
        within: a float64 bound per element of the tensor instead of equality (the sigmoid rows); the guards stay exact."""
        if within is None:
            want = self.expected(ref)
            bad = ~((self.big == want) | (self.big.isnan() & want.isnan()))
            if not bool(bad.any()):
                return None
            got, want = self.big.cpu().numpy(), want.cpu().numpy()
        else:
            got = self.big.cpu().numpy()
            want = np.full(got.shape, np.nan)
            want[self.front:self.front + self.rows * self.cols] = np.asarray(ref, np.float64).reshape(-1)
            tol = np.zeros(got.shape)
            tol[self.front:self.front + self.rows * self.cols] = within.reshape(-1)
            with np.errstate(invalid='ignore'):
                bad = ~((np.abs(got.astype(np.float64) - want) <= tol) | (np.isnan(got) & np.isnan(want)))
            if not bad.any():
                return None
        bad = bad.cpu().numpy() if torch.is_tensor(bad) else bad
        i = int(np.flatnonzero(bad)[0])
        where = f'guard element {i}' if i < self.front else f'row {(i - self.front) // self.cols} column {(i - self.front) % self.cols}' + \
            (' (guard rows)' if i >= self.front + self.rows * self.cols else '')
        return f'{int(bad.sum())} elements differ, first at {where}: got {got[i]}, want {want[i]}'


class Worker:
    def __init__(self):
        self.lib = _lib.load()
        self.log = RouteLog()
        self.failures, self.verified = [], 0

    def check(self, row, what, fn, results, launches=1):
        """fn launches; results() -> the first difference or None.  Holds the launch's route line(s) to the row."""
        self.log.new_routes()
        fn()
        torch.cuda.synchronize()          # a device error raises here and ends the process
        routes = self.log.new_routes()
        m, k, n = row.shape
        want = dict(site=D.SITE[row.entry], shape=row.shape, **row.route)
        label = f'{row.entry} {row.shape} {row.precision} {what}'
        if len(routes) != launches or any(r != want for r in routes):
            self.failures.append(f'MISMATCH {label}: route {routes}, the row expects {launches} x {want}')
            return False
        diff = results()
        if diff:
            self.failures.append(f'MISMATCH {label}: {diff}')
            return False
        self.verified += launches
        r = routes[0]
        extra = ' '.join(f'{f} {r[f]}' for f in ('splits', 'span', 'gpb') if f in r)
        print(f'ROUTE | {row.entry} | {m} {k} {n} | {row.precision} | {what} | {r["kernel"]} | grid {r["grid"][0]}x{r["grid"][1]} | {extra} | x{launches}')
        return True

    # ---------------------------------------------------------------------------------------------------------- forward
    def forward(self, row):
        m, k, n = row.shape
        cs = D.case(row)
        x = Guarded(m, k, dev(cs.x), row.align.get('x', 0)).t
        w, b, keep = dev(cs.w), dev(cs.b), dev(cs.keep, torch.uint8)
        if D.is_sigmoid(row):
            return self.sigmoid(row, cs, x, w, b)
        for bias, act, drop in D.FORWARD_VARIANTS:
            y = Guarded(m, n)
            ref = D.forward_reference(cs, bias, act, drop)
            self.check(row, f'bias {int(bias)} act {act} dropout {int(drop)}',
                       lambda: ops.dense_fwd(x, w, b if bias else None, y.t, act, keep if drop else None), lambda: y.differs(ref))

    def sigmoid(self, row, cs, x, w, b):
        m, k, n = row.shape
        s = cs.y                                                   # the exact pre-activation, bias included
        r64 = 1.0 / (1.0 + np.exp(-s))
        with np.errstate(over='ignore'):
            r32 = np.float32(1) / (np.float32(1) + np.exp(-s.astype(np.float32)))
        e32 = float(np.abs(r32.astype(np.float64) - r64).max())
        bound = np.maximum(8 * e32, np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64))
        y = Guarded(m, n)

        def results():
            got = y.t.cpu().numpy()
            err = np.abs(got.astype(np.float64) - r64)
            print(f'SIGMOID | {m} {k} {n} | splits {row.route["splits"]} | pre-activations in [{s.min():.0f}, {s.max():.0f}] | restatement error '
                  f'{e32:.3g} | kernel {np.nanmax(err):.3g} | largest error / bound {np.nanmax(err / bound):.3g} | '
                  f'{int((got != r32).sum())} of {got.size} differ from the restatement')
            return y.differs(r64, within=bound)
        self.check(row, 'bias 1 act sigmoid dropout 0', lambda: ops.dense_fwd(x, w, b, y.t, 'sigmoid', None), results)

    # ---------------------------------------------------------------------------------------------------------- plain filter gradient
    def filter_gradient(self, row):
        m, k, n = row.shape
        cs = D.case(row)
        x, dz = dev(cs.x), dev(cs.dz)
        for with_db in (True, False):
            dw, db = Guarded(k, n), Guarded(1, n)
            self.check(row, f'db {int(with_db)}', lambda: ops.dense_bwd_filter(x, dz, dw.t, db.t[0] if with_db else None),
                       lambda: dw.differs(cs.dw) or db.differs(cs.db if with_db else np.full(n, np.nan)))

    # ---------------------------------------------------------------------------------------------------------- fused gradient + Adam
    VAR, V = 0.25, 0.125

    def slots(self, row, with_bias):
        m, k, n = row.shape
        s = [Guarded(k, n, self.VAR), Guarded(k, n, 0.0), Guarded(k, n, self.V)]
        return s + ([Guarded(1, n, self.VAR), Guarded(1, n, 0.0), Guarded(1, n, self.V)] if with_bias else [])

    def adam_launch(self, row, x, dz, s, beta1, b1p):
        bias = [g.t[0] for g in s[3:]] or [None, None, None]
        ops.dense_bwd_filter_adam_tf1(x, dz, s[0].t, s[1].t, s[2].t, *bias, 0.1, beta1, 1.0, b1p, 1.0, D.GRAD_SCALE, precision=row.precision)

    def adam(self, row):
        m, k, n = row.shape
        cs = D.case(row)
        x = Guarded(m, k, dev(cs.x), row.align.get('x', 0)).t
        steps = [(dev(dz), beta1, b1p, dev(exact32(m_w)), m_b) for dz, beta1, b1p, m_w, m_b in D.adam_steps(cs)]
        var = torch.full((k, n), self.VAR, device='cuda')
        v = torch.full((k, n), self.V, device='cuda')
        for with_bias in D.ADAM_VARIANTS:
            s = self.slots(row, with_bias)
            for i, (dz, beta1, b1p, m_w, m_b) in enumerate(steps):
                def results():
                    d = s[0].differs(var) or s[1].differs(m_w) or s[2].differs(v)
                    if not d and with_bias:
                        d = s[3].differs(np.full(n, self.VAR)) or s[4].differs(m_b) or s[5].differs(np.full(n, self.V))
                    return d
                if not self.check(row, f'bias slots {int(with_bias)} step {i + 1}', lambda: self.adam_launch(row, x, dz, s, beta1, b1p), results):
                    break
        if row in D.REPEATED:
            self.repeated(row, cs, x, steps[0][0])
        if row in D.POISONED:
            self.poisoned(row, cs, x)

    def repeated(self, row, cs, x, dz):
        """three launches from the same slots (m = 1 everywhere, beta1 = 1/2): the same bits each time"""
        bits = []

        def launch():
            for _ in range(3):
                s = self.slots(row, True)
                s[1].t.fill_(1.0), s[4].t.fill_(1.0)
                self.adam_launch(row, x, dz, s, 0.5, 0.25)
                bits.append([g.big.view(torch.int32).clone() for g in s])
        self.check(row, 'three runs', launch, lambda: None if all(torch.equal(a, b) for other in bits[1:] for a, b in zip(bits[0], other))
                   else 'the bits differ from run to run', launches=3)

    def poisoned(self, row, cs, x):
        """inf in dz[0, 3], 2^66 in dz[m - 1, n - 1]: v and var take NaN exactly where dense_cases.poison_masks says, which is
        exactly where a3d_dense_bwd_filter + a3d_adam_apply_tf1 put it; m agrees with theirs (NaN where theirs is NaN)"""
        m, k, n = row.shape
        dz = dev(D.poisoned_dz(cs))
        fused = self.slots(row, True)
        self_w, self_b = D.poison_masks(cs)

        def results():
            dw, db = torch.empty((k, n), device='cuda'), torch.empty(n, device='cuda')
            ops.dense_bwd_filter(x, dz, dw, db)
            plain = self.slots(row, True)
            ops.adam_apply_tf1(plain[0].t, plain[1].t, plain[2].t, dw, 0.1, 0.5, 1.0, 1e-8, 0.25, 1.0, D.GRAD_SCALE)
            ops.adam_apply_tf1(plain[3].t[0], plain[4].t[0], plain[5].t[0], db, 0.1, 0.5, 1.0, 1e-8, 0.25, 1.0, D.GRAD_SCALE)
            torch.cuda.synchronize()
            for name, f, p in zip(('var_w', 'm_w', 'v_w', 'var_b', 'm_b', 'v_b'), fused, plain):
                d = f.differs(p.t)
                if d:
                    return f'{name} against the two passes: {d}'
            for name, g, mask, keep in (('var_w', fused[0], self_w, self.VAR), ('v_w', fused[2], self_w, self.V),
                                        ('var_b', fused[3], self_b, self.VAR), ('v_b', fused[5], self_b, self.V)):
                d = g.differs(np.where(mask, np.nan, keep))
                if d:
                    return f'{name} against the stated poison mask: {d}'
            if not bool(torch.isfinite(fused[1].t[:, n - 1]).all()) or int(fused[1].t.isfinite().logical_not().sum()) != k:
                return 'm_w: non-finite outside column 3, or finite inside it'
            return None
        self.check(row, 'poisoned gradient', lambda: self.adam_launch(row, x, dz, fused, 0.5, 0.25), results)


def main():
    assert os.environ.get('A3D_TUNING') == '1' and os.environ.get('A3D_PLAN_LOG') == '1', 'run by test_gpu_dense_exact.py'
    rows = D.GROUPS[sys.argv[1]]
    w = Worker()
    try:
        for row in rows:
            {D.FWD: w.forward, D.DW: w.filter_gradient, D.ADAM: w.adam}[row.entry](row)
            E.dense_case.cache_clear()
    finally:
        w.log.close()
    for f in w.failures:
        print(f)
    print(f'verified {w.verified} launches')
    return 1 if w.failures else 0


if __name__ == '__main__':
    sys.exit(main())
