"""Child process of test_gpu_exact.py: pinned tile configurations, split-K factors and stream-K grids, element by element.

Run with A3D_TUNING=1 (the library then reads its A3D_FORCE_* / A3D_BF16_BN / A3D_RING_CFG switches per launch) and
A3D_PLAN_LOG=1 (one `a3d plan:` line per implicit-GEMM launch on stderr).  Each reference (tests/exact_ops.py: integer
operands, exact in float32 and bf16; in the rounded-store passes of the bf16 launches: sums a bf16 tensor holds as their RNE) is computed once; every launch writes into a NaN-filled allocation with guard rows, and
the whole allocation must equal the reference.  The process reads its own stderr: a launch whose plan line does not show the
pinned configuration (or its register-staged twin), the split factor after the planner's clamp to the k-tile count, or the
stream-K grid is a MISMATCH too — a switch that silently does not apply would prove nothing.

stdout: one `MISMATCH ...` line per failure, then `verified N (configuration, split) combinations`; exit status 1 on any failure."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import exact_ops as E  # noqa: E402
from ann3depth_amd import _lib, ops  # noqa: E402

SWITCHES = ('A3D_FORCE_CFG', 'A3D_FORCE_SPLITK', 'A3D_FORCE_STREAMK', 'A3D_BF16_BN', 'A3D_RING_CFG')
PLAN = re.compile(r'a3d plan: mode (\d+) M (\d+) N (\d+) K (\d+) -> (cfg|ring) (\d+) \((\d+)x(\d+)\) splitk (\d+) streamk (\d+) grid (\d+)')
NAN = float('nan')
BF = torch.bfloat16


class PlanLog:
    """this process's stderr, in a file it can read back"""

    def __init__(self):
        self.file = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        sys.stderr.flush()
        os.dup2(self.file.fileno(), 2)
        self.pos = 0

    def new_plans(self):
        size = os.fstat(self.file.fileno()).st_size
        text = os.pread(self.file.fileno(), size - self.pos, self.pos).decode(errors='replace')
        self.pos = size
        return [dict(zip(('mode', 'M', 'N', 'K'), map(int, m.group(1, 2, 3, 4))), kind=m.group(5), index=int(m.group(6)),
                     splitk=int(m.group(9)), streamk=int(m.group(10))) for m in PLAN.finditer(text)]

    def close(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        size = os.fstat(self.file.fileno()).st_size
        other = [ln for ln in os.pread(self.file.fileno(), size, 0).decode(errors='replace').splitlines() if not ln.startswith('a3d plan:')]
        sys.stderr.write('\n'.join(other[-40:]) + ('\n' if other else ''))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda().to(dtype)


def guarded(rows, ld, dtype=torch.float32):
    return torch.full((rows + 67, ld), NAN, device='cuda', dtype=dtype)


def differs(big, rows, cols, ref):
    """None if the whole allocation equals `ref` in its first rows x cols and NaN elsewhere, else where it first differs"""
    want = np.full(tuple(big.shape), np.nan, np.float64)
    want[:rows, :cols] = np.asarray(ref, np.float64).reshape(rows, cols)
    got = big.float().cpu().numpy().astype(np.float64)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return f'{int(bad.sum())} elements differ, first at row {r} column {c}: got {got[r, c]}, want {want[r, c]}'


class Problem:
    """a conv case on the device, float32 or bf16 tensors, and one launch per direction"""

    def __init__(self, case, stored, rounded=False):
        self.case, self.stored = case, stored
        # rounded: operands up to 8, the bf16 y and dx hold RNE(exact sum) — conditions asserted by exact_ops.rounded_case
        self.cs = cs = E.rounded_case(case, 'y', 'dx') if rounded else E.conv_case(*case)
        assert stored or not rounded
        n, h, w, c, k, ks, st, pad = case
        tdt = BF if stored else torch.float32
        self.tdt = tdt
        if stored and not rounded:
            cs.bf16('y', 'dx')
        self.x, self.w, self.b, self.dz = dev(cs.x, tdt), dev(cs.w, tdt), dev(cs.b), dev(cs.dz, tdt)
        d = ops.conv_desc(n, h, w, c, k, ks, ks, st, pad, precision='bf16' if stored else 'fp32')
        X, W, Y = ops.STORE_X, ops.STORE_W, ops.STORE_Y
        self.d = {0: ops.with_storage(d, X | W | Y if stored else 0), 1: ops.with_storage(d, X | W | Y if stored else 0),
                  2: ops.with_storage(d, X | Y if stored else 0)}

    def run(self, mode, second=None):
        """-> None or a description of the first difference.  second: the type of a second output beside the forward's y (it
        must hold what y holds: written by the split-K reduction in a split launch, by second_output_kernel in a whole one)"""
        cs = self.cs
        n, h, w, c, k, ks, st, pad = self.case
        if mode == 0:                                      # bias + ReLU in the epilogue / the reduction
            rows = n * cs.ho * cs.wo
            y = guarded(rows, k, self.tdt)
            y2 = guarded(rows, k, second) if second is not None else None
            ops.conv2d_fwd(self.d[0], self.x, self.w, self.b, y[:rows].view(n, cs.ho, cs.wo, k), 'relu',
                           out2=ops.second_output(y2[:rows]) if second is not None else None)
            ref = np.maximum(cs.y, 0)
            ref = cs.stored('y', ref) if self.stored else ref
            return differs(y, rows, k, ref) or (second is not None and differs(y2, rows, k, ref) or None)
        if mode == 1:                                      # with the ReluGrad of the layer below
            rows = n * h * w
            dx = guarded(rows, c, self.tdt)
            ops.conv2d_bwd_data(self.d[1], self.dz, self.w, dx[:rows].view(n, h, w, c), relu_mask=self.x)
            ref = cs.dx * (cs.x > 0)
            return differs(dx, rows, c, cs.stored('dx', ref) if self.stored else ref)
        dw, db = guarded(ks * ks * c, k), guarded(1, k)      # with the fused BiasAddGrad
        ops.conv2d_bwd_filter(self.d[2], self.x, self.dz, dw[:ks * ks * c].view(ks, ks, c, k), db[0])
        return differs(dw, ks * ks * c, k, cs.dw) or differs(db, 1, k, cs.db)


def timed(lib, fn):
    lib.a3d_timing_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.a3d_timing_enable(0)
    arr = (_lib.TimingRecord * 64)()
    return out, [arr[i] for i in range(lib.a3d_timing_collect(arr, 64))]


def main():
    assert os.environ.get('A3D_TUNING') == '1' and os.environ.get('A3D_PLAN_LOG') == '1', 'run by test_gpu_exact.py'
    lib = _lib.load()
    log = PlanLog()
    failures, verified = [], 0
    problems = {}

    def problem(case, stored, rounded=False):
        if (case, stored, rounded) not in problems:
            problems[case, stored, rounded] = Problem(case, stored, rounded)
        return problems[case, stored, rounded]

    def launch(prob, mode, env, second=None):
        for v in SWITCHES:
            os.environ.pop(v, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        log.new_plans()
        diff, recs = timed(lib, lambda: prob.run(mode, second))
        return diff, recs, log.new_plans()

    try:
        for case, mode, cfg, kind, value in E.forced_f32_combos():
            what = f'fp32 {case} mode {mode} cfg {cfg} {kind} {value}'
            diff, recs, plans = launch(problem(case, False), mode, {'A3D_FORCE_CFG': cfg, 'A3D_FORCE_' + kind.upper(): value})
            # a strided bwd-data is one launch per parity class under a pinned tile; everything else is one launch
            want_launches = 4 if (mode == 1 and case[6] == 2) else 1
            ok = len(plans) == want_launches
            for p in plans:
                want_split = E.clamped_split(p['K'], 32, value) if kind == 'splitk' else 1
                want_grid = value if kind == 'streamk' else 0
                ok &= (p['kind'] == 'cfg' and p['index'] in (cfg, E.TWIN.get(cfg, cfg)) and p['mode'] == mode
                       and p['splitk'] == want_split and p['streamk'] == want_grid)
            if not ok:
                failures.append(f'MISMATCH {what}: the pinned plan was not applied: {plans}')
            elif diff:
                failures.append(f'MISMATCH {what}: {diff}')
            else:
                verified += 1
        # identity stores, then the same pinned launches on sums the bf16 store rounds (once, after split-K slabs are added)
        bf16_passes = [(combo, False) for combo in E.forced_bf16_combos()] + [(combo, True) for combo in E.forced_bf16_rounded_combos()]
        for (case, mode, kind, value, split), rounded in bf16_passes:
            what = f'bf16 {case} mode {mode} {kind} {value} splitk {split}' + (' rounded store' if rounded else '')
            env = {'A3D_BF16_BN': value, 'A3D_FORCE_SPLITK': split} if kind == 'bn' else {'A3D_RING_CFG': value}
            # the rounded forwards also write a second output: bf16 beside 64 columns and odd tiles, float32 beside the others, so
            # both types are written by a split launch (factors 2, 3) and by a whole one
            second = None if not (rounded and mode == 0) else BF if (value == 64 or value % 2 == 1) else torch.float32
            diff, recs, plans = launch(problem(case, True, rounded), mode, env, second)
            ok = len(plans) == 1 and len(recs) == 1 and plans[0]['mode'] == mode and recs[0].prec == 2
            if ok and kind == 'bn':          # the plan line does not show the bf16 kernel's column width: the timing record does
                ok = (plans[0]['kind'] == 'cfg' and recs[0].lds_dma == 0 and recs[0].bn == value
                      and plans[0]['splitk'] == recs[0].splitk == E.clamped_split(plans[0]['K'], 64, split) and plans[0]['streamk'] == 0)
            elif ok:
                ok = plans[0]['kind'] == 'ring' and plans[0]['index'] == value and recs[0].lds_dma == 3
            if not ok:
                failures.append(f'MISMATCH {what}: the pinned plan was not applied: {plans} '
                                f'{[(r.mode, r.prec, r.lds_dma, r.bm, r.bn, r.splitk) for r in recs]}')
            elif diff:
                failures.append(f'MISMATCH {what}: {diff}')
            else:
                verified += 1
    finally:
        log.close()
    for f in failures:
        print(f)
    print(f'verified {verified} (configuration, split) combinations')
    return 1 if failures else 0


if __name__ == '__main__':
    sys.exit(main())
