"""Plans and timing records of real launches, pinned.  One child process (A3D_TUNING=1 A3D_PLAN_LOG=1, every launch
bracketed) runs a few workloads that between them reach every place a launch is bracketed; its `a3d plan:` lines and every
field of its timing records except the measured `ms` must equal tests/golden/plan_log.json.  Unlike the workspace sizes
of test_plan_table_cpu.py this sees the tile of an unsplit plan too.

The fixture is a RECORD of a known-good library, never of the code under test; on the GPU,

    A3D_LIB=/path/to/known-good/liba3d.so python tests/test_gpu_plan_log.py --record"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'plan_log.json')
FIELDS = ('mode', 'bm', 'bn', 'waves_m', 'nwaves', 'bk', 'avec', 'bvec', 'prec', 'lds_dma', 'splitk', 'm', 'n', 'k', 'flops')
MARK = '== workload '


def workloads():
    """name -> callable; built inside the child, after the library is loaded"""
    import numpy as np
    import torch

    from ann3depth_amd import models, ops
    rng = np.random.default_rng(7)

    def msdn(precision, fine):
        def run():
            B = 2
            img = torch.from_numpy((rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)).cuda()
            dep = torch.from_numpy((rng.integers(1, 256, (B, 480, 640, 1)) / 255).astype(np.float32)).cuda()
            keep = torch.from_numpy(rng.random((B, 4096)) >= 0.5).cuda()
            net = models.MSDNReplica(B, device='cuda:0', seed=3000, precision=precision,
                                     global_step=models.SAMPLES_COARSE // B if fine else 0)
            assert net.step(img, dep, keep)['phase'] == (2 if fine else 1)
        return run

    def dcnf():
        img = torch.from_numpy((rng.integers(0, 256, (1, 480, 640, 3)) / 255).astype(np.float32)).cuda()
        net = models.DCNFUnary(1, seed=3000)
        net.forward(img)
        net.backward(torch.from_numpy(rng.standard_normal((net.P, 1)).astype(np.float32)).cuda())

    def bwd_data(B, bf16):
        # conv2d_4's shape.  fp32: the four parity classes make 360 tiles of 64x64 at B = 16 (one launch for all of them)
        # and 48 at B = 2 (below the 256 that launch wants: one launch per class); bf16 tensors: the bf16 kernel's one launch
        def run():
            d = ops.conv_desc(B, 13, 18, 384, 256, 3, 3, 2, 'VALID', precision='bf16' if bf16 else 'fp32',
                              storage=ops.STORE_X | ops.STORE_W | ops.STORE_Y if bf16 else 0)
            dt = torch.bfloat16 if bf16 else torch.float32
            dz = torch.from_numpy(rng.standard_normal((B, d.ho, d.wo, 256)).astype(np.float32)).cuda().to(dt)
            w = torch.from_numpy(rng.standard_normal((3, 3, 384, 256)).astype(np.float32)).cuda().to(dt)
            ops.conv2d_bwd_data(d, dz, w, torch.empty((B, 13, 18, 384), device='cuda', dtype=dt))
        return run

    return {'msdn fp32 coarse': msdn('fp32', False), 'msdn fp32 fine': msdn('fp32', True),
            'msdn bf16s coarse': msdn('bf16s', False), 'msdn bf16s fine': msdn('bf16s', True),
            'dcnf unary 1 image': dcnf,
            'bwd-data fp32 B16': bwd_data(16, False), 'bwd-data fp32 B2': bwd_data(2, False), 'bwd-data bf16 B16': bwd_data(16, True)}


def child_main():
    """Runs the workloads; marks each on stderr (between the library's plan lines), prints the records as JSON."""
    sys.path.insert(0, ROOT)
    import torch

    from ann3depth_amd import _lib
    lib = _lib.load()
    records = {}
    for name, run in workloads().items():
        sys.stderr.write(MARK + name + '\n')
        sys.stderr.flush()
        lib.a3d_timing_enable(1)
        run()
        torch.cuda.synchronize()
        lib.a3d_timing_enable(0)
        arr = (_lib.TimingRecord * 4096)()
        n = lib.a3d_timing_collect(arr, 4096)
        assert 0 < n < 4096
        records[name] = [[getattr(arr[i], f) for f in FIELDS] for i in range(n)]
    print(json.dumps(records))


def observe():
    """{workload: {'plans': [...], 'records': [...]}} from one child process"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    env.update(A3D_TUNING='1', A3D_PLAN_LOG='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    records = json.loads(r.stdout.strip().splitlines()[-1])
    seen = {name: {'plans': [], 'records': recs} for name, recs in records.items()}
    name = None
    for line in r.stderr.splitlines():
        if line.startswith(MARK):
            name = line[len(MARK):]
        elif line.startswith('a3d plan:'):
            seen[name]['plans'].append(line[len('a3d plan:'):].strip())
    return seen


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def observed():
    return observe()


def test_the_workloads_reach_every_bracketed_launch(recorded):
    """launch_igemm, conv3 and conv3b (lds_dma 2), the few-channel filter gradients in fp32 and bf16 (lds_dma 4), and the two
    one-launch strided bwd-datas, whose flops are the classes' sum and not 2 m n k."""
    recs = [dict(zip(FIELDS, r)) for w in recorded.values() for r in w['records']]
    assert sum(len(w['plans']) for w in recorded.values()) > 50
    for prec in (0, 2):
        assert any(r['lds_dma'] == 2 and r['prec'] == prec for r in recs), f'conv3 / conv3b forward, prec {prec}'
        assert any(r['lds_dma'] == 4 and r['prec'] == prec for r in recs), f'few-channel filter gradient, prec {prec}'
        assert any(r['mode'] == 1 and r['prec'] == prec and r['flops'] != 2.0 * r['m'] * r['n'] * r['k'] for r in recs), \
            f'multi-class bwd-data, prec {prec}'
    per_class = recorded['bwd-data fp32 B2']
    assert len(per_class['plans']) == len(per_class['records']) == 4


@pytest.mark.gpu
def test_plans_and_timing_records_are_the_recorded_ones(recorded, observed):
    assert list(observed) == list(recorded)
    for name, want in recorded.items():
        got = observed[name]
        assert got['plans'] == want['plans'], name
        assert len(got['records']) == len(want['records']), name
        for i, (g, w) in enumerate(zip(got['records'], want['records'])):
            assert g == w, (name, i, dict(zip(FIELDS, w)), dict(zip(FIELDS, g)))


if __name__ == '__main__':
    if sys.argv[1:] == ['--child']:
        child_main()
    elif sys.argv[1:] == ['--record']:
        seen = observe()
        with open(FIXTURE, 'w') as f:
            json.dump(seen, f, separators=(',', ':'))
        for name, w in seen.items():
            print(f'{name}: {len(w["plans"])} plan lines, {len(w["records"])} timing records')
    else:
        sys.exit('usage: test_gpu_plan_log.py --record | --child')
