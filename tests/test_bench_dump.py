"""bench.py --dump-outputs: what the last timed step computed, written so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_float32_and_samples_large_outputs_at_fixed_positions(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE + 12345, dtype=torch.float32)
    arrays = {'loss': torch.tensor([2.5]), 'map': torch.linspace(-1, 1, 24).view(2, 3, 4, 1).to(torch.bfloat16), 'big': big}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    loss, small, sample = (np.load(tmp_path / 'a' / f'{n}.npy') for n in ('loss', 'map', 'big'))
    assert loss.dtype == small.dtype == sample.dtype == np.float32
    assert loss.tolist() == [2.5]
    np.testing.assert_array_equal(small, arrays['map'].float().numpy())
    # big[i] == i: the sample holds DUMP_SAMPLE distinct positions in order, and the same ones in every call
    assert sample.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(sample) > 0) and sample[-1] < big.numel()
    np.testing.assert_array_equal(sample, np.load(tmp_path / 'b' / 'big.npy'))


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_in_every_run(tmp_path):
    """Two runs with the same arguments: the line reports the timed steps it was asked for, and both write the same outputs
    bit for bit (seeded inputs and weights; the kernels use no floating-point atomics and the planner no timings)."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2',
           '--no-cpu-baseline', '--no-fine', '--no-dp-rank', '--also', '']
    lines = []
    for run in ('a', 'b'):
        r = subprocess.run(cmd + ['--dump-outputs', str(tmp_path / run)], capture_output=True, text=True, cwd=ROOT,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1]))
    assert all(line['steps'] == 3 and line['ms_per_step'] > 0 for line in lines)
    names = {f'{n}.npy' for n in ('coarse_loss', 'fine_loss', 'coarse', 'fine')}
    names |= {f'{g}_{s}.npy' for g in ('CoarseConv', 'CoarseDense', 'FineA', 'FineB') for s in ('var', 'm', 'v')}
    assert set(os.listdir(tmp_path / 'a')) == set(os.listdir(tmp_path / 'b')) == names
    total = 0
    for n in sorted(names):
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert np.load(tmp_path / 'a' / 'coarse.npy').shape == (2, 55, 74, 1)
    assert np.load(tmp_path / 'a' / 'CoarseDense_m.npy').shape == (bench.DUMP_SAMPLE,)
    assert np.abs(np.load(tmp_path / 'a' / 'CoarseDense_m.npy')).max() > 0          # the step's dense gradients reached m
    assert total <= 64 << 20
