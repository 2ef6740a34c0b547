"""What the Python drivers share, without a GPU: the valid_range normaliser, the checkpoint restore in its two steps,
and the flags of the two inference drivers against the --help texts recorded before they were written once."""
import os
import re

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_valid_range_is_none_or_two_ordered_floats():
    from ann3depth_amd.models import check_valid_range
    assert check_valid_range(None) is None
    for given, want in (((0, 10), (0.0, 10.0)), (('1', 2), (1.0, 2.0)), ((2, 2), (2.0, 2.0))):
        got = check_valid_range(given)
        assert got == want and all(type(v) is float for v in got)
    for bad in ((3, 2), (float('nan'), 1)):
        with pytest.raises(ValueError, match='min_depth <= max_depth'):
            check_valid_range(bad)


class Recorder:
    """A stand-in replica: remembers what it was asked to load."""

    def __init__(self):
        self.calls = []

    def load_state_dict(self, sd):
        self.calls.append(('load_state_dict', sd))

    def load_tf_variables(self, tensors):
        self.calls.append(('load_tf_variables', tensors))


def test_restore_reads_a_pt_file_and_a_bundle_and_hands_each_to_its_loader(tmp_path):
    from ann3depth_amd import tfckpt
    from ann3depth_amd.ann3depth import load_checkpoint, read_checkpoint
    sd = {'a/kernel': torch.arange(6, dtype=torch.float32).reshape(2, 3), 'global_step': torch.tensor(7)}
    pt = str(tmp_path / 'model.ckpt-7.pt')
    torch.save(sd, pt)
    state, bundle = read_checkpoint(pt, 'cpu')
    assert bundle is False
    rep = Recorder()
    load_checkpoint(rep, state, bundle)
    (how, got), = rep.calls
    assert how == 'load_state_dict' and list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)

    arrays = {'a/kernel': np.arange(6, dtype=np.float32).reshape(2, 3), 'global_step': np.int64(7)}
    prefix = str(tmp_path / 'model.ckpt-7')
    tfckpt.write_bundle(prefix, arrays)
    state, bundle = read_checkpoint(prefix, 'cpu')
    assert bundle is True
    rep = Recorder()
    load_checkpoint(rep, state, bundle)
    (how, got), = rep.calls
    assert how == 'load_tf_variables' and sorted(got) == sorted(arrays)
    for k, a in arrays.items():
        assert got[k].dtype == np.asarray(a).dtype
        np.testing.assert_array_equal(got[k], a)


def test_a_refusing_replica_lets_its_value_error_through(tmp_path):
    from ann3depth_amd.ann3depth import load_checkpoint, read_checkpoint

    class Refuses(Recorder):
        def load_state_dict(self, sd):
            raise ValueError('a [3, 1] kernel')

    pt = str(tmp_path / 'm.pt')
    torch.save({'global_step': torch.tensor(1)}, pt)
    with pytest.raises(ValueError, match=r'a \[3, 1\] kernel'):
        load_checkpoint(Refuses(), *read_checkpoint(pt, 'cpu'))


def help_text(driver, monkeypatch, capsys):
    monkeypatch.setenv('COLUMNS', '100')                     # the width the recorded texts were wrapped at
    monkeypatch.setattr('sys.argv', ['prog'])
    with pytest.raises(SystemExit) as e:
        driver.parse_args(['--help'])
    assert e.value.code == 0
    return capsys.readouterr().out


@pytest.mark.parametrize('name', ['evaluate', 'predict'])
def test_help_is_the_recorded_text(name, monkeypatch, capsys):
    import importlib
    driver = importlib.import_module(f'ann3depth_amd.{name}')
    with open(os.path.join(GOLD, f'{name}_help.txt')) as f:
        want = f.read()
    squeeze = lambda s: re.sub(r'\s+', ' ', s).strip()
    assert squeeze(help_text(driver, monkeypatch, capsys)) == squeeze(want)


def test_shared_flags_keep_their_defaults_and_short_names():
    from ann3depth_amd import evaluate, predict
    want = dict(model='msdn', batchsize=32, ckptdir='checkpoints', id='', checkpoint='', precision='fp32', superpixel=40)
    for args in (evaluate.parse_args(['nyu']), predict.parse_args(['--out', 'o'])):
        assert {k: getattr(args, k) for k in want} == want
        assert all(type(getattr(args, k)) is type(v) for k, v in want.items())
    given = ['-m', 'dcnf', '-b', '3', '-p', 'c', '--id', 'r', '--checkpoint', 'x.pt', '--precision', 'bf16', '--superpixel', '10']
    want = dict(model='dcnf', batchsize=3, ckptdir='c', id='r', checkpoint='x.pt', precision='bf16', superpixel=10)
    for args in (evaluate.parse_args(given + ['nyu']), predict.parse_args(given + ['--out', 'o'])):
        assert {k: getattr(args, k) for k in want} == want
