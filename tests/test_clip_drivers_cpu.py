"""--clip-norm on the training driver: listed as NON-REFERENCE, parsed (inf included), refused before anything is set up for a
value that is no bound and for a model without an optimizer group, and validated alike by the replicas' check.  No GPU."""
import math
import os

import pytest

from test_gpu_berhu_train import restore_signals


def test_the_flag_is_listed_as_non_reference_and_parses(capsys):
    from ann3depth_amd import ann3depth
    with pytest.raises(SystemExit):
        ann3depth.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--clip-norm C' in text and text.split('--clip-norm C')[-1].lstrip().startswith('NON-REFERENCE')
    assert ann3depth.parse_args(['nyu']).clip_norm is None
    assert ann3depth.parse_args(['--clip-norm', '10', 'nyu']).clip_norm == 10.0
    assert ann3depth.parse_args(['--clip-norm', 'inf', 'nyu']).clip_norm == math.inf
    assert '--clip-norm' in ann3depth.__doc__


def test_cli_refusals_come_before_anything_is_set_up(tmp_path, caplog):
    from ann3depth_amd import ann3depth, models
    try:
        common = ['--ckptdir', str(tmp_path), '--datadir', str(tmp_path)]
        for model in ('msdn', 'dcnf'):
            for bad in ('0', '-1', '-inf', 'nan'):
                assert ann3depth.main(['--model', model, *common, '--clip-norm=' + bad, 'nyu']) == 2, (model, bad)
        assert ann3depth.main(['--model', 'msdn', *common, '--optimizer', 'momentum', '--clip-norm', '0', 'nyu']) == 2
        assert ann3depth.main(['--model', 'dcnf', *common, '--train-pairwise', '--clip-norm', 'nan', 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
        assert models.msdn.clip_norm is None and models.dcnf.clip_norm is None
    finally:
        restore_signals()


def test_a_model_without_an_optimizer_group_is_refused(tmp_path, monkeypatch):
    from ann3depth_amd import ann3depth, models

    class NoGroups:
        """A plugin that trains nothing the flag could bound."""
    monkeypatch.setattr(models, 'plain', NoGroups(), raising=False)
    try:
        assert ann3depth.main(['--model', 'plain', '--ckptdir', str(tmp_path), '--datadir', str(tmp_path), '--clip-norm', '1',
                               'nyu']) == 2
        assert not os.listdir(tmp_path)
    finally:
        restore_signals()


def test_the_replicas_check_is_the_drivers():
    from ann3depth_amd import models
    assert models.check_clip_norm(None) is None and models.check_clip_norm('2.5') == 2.5
    assert models.check_clip_norm(math.inf) == math.inf
    for bad in (0, -1.0, -math.inf, math.nan):
        with pytest.raises(ValueError, match='clip_norm'):
            models.check_clip_norm(bad)
    assert models.MSDN_PHASE_GROUPS == {1: ('CoarseConv', 'CoarseDense'), 2: ('FineA', 'FineB')}
    assert set(sum(models.MSDN_PHASE_GROUPS.values(), ())) == set(models.MSDN_OPTIMIZERS)
