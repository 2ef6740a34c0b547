"""The wiring of MSDNReplica's objectives: for each of the launch sets a replica can be built with, two coarse-phase and two
fine-phase steps at B = 2 leave the loss words, the summary scalars and the parameters that the same steps left before the
replica read its objective from one record (tests/golden/objective_step_bits.json, recorded twice with equal bits).
Equality is exact: no kernel and no launch differs, only where the Python layer looks the launches up."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_valid_train import fine_start, stored_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'objective_step_bits.json')
B = 2
HOLES = (0.0, 0.99)
CONFIGS = {
    'silog': {},
    'silog_masked': dict(valid_range=HOLES),
    'silog_grad': dict(grad_weight=0.5),
    'silog_grad_masked': dict(grad_weight=0.5, valid_range=HOLES),
    'berhu_masked': dict(objective='berhu', berhu_fraction=0.3, valid_range=HOLES),
    'ssi': dict(objective='ssi'),
    'ssi_masked': dict(objective='ssi', valid_range=HOLES),
}


def bits(t):
    return [f'{w:08x}' for w in t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).tolist()]


def observe(name):
    """What the four steps of configuration `name` leave, in a form JSON holds exactly."""
    from ann3depth_amd import models
    kw = CONFIGS[name]
    img, dep, keep = (torch.from_numpy(a).cuda() for a in stored_batch(7, holes='valid_range' in kw))
    net = models.MSDNReplica(B, seed=3000, beta2=0.999, keep_dense_grads=True, overlap=False, **kw)
    steps = []
    for start in (0, 1, fine_start(models), fine_start(models) + 1):
        net.global_step = start
        out = net.step(img, dep, keep)
        torch.cuda.synchronize()
        assert out['phase'] == models.phase_of(start, B) == (1 if start < 2 else 2)
        steps.append({'loss_out_c': bits(net.loss_out_c), 'loss_out_f': bits(net.loss_out_f),
                      'summary_scalars': [[k, v if isinstance(v, int) else float(v).hex()]
                                          for k, v in net.summary_scalars(out).items()]})
    groups = {f'{gname}.{slot}': hashlib.sha256(getattr(g, slot).cpu().numpy().tobytes()).hexdigest()
              for gname, g in net.groups.items() for slot in ('var', 'm')}
    return {'steps': steps, 'groups': groups}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_steps_leave_the_recorded_bits(name):
    want = json.load(open(GOLDEN))[name]
    got = observe(name)
    assert len(got['steps']) == 4 and len(got['groups']) == 8
    assert json.loads(json.dumps(got)) == want
