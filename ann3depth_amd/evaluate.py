"""Evaluation driver: restore an MSDN or DCNF checkpoint and measure it on the test split.

The converter writes ``test.tfrecords`` beside ``train.tfrecords`` (tools/data_tf_converter.py, src/data.py:58-59);
training never reads it.  This driver reads every test record once, in file order (data.OrderedBatch), runs the
network's forward without targets (the replica's predict(): dropout off, no loss, weights untouched) and reports the
held-out error metrics of Eigen et al. 2014, Table 1 (ops.depth_metrics on the GPU, ops.summarize_depth_metrics on the
host), plus the training objective on the test split.

    python -m ann3depth_amd.evaluate nyu --model msdn|dcnf --id r1 [--checkpoint PATH] [--resolution grid|record] ...

msdn: the coarse and the coarse + fine output, each with its scale-invariant log loss ``silog``; ``grid`` is 55 x 74.
dcnf: ``unary``, the unary stack's z (what the reference draws as its Output image), and ``crf``, the MAP depths
A^-1 z of the conditional random field (ops.crf_map: one pivoted LU per image; the reference never forms them), both on
the 6 x 8 superpixel grid and sampled at the target's pixels inside the metrics kernel; ``grid`` is 240 x 320, the size
the DCNF step resizes its targets to.  The objective is reported once, as ``crf_nll``; ``singular_systems`` counts the
images whose system had no solution (their crf row is NaN and shows up under ``nonfinite``).

``--upsample joint`` (NON-REFERENCE; ``--radius``, ``--sigma-space``, ``--sigma-range``) adds a third output, ``fine_joint``
or ``crf_joint``: the same prediction brought to the record image's size by joint bilateral upsampling under the batch's
images (ops.joint_bilateral_upsample, include/a3d_upsample.h), judged against the same target.  The default,
``none``, launches nothing more and adds no key.

``--condition KEEP --condition-seed S`` (NON-REFERENCE, dcnf, ``--resolution grid``, 0 < KEEP < 1) judges depth completion
(include/a3d_posterior.h, DCNFReplica.posterior).  Per record a host generator seeded by (S, the record's index in the
file) keeps each target superpixel with probability KEEP; the field is conditioned on the kept ones, and two outputs are
judged over the pixels of the other superpixels only (the kept superpixels' pixels of a copy of the target are set to
min_depth, which the metrics' validity test ``min_depth < t`` refuses): ``crf_cond``, the completed map, and
``crf_hidden``, the unconditioned MAP depths on the same pixels.  Also ``condition_z2``, the mean over the hidden
superpixels of (y - mean)^2 / var in float64 on the host, which is 1 for a calibrated field (var is the conditional
variance of y itself), ``hidden_fraction`` (hidden / measured superpixels, images whose system was rejected left out) and
``rejected_systems``.  Without the flag nothing more is launched and the report has no new key.

``--segmentation slic [--slic-iters N --slic-compactness M]`` (NON-REFERENCE, dcnf, a checkpoint of ``--unary fcsp``;
include/a3d_slic.h, DCNFReplica(segmentation='slic'); the training driver's three flags, not listed by ``--help``) runs the
field over SLIC superpixels of the resized image instead of square blocks, at any ``--superpixel``; no weight depends on
it.  ``unary`` and ``crf`` are painted onto 240 x 320 by the labels (DCNFReplica.depth_map) before the metrics kernel reads
them, and the report gains ``segmentation``, ``slic_iters``, ``slic_compactness``.  Refused with it, before any GPU work:
``--upsample joint``, ``--observed-nll``, ``--condition``.  Without the flag (``grid``) nothing differs.

``--loss berhu [--berhu-fraction F]`` (NON-REFERENCE, msdn; the training driver's two flags, not listed by ``--help``;
include/a3d_berhu.h) adds ``berhu`` beside ``silog`` to ``coarse`` and ``fine``: the plain reverse Huber loss on the grid
targets with the threshold F (default 0.2, 0 < F <= 1) times each image's largest error, averaged the way ``silog`` is, and the
report gains ``loss`` and ``berhu_fraction``.  Checkpoints do not record the objective: any MSDN checkpoint can be asked.
Without the flag nothing more is launched and the report has no new key.

``--loss ssi`` (NON-REFERENCE, msdn; not listed by ``--help`` either; include/a3d_ssi.h) adds ``ssi`` beside ``silog`` to
``coarse`` and ``fine``: the plain least-squares scale-and-shift-invariant loss on the grid targets, averaged the way ``silog``
is, and the report gains ``loss``.  A checkpoint trained under it is judged with ``--align affine``.

``--align median|scale|affine`` (NON-REFERENCE, both models; include/a3d_align.h, ops.depth_align; not listed by ``--help``):
the depth maps the models train on are min-max scaled per image, so a checkpoint predicts depth up to an affine map per
image.  Every output judged is judged a second time as ``<name>_aligned`` after a per-image scale (``median``: the ratio of
the lower medians; ``scale``: least squares) or scale and shift (``affine``: least squares) fitted against the same target
over the pixels the metrics count, under the same ``--min-depth`` / ``--max-depth``.  Each ``_aligned`` entry also carries
``unaligned_images`` (images that could not be fitted and were judged as they are) and ``mean_scale`` / ``mean_shift`` over
the others; the report gains ``align``.  ``--predictions`` keeps writing the unaligned maps.  The default, ``none``,
launches nothing more and adds no key.

Output: one JSON line on stdout, ``<ckptdir>/<model>_<id>/eval-<global_step>.json`` and TensorBoard scalars
``eval/<output>/<metric>`` (and ``eval/crf_nll``) at the checkpoint's global step.  Exit code 2 when there is nothing to
evaluate (no checkpoint, no test split) or the request is unsupported (an unknown model, more than one process).
"""
import argparse
import collections
import json
import os
import sys

import numpy as np
import torch

from . import data, ops, summary, tfckpt
from .ann3depth import add_segmentation_args, latest_checkpoint, load_checkpoint, read_checkpoint
from .feed import DeviceFeed

OUTPUTS = {'msdn': ('coarse', 'fine'), 'dcnf': ('unary', 'crf')}
# --loss NAME beside silog: what its refusal calls it, the Evaluator's keyword arguments for it, whether the report repeats them
ExtraLoss = collections.namedtuple('ExtraLoss', 'phrase keywords reported')
EXTRA_LOSSES = {
    'berhu': ExtraLoss('the reverse Huber loss',
                       lambda args: {'berhu_fraction': 0.2 if args.berhu_fraction is None else args.berhu_fraction}, True),
    'ssi': ExtraLoss('the scale-and-shift-invariant loss', lambda args: {'ssi': True}, False),
}


def _say(msg):
    print(f'evaluate: {msg}', file=sys.stderr, flush=True)


class EvalOp:
    """The test split's batches on the device, in file order, through a feed.DeviceFeed.  run(fn) calls
    fn(images, depths, n) on the current stream with batch k's device tensors (B rows, the first n of them this batch's
    records; each uint8 when every record of the batch staged that feature as pixel values) and returns what fn returns;
    OutOfRangeError after the last batch."""

    def __init__(self, pipeline, batchsize, device):
        self.pipeline, self.B = pipeline, batchsize
        self.feed = DeviceFeed(pipeline, batchsize, device)
        self.feed.start()

    def run(self, fn):
        images, depths, n, _ = self.feed.take()
        out = fn(images, depths, n)
        self.feed.give_back()
        return out


class MetricRows:
    """What the evaluators of both models keep: the metric rows of every output per batch, the batch sizes and, when
    asked for, the predictions."""

    def __init__(self, replica, resolution, more_outputs, prediction_shape, min_depth, max_depth, clamp_lo, clamp_hi,
                 keep_predictions, align=None):
        """align (NON-REFERENCE, --align median|scale|affine): every output judged is judged a second time as
        `<name>_aligned`, after the per-image scale and shift of ops.depth_align against the same target."""
        self.rep, self.resolution = replica, resolution
        self.outputs = self.outputs + more_outputs
        self.kw = dict(min_depth=min_depth, max_depth=max_depth, clamp_lo=clamp_lo, clamp_hi=clamp_hi)
        self.align = align
        self.aligned = tuple(o + '_aligned' for o in self.outputs) if align is not None else ()
        self.rows = {o: [] for o in self.outputs + self.aligned}
        self.fits = {o: [] for o in self.aligned}            # (coef, status) per batch
        self.counts = []
        self.predictions = [] if keep_predictions else None
        self.prediction_shape = prediction_shape

    def judge(self, name, out, n, target):
        """Append the metric rows of out[:n] against target under output `name`."""
        self.rows[name].append(ops.depth_metrics(out[:n], target, **self.kw))
        if self.align is not None:
            coef, _, status = ops.depth_align(out[:n], target, self.align, min_depth=self.kw['min_depth'],
                                              max_depth=self.kw['max_depth'])
            self.rows[name + '_aligned'].append(ops.depth_metrics(out[:n], target, coef=coef, **self.kw))
            self.fits[name + '_aligned'].append((coef, status))

    def mean(self, per_batch):
        """The mean over the records of per-batch means ([1] device tensors, one per batch)."""
        n = np.asarray(self.counts, np.float64)
        per_batch = torch.cat(per_batch).double().cpu().numpy()
        return float((per_batch * n).sum() / n.sum())

    def results(self):
        torch.cuda.synchronize()
        out = {name: ops.summarize_depth_metrics(torch.cat(self.rows[name])) for name in self.outputs + self.aligned}
        for name in self.aligned:
            coef = torch.cat([c for c, _ in self.fits[name]]).double().cpu().numpy()
            ok = torch.cat([s for _, s in self.fits[name]]).cpu().numpy() == 0
            out[name].update(unaligned_images=int((~ok).sum()),
                             mean_scale=float(coef[ok, 0].mean()) if ok.any() else float('nan'),
                             mean_shift=float(coef[ok, 1].mean()) if ok.any() else float('nan'))
        return out


class Evaluator(MetricRows):
    """MSDN's per-batch work: predict, targets on the grid (the training step's resize), metric rows, the objective."""
    outputs = OUTPUTS['msdn']

    def __init__(self, replica, resolution='grid', min_depth=0., max_depth=float('inf'), clamp_lo=1e-3,
                 clamp_hi=float('inf'), keep_predictions=False, upsample=None, berhu_fraction=None, align=None,
                 ssi=False):
        """upsample (NON-REFERENCE, --upsample joint): an ops.JointUpsampler; a third output `fine_joint`, the fine map
        brought to the record image's size under the batch's images, is judged against the same target.
        berhu_fraction (NON-REFERENCE, --loss berhu): also report `berhu`, the plain reverse Huber loss on the grid targets
        with this threshold fraction, beside `silog`.
        ssi (NON-REFERENCE, --loss ssi): also report `ssi`, the plain scale-and-shift-invariant loss on the grid targets."""
        from .models import OUT_H, OUT_W
        super().__init__(replica, resolution, ('fine_joint',) if upsample is not None else (), (OUT_H, OUT_W), min_depth,
                         max_depth, clamp_lo, clamp_hi, keep_predictions, align)
        self.upsample = upsample
        self.t = torch.empty((replica.B, OUT_H, OUT_W), device=replica.device)
        # the plain losses reported per output, silog and what was asked for beside it: report key -> (floats a launch writes, the
        # first the mean over the batch's images; workspace factory; launch(out, target, loss, ws))
        self.objectives = {'silog': (1, ops.silog_ws, ops.silog_loss_fwd)}
        if berhu_fraction is not None:
            self.objectives['berhu'] = (4, ops.berhu_ws, lambda o, t, loss, ws: ops.berhu_loss_fwd(o, t, 0, berhu_fraction, loss, ws))
        if ssi:
            self.objectives['ssi'] = (4, ops.ssi_ws, lambda o, t, loss, ws: ops.ssi_loss_fwd(o, t, 0, loss, ws))
        self.loss_ws = {}               # per (key, batch size): the launches' per-sample sums and partials
        self.losses = {(o, key): [] for o in OUTPUTS['msdn'] for key in self.objectives}

    def __call__(self, images, depths, n):
        coarse, fine = self.rep.predict(images, n)
        ops.resize_bilinear_tf1(depths[:n], self.t[:n].view(n, self.t.shape[1], self.t.shape[2], 1))
        target = self.t[:n] if self.resolution == 'grid' else depths[:n]
        for name, out in zip(OUTPUTS['msdn'], (coarse, fine)):
            self.judge(name, out, n, target)
            for key, (width, ws_for, launch) in self.objectives.items():
                loss = torch.empty(width, device=out.device)
                ws = self.loss_ws.get((key, n))
                if ws is None:
                    ws = self.loss_ws[key, n] = ws_for(n, out.device)
                launch(out[:n], self.t[:n], loss, ws)                            # the mean over these n images
                self.losses[name, key].append(loss[:1])
        if self.upsample is not None:
            self.judge('fine_joint', self.upsample(fine[:n], images[:n]), n, target)
        self.counts.append(n)
        if self.predictions is not None:
            self.predictions.append(fine[:n].clone())

    def results(self):
        out = super().results()
        for (name, key), losses in self.losses.items():
            out[name][key] = self.mean(losses)
        return out


class DCNFEvaluator(MetricRows):
    """DCNF's per-batch work: predict (unary z and the field's MAP depths), the objective on the same batch, which also
    leaves the targets at 240 x 320, and the metric rows of both outputs; the replica's rows x cols predictions are sampled at the
    target's pixels inside a3d_depth_metrics."""
    outputs = OUTPUTS['dcnf']

    def __init__(self, replica, resolution='grid', min_depth=0., max_depth=float('inf'), clamp_lo=1e-3,
                 clamp_hi=float('inf'), keep_predictions=False, observed_nll=False, upsample=None, condition=None,
                 align=None):
        """observed_nll (NON-REFERENCE): also the training objective of a run with --min-depth / --max-depth, the
        likelihood of the superpixels that (min_depth, max_depth] leaves observed (DCNFReplica.nll(valid_range=...)); it
        runs last in a batch, after the metrics have read the plainly resized targets.
        upsample (NON-REFERENCE, --upsample joint): an ops.JointUpsampler; a third output `crf_joint`, the MAP depths
        brought to the record image's size under the batch's images, is judged against the same target.
        condition (NON-REFERENCE, --condition KEEP --condition-seed S): (keep, seed); two more outputs, `crf_cond` and
        `crf_hidden`, judged over the pixels of the superpixels hidden from the field; it runs last in a batch."""
        super().__init__(replica, resolution, (('crf_joint',) if upsample is not None else ()) +
                         (('crf_cond', 'crf_hidden') if condition is not None else ()), (replica.rows, replica.cols),
                         min_depth, max_depth, clamp_lo, clamp_hi, keep_predictions, align)
        self.upsample, self.condition = upsample, condition
        if condition is not None:
            self.z2_sum, self.z2_n, self.measured, self.rejected = 0.0, 0, 0, 0
        self.observed = (float(min_depth), float(max_depth)) if observed_nll else None
        self.onll, self.nobs = [], []
        self.nll, self.status = [], []

    def __call__(self, images, depths, n):
        rep = self.rep
        unary, crf = rep.predict(images, n)
        self.nll.append(rep.nll(depths, n))                                      # the mean over these n images
        target = rep.depths240[:n] if self.resolution == 'grid' else depths[:n]
        for name, out in zip(OUTPUTS['dcnf'], (unary, crf)):
            self.judge(name, rep.depth_map(out) if rep.slic else out, n, target)     # a label map has no grid to sample
        if self.upsample is not None:
            self.judge('crf_joint', self.upsample(crf[:n], images[:n]), n, target)
        self.status.append(rep.status[:n].clone())
        self.counts.append(n)
        if self.predictions is not None:
            self.predictions.append(crf[:n].clone())
        if self.observed is not None:
            self.onll.append(rep.nll(depths, n, valid_range=self.observed))
            self.nobs.append(rep.nobs.sum().reshape(1))
        if self.condition is not None:
            self._condition(crf, depths, n, int(sum(self.counts)) - n)

    def _condition(self, crf, depths, n, first):
        """Hide target superpixels from the field, complete them, judge the completion and the MAP on their pixels."""
        rep = self.rep
        keep_p, seed = self.condition
        keep = np.stack([np.random.default_rng([int(seed), first + k]).random(rep.nsp) < keep_p for k in range(n)])
        keep_d = torch.from_numpy(keep).to(rep.device)
        mean, var = rep.posterior(None, depths, n, (self.kw['min_depth'], self.kw['max_depth']), keep=keep_d)
        sp = rep.sp
        kept_pixels = keep_d.view(n, rep.rows, rep.cols).repeat_interleave(sp, 1).repeat_interleave(sp, 2)
        target = rep.depths240[:n].clone()                       # the validity-aware resize: NaN where nothing was measured
        target.view(n, target.shape[1], target.shape[2])[kept_pixels] = self.kw['min_depth']
        self.judge('crf_cond', mean, n, target)
        self.judge('crf_hidden', crf, n, target)
        y = rep.y.view(rep.B, rep.nsp)[:n].double().cpu().numpy()
        m, v = (t[:n].reshape(n, rep.nsp).double().cpu().numpy() for t in (mean, var))
        bad = rep.status[:n].cpu().numpy() != 0
        hidden = np.isfinite(y) & ~keep & ~bad[:, None]
        self.rejected += int(bad.sum())
        self.measured += int((np.isfinite(y) & ~bad[:, None]).sum())
        self.z2_n += int(hidden.sum())
        self.z2_sum += float((((y - m) ** 2)[hidden] / v[hidden]).sum())

    def results(self):
        out = super().results()
        out['crf_nll'] = self.mean(self.nll)
        out['singular_systems'] = int(torch.cat(self.status).sum().item())
        if self.observed is not None:
            out['observed_nll'] = self.mean(self.onll)
            out['observed_fraction'] = float(torch.cat(self.nobs).sum().item() / (sum(self.counts) * self.rep.nsp))
        if self.condition is not None:
            out['condition_z2'] = self.z2_sum / self.z2_n if self.z2_n else float('nan')
            out['hidden_fraction'] = self.z2_n / self.measured if self.measured else float('nan')
            out['rejected_systems'] = self.rejected
        return out


def find_checkpoint(args, run_dir):
    if args.checkpoint:
        path = args.checkpoint
        return path if (os.path.isfile(path) or tfckpt.is_bundle(path)) else None
    return latest_checkpoint(run_dir)


def current_gpu(what):
    if not torch.cuda.is_available():
        raise RuntimeError(f'ann3depth_amd needs an MI355X: {what} has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def restore_replica(args, ckpt, say, dev=None):
    """The replica of args.model (msdn, dcnf) at args.batchsize / args.precision / args.superpixel with the weights of
    checkpoint `ckpt` (a .pt file or a TF bundle prefix; ann3depth.read_checkpoint, load_checkpoint): (replica, texture,
    unary), the last two what a dcnf checkpoint says about its own form.  None, after say(why), for a checkpoint this
    model and --superpixel cannot use.  dev: the GPU to restore to; None (the prediction driver) reads the checkpoint on
    the host and asks for the current GPU only once nothing is left to refuse."""
    from .models import (DCNF_PAIR_PREFIX, DCNF_PREFIX, DCNFReplica, MSDNReplica, check_dcnf_segmentation,
                         check_dcnf_superpixel, checkpoint_optimizer)
    say(f'restoring {ckpt}')
    state, bundle = read_checkpoint(ckpt, 'cpu' if dev is None else dev)
    texture, unary = False, 'patch'
    if args.model == 'dcnf':
        # the checkpoint says how many similarities its pairwise layer weighs: 2, or 3 with --pairwise-texture
        name = DCNF_PAIR_PREFIX + 'kernel'
        shape = tuple(np.shape(state[name])) if name in state else None
        if shape not in ((2, 1), (3, 1)):
            say(f'{ckpt}: {name} has shape {None if shape is None else list(shape)}; a dcnf checkpoint holds a [2, 1] '
                f'kernel, or a [3, 1] one when it was trained with --pairwise-texture.')
            return None
        texture = shape == (3, 1)
        # ... and which form its unary part has: dense/kernel is [256, 128] with --unary fcsp, [12544, 128] without
        dense = DCNF_PREFIX + 'dense/kernel'
        unary = 'fcsp' if dense in state and tuple(np.shape(state[dense])) == (256, 128) else 'patch'
        try:
            check_dcnf_superpixel(args.superpixel, unary, None)
        except ValueError as e:
            say(f'{ckpt}: a checkpoint of the patch form; {e}.')
            return None
        try:
            check_dcnf_segmentation(args.segmentation, unary, texture, None, args.slic_iters, args.slic_compactness)
        except ValueError as e:
            say(f'{ckpt}: a checkpoint of --unary {unary}{" --pairwise-texture" if texture else ""}; {e}.')
            return None
    if dev is None:
        dev = current_gpu('prediction')
    if args.model == 'dcnf':
        replica = DCNFReplica(args.batchsize, device=dev, precision=args.precision, pairwise_texture=texture, unary=unary,
                              superpixel=args.superpixel, segmentation=args.segmentation, slic_iters=args.slic_iters,
                              slic_compactness=args.slic_compactness)
    else:
        # the checkpoint says which optimizer's slots it holds: a run of --optimizer momentum restores with no flag
        replica = MSDNReplica(args.batchsize, device=dev, precision=args.precision, keep_dense_grads=False,
                              optimizer=checkpoint_optimizer(state))
    load_checkpoint(replica, state, bundle)
    return replica, texture, unary


def refuse_model(args, say, can, own=lambda: None):
    """The opening of both inference drivers' main(), first half: 2 after say(why) for an unknown model, for what own()
    refuses (the driver's own refusal that comes next in its order; it says why itself) and for --superpixel without dcnf."""
    if args.model not in OUTPUTS:
        say(f'unknown model {args.model!r}; msdn and dcnf {can}.')
        return 2
    if own():
        return 2
    if args.superpixel != 40 and args.model != 'dcnf':
        say(f'--superpixel {args.superpixel} sets the grid of the CRF of --model dcnf: {args.model} has no superpixels.')
        return 2
    if args.segmentation != 'grid' and args.model != 'dcnf':
        say(f'--segmentation {args.segmentation} chooses the superpixels of the CRF of --model dcnf: {args.model} has no '
            f'superpixels.')
        return 2


def refuse_under_slic(args, say, flags):
    """2 after say(why) when --segmentation slic meets one of `flags`, (flag text, given?) pairs of what a driver cannot do
    on a label map yet, or --slic-iters / --slic-compactness outside their range; before any GPU work."""
    if args.segmentation != 'slic':
        return None
    for flag, given in flags:
        if given:
            say(f'--segmentation slic cannot go with {flag} yet: it reads the square blocks of the grid, and its form on a '
                f'label map is a later change.')
            return 2
    if args.slic_iters < 0 or not 0 <= args.slic_compactness < float('inf'):
        say(f'--slic-iters {args.slic_iters} must be >= 0 and --slic-compactness {args.slic_compactness} finite and >= 0.')
        return 2


def open_checkpoint(args, say, noun, refusing, own=lambda: None):
    """... second half, after the driver's own flags: (upsample, run_dir, ckpt), the ops.JointUpsampler of --upsample joint
    or None, <ckptdir>/<model>_<id> and the checkpoint to restore; or 2 after say(why), own() as in refuse_model."""
    upsample = None
    if args.upsample == 'joint':
        try:
            upsample = ops.JointUpsampler('block' if args.model == 'dcnf' else 'corner',
                                          args.superpixel if args.model == 'dcnf' else None, args.radius, args.sigma_space,
                                          args.sigma_range)
        except ValueError as e:
            say(f'--upsample joint: {e}.')
            return 2
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        say(f'{noun} runs in one process on one GPU; start it without a distributed launcher.')
        return 2
    if own():
        return 2
    run_dir = os.path.join(args.ckptdir, args.model + ('' if not args.id else f'_{args.id}'))
    ckpt = find_checkpoint(args, run_dir)
    if not ckpt:
        say(f'no checkpoint found ({args.checkpoint or run_dir}); refusing to {refusing}.')
        return 2
    return upsample, run_dir, ckpt


def main(argv=None):
    args = parse_args(argv)

    def observed_nll_without_dcnf():
        if args.observed_nll and args.model != 'dcnf':
            _say('--observed-nll is the held-out objective of a dcnf run trained with --min-depth / --max-depth.')
            return 2

    if refuse_model(args, _say, 'can be evaluated', observed_nll_without_dcnf):
        return 2
    if args.superpixel != 40 and args.observed_nll:
        _say(f'--superpixel {args.superpixel} cannot go with --observed-nll yet: the likelihood of the observed superpixels '
             f'alone exists only for the dense 6 x 8 CRF (--superpixel 40).')
        return 2
    if refuse_under_slic(args, _say, (('--upsample joint', args.upsample == 'joint'), ('--observed-nll', args.observed_nll),
                                      ('--condition', args.condition is not None))):
        return 2
    loss = 'berhu' if args.berhu_fraction is not None else args.loss         # its own flag speaks for --loss berhu
    if loss in EXTRA_LOSSES and args.model != 'msdn':
        _say(f'--loss {loss} reports {EXTRA_LOSSES[loss].phrase} of the two outputs of --model msdn: {args.model} has no loss '
             f'over a pixel grid.')
        return 2
    if args.berhu_fraction is not None and (args.loss != 'berhu' or not 0 < args.berhu_fraction <= 1):
        _say(f'--berhu-fraction {args.berhu_fraction} sets the threshold of --loss berhu, a fraction in (0, 1] of the largest error.')
        return 2
    if args.condition is not None:
        if args.model != 'dcnf':
            _say('--condition hides superpixels from the CRF of --model dcnf; msdn has no field to condition.')
            return 2
        if args.resolution != 'grid' or not 0 < args.condition < 1:
            _say(f'--condition {args.condition} needs --resolution grid (the superpixels tile the 240 x 320 target) and '
                 f'0 < KEEP < 1.')
            return 2
    opened = open_checkpoint(args, _say, 'evaluation', 'evaluate untrained weights')
    if opened == 2:
        return 2
    upsample, run_dir, ckpt = opened
    try:
        inputs, _ = data.inputs(args.datadir, args.dataset, args.batchsize, train_or_test='test', shuffle=False)
    except FileNotFoundError as e:
        _say(f'no test split: {e} is missing.')
        return 2
    dev = current_gpu('evaluation')
    restored = restore_replica(args, ckpt, _say, dev)
    if restored is None:
        inputs.pipeline.close()
        return 2
    replica, texture, unary = restored
    step = replica.global_step
    pipeline = inputs.pipeline
    evaluator = DCNFEvaluator if args.model == 'dcnf' else Evaluator
    extra = {'observed_nll': True} if args.observed_nll else {}
    if upsample is not None:
        extra['upsample'] = upsample
    if args.condition is not None:
        extra['condition'] = (args.condition, args.condition_seed)
    loss_kw = EXTRA_LOSSES[args.loss].keywords(args) if args.loss in EXTRA_LOSSES else {}
    extra.update(loss_kw)
    if args.align != 'none':
        extra['align'] = args.align
    ev = evaluator(replica, args.resolution, args.min_depth, args.max_depth, args.clamp_lo, args.clamp_hi,
                   keep_predictions=bool(args.predictions), **extra)
    op = EvalOp(pipeline, args.batchsize, dev)
    try:
        while True:
            try:
                op.run(ev)
            except data.OutOfRangeError:
                break
    finally:
        pipeline.close()
    res = ev.results()
    records = int(sum(ev.counts))
    out = {'checkpoint': ckpt, 'global_step': step, 'dataset': args.dataset, 'records': records,
           'resolution': args.resolution, 'precision': args.precision,
           'min_depth': args.min_depth, 'max_depth': args.max_depth, 'clamp_lo': args.clamp_lo, 'clamp_hi': args.clamp_hi,
           **res}
    if texture:
        out['pairwise_texture'] = True
    if unary != 'patch':
        out['unary_form'] = unary          # ('unary' holds the metrics of the unary output)
    if args.model == 'dcnf':
        out['superpixel'] = args.superpixel
    if args.segmentation != 'grid':
        out.update(segmentation=args.segmentation, slic_iters=args.slic_iters, slic_compactness=args.slic_compactness)
    if upsample is not None:
        out.update(upsample='joint', radius=upsample.radius, sigma_space=upsample.sigma_space,
                   sigma_range=upsample.sigma_range)
    if args.condition is not None:
        out.update(condition=args.condition, condition_seed=args.condition_seed)
    if args.loss in EXTRA_LOSSES:
        out.update(loss=args.loss, **(loss_kw if EXTRA_LOSSES[args.loss].reported else {}))
    if args.align != 'none':
        out['align'] = args.align
    if args.predictions:
        np.save(args.predictions, torch.cat(ev.predictions).cpu().numpy() if ev.predictions else
                np.zeros((0,) + ev.prediction_shape, np.float32))
    os.makedirs(run_dir, exist_ok=True)
    with open(os.path.join(run_dir, f'eval-{step}.json'), 'w') as f:
        json.dump(out, f, indent=1)
    events = summary.EventFileWriter(run_dir)
    scalars = {f'eval/{o}/{k}': float(v) for o in ev.outputs + ev.aligned for k, v in res[o].items()}
    if 'condition_z2' in res:
        scalars['eval/condition_z2'] = res['condition_z2']
    if 'crf_nll' in res:
        scalars['eval/crf_nll'] = res['crf_nll']
    if 'observed_nll' in res:
        scalars['eval/observed_nll'] = res['observed_nll']
    events.add_scalars(step, scalars)
    events.close()
    print(json.dumps(out), flush=True)
    return 0


def parse_args(argv=None):
    """The training driver's flags that apply to evaluation (src/ann3depth.py:221-254), plus the evaluation's own."""
    p = argparse.ArgumentParser(
        description='Evaluate an MSDN or DCNF checkpoint on <datadir>/<dataset>/test.tfrecords.')
    p.add_argument('dataset', default='nyu', type=str, help='The dataset to use.')
    add_shared_args(p, 'model', 'batchsize', 'ckptdir', 'id')
    p.add_argument('--datadir', '-d', default='data', type=str, help='The data directory containing the datasets.')
    add_shared_args(p, 'precision', 'checkpoint')
    p.add_argument('--resolution', default='grid', choices=['grid', 'record'],
                   help='grid: targets resized as the training step does (msdn 55x74, dcnf 240x320); record: the depth '
                        'map as stored.  A prediction on another grid than the target is resampled at its pixels.')
    p.add_argument('--min-depth', default=0., type=float, help='Valid targets are > this.')
    p.add_argument('--max-depth', default=float('inf'), type=float, help='Valid targets are <= this.')
    p.add_argument('--clamp-lo', default=1e-3, type=float, help='Predictions are clamped to at least this.')
    p.add_argument('--clamp-hi', default=float('inf'), type=float, help='Predictions are clamped to at most this.')
    p.add_argument('--observed-nll', action='store_true',
                   help='NON-REFERENCE, dcnf: also report observed_nll, the objective of a run trained with --min-depth / '
                        '--max-depth (the likelihood of the superpixels those two thresholds leave observed), and the share '
                        'of superpixels it counted.')
    p.add_argument('--predictions', default='', type=str,
                   help='Write the fine (msdn, [N,55,74]) or crf (dcnf, [N,6,8]; [N,12,16] or [N,24,32] with --superpixel 20 or '
                        '10) predictions to this .npy.')
    add_shared_args(p, 'superpixel',
                    superpixel='NON-REFERENCE unless 40, dcnf: the edge of the superpixels the checkpoint is evaluated at (6 x 8, '
                               '12 x 16 or 24 x 32 depths per image). Checkpoints hold no grid: one trained at 40 evaluates at 10 '
                               'and the reverse. 20 and 10 need a checkpoint of --unary fcsp; crf_nll is then the banded '
                               'likelihood, not comparable with the value at 40.')
    p.add_argument('--condition', default=None, type=float, metavar='KEEP',
                   help='NON-REFERENCE, dcnf, --resolution grid: judge depth completion. Each target superpixel is kept with '
                        'probability KEEP (0 < KEEP < 1), the field is conditioned on the kept ones, and crf_cond (completed) '
                        'and crf_hidden (the plain MAP) are judged on the pixels of the hidden ones.')
    p.add_argument('--condition-seed', default=0, type=int,
                   help='--condition: the masks are drawn on the host from (this seed, the record\'s index).')
    # NON-REFERENCE, msdn: --loss berhu [--berhu-fraction F], --loss ssi (see the module docstring).  Kept out of --help like --segmentation:
    # this driver's help text is recorded word for word (tests/golden/evaluate_help.txt).
    p.add_argument('--loss', default='silog', choices=['silog', 'berhu', 'ssi'], help=argparse.SUPPRESS)
    p.add_argument('--berhu-fraction', default=None, type=float, metavar='F', help=argparse.SUPPRESS)
    add_shared_args(p, 'segmentation')
    # NON-REFERENCE: --align (see the module docstring), kept out of --help for the same reason
    p.add_argument('--align', default='none', choices=['none'] + list(ops.ALIGN_MODES), help=argparse.SUPPRESS)
    add_upsample_args(p, ['none', 'joint'], 'none',
                      'NON-REFERENCE: joint also judges a third output, fine_joint (msdn) or crf_joint (dcnf): the prediction '
                      'brought to the record image\'s size by joint bilateral upsampling under the image '
                      '(ops.joint_bilateral_upsample), against the same target as the other outputs.')
    return p.parse_args(argv)


def add_shared_args(p, *names, **text):
    """The flags both inference drivers take, in the order `names` gives them (each driver's --help interleaves its own
    flags); text: the help strings that differ between the two, by flag name."""
    shared = {
        'model': (('--model', '-m'), dict(default='msdn', type=str, help='Model name (msdn, dcnf).')),
        'batchsize': (('--batchsize', '-b'), dict(default=32, type=int, help='Batchsize')),
        'ckptdir': (('--ckptdir', '-p'), dict(default='checkpoints', help='Checkpoint directory')),
        'id': (('--id',), dict(default='', type=str, help='Checkpoint path suffix.')),
        'checkpoint': (('--checkpoint',), dict(default='', type=str, help='A .pt file or TF bundle prefix instead of the newest '
                                                                         'checkpoint of <ckptdir>/<model>_<id>.')),
        'precision': (('--precision',), dict(default='fp32', choices=['fp32', 'bf16x3', 'bf16', 'bf16s'],
                                             help='Arithmetic of the conv contractions, as in training.')),
        'superpixel': (('--superpixel',), dict(default=40, type=int, choices=[40, 20, 10])),
    }
    for name in names:
        if name == 'segmentation':                  # --segmentation, --slic-iters, --slic-compactness: the training driver's
            add_segmentation_args(p, listed=False)
            continue
        flags, kw = shared[name]
        p.add_argument(*flags, **dict(kw, **({'help': text[name]} if name in text else {})))


def add_upsample_args(p, choices, default, text):
    """--upsample and the three parameters of the joint bilateral filter, shared with the prediction driver."""
    p.add_argument('--upsample', default=default, choices=choices, help=text)
    p.add_argument('--radius', default=ops.UPSAMPLE_RADIUS, type=int,
                   help=f'--upsample joint: cells around a pixel that count, 1 .. {ops.UPSAMPLE_MAX_RADIUS} (a window of '
                        f'(2 radius + 1)^2).')
    p.add_argument('--sigma-space', default=ops.UPSAMPLE_SIGMA_SPACE, type=float,
                   help='--upsample joint: width of the distance weight, in cells of the prediction.')
    p.add_argument('--sigma-range', default=ops.UPSAMPLE_SIGMA_RANGE, type=float,
                   help='--upsample joint: width of the colour weight, in units of the [0, 1] colour range; inf: distance only.')


if __name__ == '__main__':
    sys.exit(main())
