"""Driver — the surface of the reference's ``src/ann3depth.py``: same flags (src/ann3depth.py:221-254), same
checkpoint directory convention, same stop conditions, same exit code, same one-line hot loop
``while not should_stop: run(train_op)`` (src/ann3depth.py:126-127).

TensorFlow's session machinery is not reproduced: `Session` below is the minimal stand-in for
`MonitoredTrainingSession` + the reference's hooks (StopAtStepHook, StopAtSignalHook, summary saver,
checkpoint saver/restorer, TraceHook).  The parameter-server path (`--job-name ps`, src/ann3depth.py:62-67) is
replaced by synchronous RCCL data parallelism: launch one process per GPU with
``python -m torch.distributed.run --nproc-per-node N -m ann3depth_amd.ann3depth ...``; the old cluster flags are
accepted and ignored.

Flags that are not the reference's: --beta2, --precision, --augment, --min-depth / --max-depth, --loss-gradient,
--loss {silog,berhu,ssi}, --berhu-fraction, --optimizer {adam,momentum}, --momentum, --lr-scale, --clip-norm,
--train-pairwise, --pairwise-texture, --superpixel {40,20,10}, --unary {patch,fcsp} (dcnf: the unary part over 48 patches per image, the
reference's, or once over the whole image with superpixel pooling before the dense head), --seed, --tf-checkpoints,
--trace-every, --profiler.
"""
import argparse
import json
import logging
import logging.config
import os
import signal
import sys
import time

import torch

from . import _lib, augment, data, dp, models, summary, tfckpt, tracehook

# --loss NAME other than silog: what a refusal calls it
LINEAR_LOSSES = {'berhu': 'the reverse Huber loss', 'ssi': 'the scale-and-shift-invariant loss'}


def main(argv=None):
    ini = 'logging.ini' if os.path.exists('logging.ini') else os.path.join(os.path.dirname(__file__), 'logging.ini')
    logging.config.fileConfig(ini, disable_existing_loggers=False)
    logger = logging.getLogger('ann3depth')

    args = parse_args(argv)
    logger.debug(args)
    logger.info(f'This is a {args.job_name} with index {args.task_index}')
    if args.cluster_spec:
        logger.info(f'Ignoring cluster spec {args.cluster_spec}: replicas are RCCL ranks, not TF servers.')
    else:
        logger.info('Using default local cluster spec.')

    if args.job_name == 'ps':
        logger.info('Parameter servers do not exist in this build (gradients are all-reduced over xGMI).')
        return 0
    if args.job_name not in ('worker', 'local'):
        logger.warning(f'No suitable job description found! {args.job_name}')
        return 0
    if args.augment != 'none' and args.model != 'msdn':
        logger.error(f'--augment {args.augment} is the augmentation of Eigen et al. 2014 and applies to --model msdn only: '
                     f'{args.model or "(no model)"} is not trained with it (dcnf computes its pairwise features from the '
                     f'resized image, and the paper behind it does not augment this way).')
        return 2
    if (args.min_depth is not None or args.max_depth is not None) and not hasattr(getattr(models, args.model, None),
                                                                                  'valid_range'):
        logger.error(f'--min-depth / --max-depth keep the holes of a depth map out of the targets of msdn and dcnf: '
                     f'{args.model or "(no model)"} is not trained with them.')
        return 2
    if args.model == 'dcnf' and (args.min_depth is None) != (args.max_depth is None):
        logger.error('--model dcnf takes --min-depth and --max-depth together: its targets are means over 1600 pixels, the '
                     'data sets it is reported on have holes at both ends of the range (no return and the range cap), and '
                     'the kind a one-sided range lets through would be averaged into every superpixel it touches.')
        return 2
    if args.train_pairwise and not hasattr(getattr(models, args.model, None), 'train_pairwise'):
        logger.error(f'--train-pairwise learns the pairwise weights of the CRF of --model dcnf (Liu et al. 2015): '
                     f'{args.model or "(no model)"} has no such layer.')
        return 2
    if args.pairwise_texture and not hasattr(getattr(models, args.model, None), 'pairwise_texture'):
        logger.error(f'--pairwise-texture adds the texture similarity to the pairwise part of the CRF of --model dcnf '
                     f'(Liu et al. 2015): {args.model or "(no model)"} has no such part.')
        return 2
    if args.unary != 'patch' and not hasattr(getattr(models, args.model, None), 'unary'):
        logger.error(f'--unary {args.unary} chooses the form of the unary part of --model dcnf (Liu et al. 2015, DCNF-FCSP): '
                     f'{args.model or "(no model)"} has no such part.')
        return 2
    if args.superpixel != models.DCNF_SP:
        if not hasattr(getattr(models, args.model, None), 'superpixel'):
            logger.error(f'--superpixel {args.superpixel} sets the grid of the CRF of --model dcnf: '
                         f'{args.model or "(no model)"} has no superpixels.')
            return 2
        try:
            models.check_dcnf_superpixel(args.superpixel, args.unary,
                                         None if args.min_depth is None and args.max_depth is None else (0, 0))
        except ValueError as e:
            logger.error(f'--superpixel {args.superpixel}: {e}.')
            return 2
    if args.segmentation != 'grid':
        if not hasattr(getattr(models, args.model, None), 'segmentation'):
            logger.error(f'--segmentation {args.segmentation} chooses the superpixels of the CRF of --model dcnf: '
                         f'{args.model or "(no model)"} has no superpixels.')
            return 2
        try:
            models.check_dcnf_segmentation(args.segmentation, args.unary, args.pairwise_texture,
                                           None if args.min_depth is None and args.max_depth is None else (0, 0),
                                           args.slic_iters, args.slic_compactness)
        except ValueError as e:
            logger.error(f'{e}.')
            return 2
    if args.loss_gradient is not None and args.model != 'msdn':
        logger.error(f'--loss-gradient weighs the gradient-matching term of Eigen & Fergus 2015 in the two losses of --model '
                     f'msdn: {args.model or "(no model)"} has no loss over a pixel grid (dcnf regresses superpixel means).')
        return 2
    if args.loss_gradient is not None and not args.loss_gradient >= 0:
        logger.error(f'--loss-gradient {args.loss_gradient}: the weight is a number >= 0.')
        return 2
    if args.loss in LINEAR_LOSSES and args.model != 'msdn':
        logger.error(f'--loss {args.loss} is {LINEAR_LOSSES[args.loss]} on the linear depths of --model msdn: '
                     f'{args.model or "(no model)"} has no loss over a pixel grid (dcnf regresses superpixel means through a '
                     f'likelihood).')
        return 2
    if args.loss in LINEAR_LOSSES and args.loss_gradient is not None:
        logger.error(f'--loss {args.loss} cannot go with --loss-gradient: the gradient-matching term is defined on differences of '
                     f'log depth and belongs to --loss silog.')
        return 2
    if args.berhu_fraction is not None and args.loss != 'berhu':
        logger.error(f'--berhu-fraction sets the threshold of --loss berhu; --loss {args.loss} has none.')
        return 2
    if args.berhu_fraction is not None and not 0 < args.berhu_fraction <= 1:
        logger.error(f'--berhu-fraction {args.berhu_fraction}: the threshold is a fraction in (0, 1] of the largest error.')
        return 2
    given = [f for f, on in (('--optimizer', args.optimizer != 'adam'), ('--momentum', args.momentum is not None),
                             ('--lr-scale', args.lr_scale is not None)) if on]
    if given and args.model != 'msdn':
        logger.error(f'{" / ".join(given)} choose the optimizer and the rates of --model msdn (Eigen et al. 2014 trained it by SGD '
                     f'with momentum): {args.model or "(no model)"} is not trained with them (dcnf descends by plain gradient '
                     f'descent at 0.1, as the reference does).')
        return 2
    if args.optimizer == 'momentum' and args.beta2 is not None:
        logger.error('--optimizer momentum cannot go with --beta2: beta2 belongs to --optimizer adam.')
        return 2
    if args.momentum is not None and args.optimizer != 'momentum':
        logger.error(f'--momentum sets the momentum of --optimizer momentum; --optimizer {args.optimizer} has none.')
        return 2
    if args.momentum is not None and not 0 <= args.momentum < 1:
        logger.error(f'--momentum {args.momentum}: a number in [0, 1).')
        return 2
    if args.lr_scale is not None and not 0 < args.lr_scale < float('inf'):
        logger.error(f'--lr-scale {args.lr_scale}: a finite number > 0.')
        return 2
    if args.clip_norm is not None:
        if not hasattr(getattr(models, args.model, None), 'clip_norm'):
            logger.error(f'--clip-norm bounds the gradient norm of every optimizer group of --model msdn or dcnf: '
                         f'{args.model or "(no model)"} has no optimizer group.')
            return 2
        try:
            models.check_clip_norm(args.clip_norm)
        except ValueError:
            logger.error(f'--clip-norm {args.clip_norm}: a number > 0 (inf: measure the norms and skip non-finite steps, never '
                         f'clip).')
            return 2
    if args.min_depth is not None or args.max_depth is not None:
        lo = 0. if args.min_depth is None else args.min_depth
        hi = float('inf') if args.max_depth is None else args.max_depth
        if not lo <= hi:
            logger.error(f'--min-depth {lo} --max-depth {hi}: need min <= max.')
            return 2

    run_id = args.model + ('' if not args.id else f'_{args.id}')
    ckptdir = str(os.path.join(args.ckptdir, run_id))                    # src/ann3depth.py:73-75
    if args.profiler == 'rocprofv3' and args.trace_every and not tracehook.under_profiler():
        # TraceHook as a profiler capture: nothing above has touched the GPU, so this process may still start the
        # profiled copy of itself as a child; from here on it only waits (ann3depth_amd/tracehook.py)
        out = os.path.join(ckptdir, 'rocprof')
        logger.info(f'Starting the training process under rocprofv3; traces of the traced steps go to {out}.')
        return tracehook.respawn(sys.argv[1:] if argv is None else argv, out)

    rank, local_rank, world = dp.init_from_env()
    if not torch.cuda.is_available():
        raise RuntimeError('ann3depth_amd needs an MI355X: the training path has no CPU fallback')
    torch.cuda.set_device(local_rank % torch.cuda.device_count())
    chief = rank == 0
    logger.info(f'Task: {rank} of {world} -- Chief? {chief}')

    logger.info(f'Checkpoint dir is {ckptdir}.')

    logger.info(f'Loading model {args.model}.')
    model_op = setup_model(args, rank, world)

    size_train = sum(g.count for g in model_op.replica.groups.values()) * 4 / 1024 / 1024
    logger.debug(f'Trainable variables have about {size_train:.1f} MB')

    logger.info('Setting up hooks.')
    stop_at_signal = StopAtSignal()
    if args.job_name != 'local':
        logger.info(f'Starting alarm: {args.timeout} s timeout.')
        signal.alarm(args.timeout)                                       # src/ann3depth.py:108-110

    logger.info('Starting session.')
    with Session(model_op, ckptdir if chief else None, last_step=args.steps, stop_at_signal=stop_at_signal,
                 save_checkpoint_secs=args.ckptfreq, save_summaries_steps=args.sumfreq,
                 trace_every=args.trace_every, logger=logger, world=world,
                 tf_checkpoints=args.tf_checkpoints) as session:
        while not session.should_stop():
            session.run(model_op)
    logger.info('Session stopped.')
    return stop_at_signal.signal_received                                # src/ann3depth.py:129


def setup_model(args, rank=0, world=1):
    """src/ann3depth.py:134-145."""
    model = getattr(models, args.model)
    if world > 1:
        model.reducer = dp.GradReducer()
    if args.beta2 is not None:
        model.beta2 = args.beta2
    model.precision = args.precision
    if hasattr(model, 'augment'):                                        # main() has refused the models that have none
        model.augment = augment.Eigen2014() if args.augment == 'eigen' else None
    if hasattr(model, 'valid_range'):
        model.valid_range = None
        if args.min_depth is not None or args.max_depth is not None:
            model.valid_range = (0. if args.min_depth is None else args.min_depth,
                                 float('inf') if args.max_depth is None else args.max_depth)
    if hasattr(model, 'grad_weight'):                                    # main() has refused the models that have none
        model.grad_weight = float(args.loss_gradient or 0.0)
    if hasattr(model, 'objective'):                                      # main() has refused the models that have none
        model.objective = args.loss
        model.berhu_fraction = 0.2 if args.berhu_fraction is None else float(args.berhu_fraction)
    if hasattr(model, 'optimizer'):                                      # main() has refused the models that have none
        model.optimizer = args.optimizer
        model.momentum = 0.9 if args.momentum is None else float(args.momentum)
        model.lr_scale = 1.0 if args.lr_scale is None else float(args.lr_scale)
    if hasattr(model, 'clip_norm'):                                      # main() has refused the models that have none
        model.clip_norm = args.clip_norm
    if hasattr(model, 'train_pairwise'):                                 # main() has refused the models that have none
        model.train_pairwise = bool(args.train_pairwise)
    if hasattr(model, 'pairwise_texture'):
        model.pairwise_texture = bool(args.pairwise_texture)
    if hasattr(model, 'unary'):
        model.unary = args.unary
    if hasattr(model, 'superpixel'):
        model.superpixel = args.superpixel
    if hasattr(model, 'segmentation'):                                   # main() has refused the models that have none
        model.segmentation, model.slic_iters, model.slic_compactness = (args.segmentation, args.slic_iters,
                                                                        args.slic_compactness)
    inputs, targets = data.inputs(args.datadir, args.dataset, args.batchsize, rank=rank, world=world,
                                  seed=args.seed + rank)
    return model(inputs, targets)


class StopAtSignal:
    """tfhelper.StopAtSignalHook (src/tfhelper.py:160-189): remember the signal, stop after the current step."""

    def __init__(self, signals=None):
        self.signal_received = 0
        if signals is None:
            signals = [signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM]
        for s in signals:
            signal.signal(s, self._handler)

    def _handler(self, signum, frame):
        self.signal_received = signum


class Session:
    """Stand-in for tf.train.MonitoredTrainingSession as the reference configures it (src/ann3depth.py:113-125):
    restore the newest checkpoint of `checkpoint_dir`, save every `save_checkpoint_secs` and on exit, write loss
    scalars every `save_summaries_steps` steps, log steps/sec, stop at `last_step`, on a signal, or when the input
    pipeline runs dry."""

    def __init__(self, train_op, checkpoint_dir, last_step, stop_at_signal, save_checkpoint_secs, save_summaries_steps,
                 trace_every, logger, world=1, tf_checkpoints=False, keep_checkpoints=5):
        self.keep_checkpoints = keep_checkpoints          # tf.train.Saver(max_to_keep=5), the Saver default
        self.op, self.dir, self.last_step, self.sig = train_op, checkpoint_dir, last_step, stop_at_signal
        self.ckpt_secs, self.sum_steps, self.trace_every = save_checkpoint_secs, save_summaries_steps, trace_every
        self.log, self.world = logger, world
        self.tf_checkpoints = tf_checkpoints
        self.stop = False
        self.trace_next = True               # TraceHook: the first step after every (re)start is traced
        # under `--profiler rocprofv3` (this is then the profiled child): the traced steps are the profiler's regions
        self.roctx = tracehook.Roctx() if tracehook.under_profiler() else None
        self.t_last_ckpt = time.time()
        self.t_last_sum, self.step_last_sum = time.time(), None
        self.summaries = None
        self.events = None

    def __enter__(self):
        rep = self.op.replica
        latest = latest_checkpoint(self.dir) if self.dir else None
        if latest:
            self.log.info(f'Restoring {latest}')
            try:
                load_checkpoint(rep, *read_checkpoint(latest, rep.device))
            except ValueError:                                # refused (dcnf: a [2,1] / [3,1] pairwise kernel across
                self.op.pipeline.close()                      # --pairwise-texture, a dense/kernel across --unary): no __exit__
                raise
        if self.world > 1:                                    # non-chief replicas take the chief's state
            import torch.distributed as dist
            rep.broadcast_state(dist, 0)
        if self.dir:
            os.makedirs(self.dir, exist_ok=True)
            self.summaries = open(os.path.join(self.dir, 'summaries.jsonl'), 'a')
            self.events = summary.EventFileWriter(self.dir)
        self.step_last_sum = rep.global_step
        if self.world > 1:
            # before the first step: a rank whose shard cannot fill even one batch (or whose reader already failed) must
            # not leave the others waiting in step 1's collectives
            self._decide(self.op)
        return self

    def _decide(self, train_op, want_save=False):
        """The replicas decide TOGETHER (dp.GradReducer.agree_all, one host collective): a signal reaches the ranks at
        different steps, an input shard runs dry on one rank first, the chief's checkpoint timer fires on the chief only —
        and the next step's collectives (and a sharded optimizer state's gather) need everyone.  Agreed values: the
        signal number (exit code of every rank, src/ann3depth.py:129) or 1 when a rank's input has no batch left for
        the next step; whether a rank's reader FAILED (CRC mismatch, malformed record: raised on every rank, never
        mistaken for a clean end of input); whether the chief wants a checkpoint now."""
        rep = train_op.replica
        due = train_op.feed.due()
        dry = isinstance(due, data.OutOfRangeError)
        failed = due is not None and not dry
        stop, err, save = rep.reducer.agree_all([self.sig.signal_received or (1 if dry else 0), int(failed),
                                                 int(want_save)])
        if err:
            if failed:
                raise due
            raise RuntimeError('the input pipeline of another replica failed; stopping with it')
        if stop:
            self.stop = True
            if stop > 1 and not self.sig.signal_received:
                self.sig.signal_received = stop
        return bool(save)

    def should_stop(self):
        return self.stop or self.op.replica.global_step >= self.last_step

    def run(self, train_op):
        rep = train_op.replica
        tracing = self.trace_next and self.dir is not None
        marking = self.trace_next and self.roctx is not None
        if tracing:
            _lib.load().a3d_timing_enable(1)
        if marking:
            self.roctx.begin(rep.global_step + 1)
        try:
            out = train_op.run()
        except data.OutOfRangeError as e:
            self.log.info(f'Input pipeline exhausted: {e}')
            self.stop = True
            return None
        finally:
            if marking:
                torch.cuda.synchronize()               # the step's kernels belong inside the region
                self.roctx.end()
            if tracing:
                self._write_trace(rep.global_step)
        step = rep.global_step
        # tfhelper.TraceHook (src/tfhelper.py:192-249): trace the first step and every `trace_every`-th global step
        self.trace_next = bool(self.trace_every) and (step + 1) % self.trace_every == 0
        save_due = bool(self.dir and self.ckpt_secs and time.time() - self.t_last_ckpt >= self.ckpt_secs)
        if self.world > 1:
            save_due = self._decide(train_op, save_due)
        elif self.sig.signal_received:                                   # StopAtSignalHook.after_run
            self.stop = True
        if self.sum_steps and step % self.sum_steps == 0:
            now = time.time()
            rate = (step - self.step_last_sum) / max(now - self.t_last_sum, 1e-9)
            rec = {'global_step': step, **rep.summary_scalars(out),       # the reference's summary tags
                   'global_step/sec': rate, 'images/sec': rate * rep.B * self.world}
            self.log.info('global_step/sec: %.4g  %s', rate, json.dumps(rec))
            if self.summaries:
                self.summaries.write(json.dumps(rec) + '\n')
                self.summaries.flush()
                self.events.add_scalars(step, {k: v for k, v in rec.items() if k != 'global_step'})
                for tag, t, max_outputs in rep.summary_images():
                    self.events.add_images(step, tag, t[:max_outputs].cpu().numpy(), max_outputs)
                self.events.flush()
            self.t_last_sum, self.step_last_sum = now, step
        if save_due:
            self.save()
        return out

    def _write_trace(self, step):
        """Per-launch timings of the implicit-GEMM kernels of one step (hipEvent pairs recorded by the library),
        the stand-in for the reference's RunMetadata FULL_TRACE; whole-process traces come from rocprofv3."""
        lib = _lib.load()
        lib.a3d_timing_enable(0)
        cap = 4096
        arr = (_lib.TimingRecord * cap)()
        n = lib.a3d_timing_collect(arr, cap)
        recs = [{'mode': ('fwd', 'bwd_data', 'bwd_filter')[r.mode], 'tile': f'{r.bm}x{r.bn}', 'waves': r.nwaves,
                 'precision': ('fp32', 'bf16x3', 'bf16')[r.prec], 'kernel': ('igemm', 'igemm_glds', 'conv3_fwd', 'igemm_ring', 'fewch_bwdf', 'retired')[r.lds_dma], 'splitk': r.splitk, 'm': r.m, 'n': r.n, 'k': r.k,
                 'ms': round(r.ms, 4), 'tflops': round(r.flops / max(r.ms, 1e-6) / 1e9, 1)} for r in arr[:n]]
        with open(os.path.join(self.dir, f'trace-{step}.json'), 'w') as f:
            json.dump({'global_step': step, 'launches': recs}, f)

    def save(self):
        """Every replica calls this together (a sharded optimizer state is gathered first); the chief writes."""
        rep = self.op.replica
        rep.gather_state()
        if not self.dir:
            return
        torch.cuda.synchronize()
        prefix = f'model.ckpt-{rep.global_step}'
        path = os.path.join(self.dir, prefix + '.pt')
        tmp = path + '.tmp'
        torch.save({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in rep.state_dict().items()}, tmp)
        os.replace(tmp, path)
        if self.tf_checkpoints:                               # the same state as a TensorFlow V2 checkpoint
            tfckpt.write_bundle(os.path.join(self.dir, prefix), rep.tf_variables())
        # CheckpointState as tf.train.Saver writes it: with --tf-checkpoints the entries are bundle prefixes, so
        # tf.train.latest_checkpoint finds them (latest_checkpoint() below prefers '<prefix>.pt' when it exists)
        kept = [n for n in self._kept_checkpoints() if n != prefix] + [prefix]
        for old in kept[:-self.keep_checkpoints] if self.keep_checkpoints else []:
            for f in os.listdir(self.dir):
                if f == old + '.pt' or f == old + '.index' or f.startswith(old + '.data-'):
                    os.remove(os.path.join(self.dir, f))
        kept = kept[-self.keep_checkpoints:] if self.keep_checkpoints else kept
        entry = (lambda n: n) if self.tf_checkpoints else (lambda n: n + '.pt')
        tmp = os.path.join(self.dir, 'checkpoint.tmp')
        with open(tmp, 'w') as f:
            f.write(f'model_checkpoint_path: "{entry(prefix)}"\n')
            for n in kept:
                f.write(f'all_model_checkpoint_paths: "{entry(n)}"\n')
        os.replace(tmp, os.path.join(self.dir, 'checkpoint'))
        self.t_last_ckpt = time.time()
        self.log.info(f'Saved checkpoint {path}')

    def _kept_checkpoints(self):
        """Checkpoint prefixes of this directory, oldest first (by global step)."""
        steps = set()
        for f in os.listdir(self.dir):
            if f.startswith('model.ckpt-') and (f.endswith('.pt') or f.endswith('.index')):
                try:
                    steps.add(int(f[len('model.ckpt-'):].rsplit('.', 1)[0]))
                except ValueError:
                    pass
        return [f'model.ckpt-{s_}' for s_ in sorted(steps)]

    def __exit__(self, exc_type, exc, tb):
        self.op.pipeline.close()
        if exc_type is None:
            self.save()                                                  # session close saves a final checkpoint
        if self.summaries:
            self.summaries.close()
        if self.events:
            self.events.close()
        return False


def latest_checkpoint(ckptdir):
    index = os.path.join(ckptdir, 'checkpoint')
    if not os.path.exists(index):
        return None
    with open(index) as f:
        line = f.readline()
    name = line.split('"')[1] if '"' in line else ''
    path = name if os.path.isabs(name) else os.path.join(ckptdir, name)
    if name and not name.endswith('.pt') and os.path.exists(path + '.pt'):
        return path + '.pt'                                           # our own full state beside a bundle of the same step
    if name and (os.path.exists(path) or tfckpt.is_bundle(path)):    # ours (.pt file) or TensorFlow's (bundle prefix)
        return path
    return None


def read_checkpoint(path, map_location):
    """The state a checkpoint holds -> (state, bundle): a TF bundle prefix (written by TensorFlow or --tf-checkpoints) is
    read into name -> ndarray on the host, anything else is a .pt file of name -> tensor, loaded to map_location."""
    if tfckpt.is_bundle(path):
        return tfckpt.read_bundle(path), True
    return torch.load(path, map_location=map_location), False


def load_checkpoint(replica, state, bundle):
    """Put what read_checkpoint returned into a replica."""
    if bundle:
        replica.load_tf_variables(state)
    else:
        replica.load_state_dict(state)


def add_segmentation_args(parser, listed=True):
    """--segmentation, --slic-iters, --slic-compactness: the same three flags on the training, evaluation and prediction
    drivers (evaluate.add_shared_args).  listed=False keeps them out of --help: the two inference drivers' help texts are
    recorded word for word (tests/golden/*_help.txt), so there the flags are described in the module docstrings and in
    INTEGRATION.md instead; they parse and default the same either way."""
    def text(t):
        return t if listed else argparse.SUPPRESS
    parser.add_argument('--segmentation', default='grid', choices=list(models.DCNF_SEGMENTATIONS),
                        help=text('NON-REFERENCE unless grid: what a superpixel is (dcnf only). grid: the square blocks of '
                             '--superpixel. slic: SLIC superpixels of the resized image, each pixel joining one of the 3 x 3 '
                             'clusters around its block, so the pair graph and the CRF stay the grid\'s (Liu et al. 2015 define '
                             'DCNF over such an over-segmentation); targets, colour statistics and the pooled features are taken '
                             'over the labels, and the two similarities are the paper\'s (mean colours, frequency histograms). '
                             'Needs --unary fcsp; not with --pairwise-texture or --min-depth / --max-depth yet. No weight '
                             'depends on it: a checkpoint trained on one segmentation evaluates on the other.'))
    parser.add_argument('--slic-iters', default=models.DCNF_SLIC_ITERS, type=int,
                        help=text('--segmentation slic: assignment / update rounds after the grid start (0: the grid).'))
    parser.add_argument('--slic-compactness', default=models.DCNF_SLIC_COMPACTNESS, type=float,
                        help=text('--segmentation slic: the colour distance, in units of the [0, 1] RGB range, that one '
                                  'superpixel edge of distance weighs as much as; larger keeps the superpixels squarer.'))


def parse_args(argv=None):
    """The reference's flags verbatim (src/ann3depth.py:221-254), plus --beta2 / --augment / --min-depth / --max-depth / --loss-gradient /
    --train-pairwise / --pairwise-texture / --unary / --seed / --trace-every / --profiler."""
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', default='nyu', type=str, help='The dataset to use.')
    parser.add_argument('--model', '-m', default='', type=str, help='Enter a model name.')
    parser.add_argument('--steps', '-s', default=1000000, type=int, help='Total steps')
    parser.add_argument('--batchsize', '-b', default=32, type=int, help='Batchsize')
    parser.add_argument('--ckptdir', '-p', default='checkpoints', help='Checkpoint directory')
    parser.add_argument('--id', default='', type=str, help='Checkpoint path suffix.')
    parser.add_argument('--ckptfreq', '-f', default=900, type=int, help='Create a checkpoint every N seconds.')
    parser.add_argument('--sumfreq', '-r', default=100, type=int, help='Create a summary every N steps.')
    parser.add_argument('--datadir', '-d', default='data', type=str,
                        help='The data directory containing the datasets.')
    parser.add_argument('--timeout', '-k', default=4200, type=int, help='The time after which the process dies.')
    parser.add_argument('--cluster-spec', default='', type=str,
                        help='(ignored) The path to the cluster specification json.')
    parser.add_argument('--job-name', default='local', type=str, help='"worker" or "local"; "ps" exits at once.')
    parser.add_argument('--task-index', default=0, type=int, help='(ignored) rank comes from the launcher.')
    parser.add_argument('--beta2', default=None, type=float,
                        help='NON-REFERENCE: Adam beta2 (the reference hard-codes 1, which freezes the weights).')
    parser.add_argument('--precision', default='fp32', choices=['fp32', 'bf16x3', 'bf16', 'bf16s'],
                        help='NON-REFERENCE unless fp32: arithmetic of the conv contractions.')
    parser.add_argument('--augment', default='none', choices=['none', 'eigen'],
                        help='NON-REFERENCE: train-time augmentation of the input batch on the GPU (msdn only). eigen: scale, '
                             'rotation, translation, flip and colour of Eigen et al. 2014, section 3.4.')
    parser.add_argument('--min-depth', default=None, type=float,
                        help='NON-REFERENCE: the depth maps have holes (msdn, dcnf). A target pixel counts iff its stored depth t '
                             '(the float after the loader\'s +0.5: k/255 for converter-written records) is finite and '
                             'min < t <= max; the others leave the resized target and, for msdn, both losses; dcnf takes a '
                             'superpixel as a target only if at least half of it counts, and trains on the likelihood of those '
                             'superpixels alone. msdn: giving either flag turns the mode on, the other defaults to 0 / +inf; dcnf '
                             'wants both. Still msdn only: --augment and --loss-gradient.')
    parser.add_argument('--max-depth', default=None, type=float, help='NON-REFERENCE: see --min-depth.')
    parser.add_argument('--loss-gradient', default=None, type=float, metavar='W',
                        help='NON-REFERENCE: add W times the gradient-matching term of Eigen & Fergus 2015 (eq. 4) to both '
                             'losses (msdn only): the squared horizontal and vertical differences of the log-depth error over '
                             'the 55 x 74 grid, over the pairs of valid pixels under --min-depth / --max-depth. W >= 0; 0 is '
                             'the run without the flag.')
    parser.add_argument('--loss', default='silog', choices=['silog', 'berhu', 'ssi'],
                        help='NON-REFERENCE unless silog: the objective of both losses (msdn only). silog: the reference\'s '
                             'scale-invariant log loss, under which an output at or below zero gets no gradient. berhu: the reverse '
                             'Huber loss of Laina et al. 2016 on linear depth, L1 up to a threshold and quadratic beyond it, over '
                             'the valid pixels under --min-depth / --max-depth. ssi: the least-squares scale-and-shift-invariant loss of '
                             'Ranftl et al. 2020 on linear depth, the squared error left after the best scale and shift of each '
                             'output, the objective that matches evaluate --align affine. Neither with --loss-gradient.')
    parser.add_argument('--berhu-fraction', default=None, type=float, metavar='F',
                        help='NON-REFERENCE, --loss berhu: the threshold is F times the largest error of each sample (per sample, '
                             'not per batch, so that a sample\'s gradient does not depend on its batch). 0 < F <= 1, default 0.2.')
    parser.add_argument('--optimizer', default='adam', choices=['adam', 'momentum'],
                        help='NON-REFERENCE unless adam: the update rule (msdn only). adam: the reference\'s AdamOptimizer(rate, 0.9, '
                             'beta2), which at its beta2 = 1 never moves a weight. momentum: SGD with momentum without Nesterov '
                             '(TensorFlow\'s MomentumOptimizer), the rule the per-group rates 0.001 / 0.1 / 0.001 / 0.01 were published '
                             'for (Eigen et al. 2014); one slot per variable instead of two, and the dense layers\' filter gradient '
                             'goes straight into the update. Not with --beta2. A checkpoint restores only under the optimizer '
                             'that wrote it; evaluate and predict read that from the checkpoint.')
    parser.add_argument('--momentum', default=None, type=float, metavar='M',
                        help='NON-REFERENCE, --optimizer momentum: its momentum. 0 <= M < 1, default 0.9.')
    parser.add_argument('--lr-scale', default=None, type=float, metavar='S',
                        help='NON-REFERENCE: multiply every per-group rate by S (msdn only, either optimizer). S > 0, default 1.')
    parser.add_argument('--clip-norm', default=None, type=float, metavar='C',
                        help='NON-REFERENCE: bound the gradient of every optimizer group (msdn: CoarseConv, CoarseDense, FineA, '
                             'FineB; dcnf: unary, pairwise) by its own global norm C, as tf.clip_by_global_norm over one '
                             'optimizer\'s gradients, and skip a group\'s step when its gradient is not finite. C > 0; inf measures '
                             'and skips without clipping. The norms, scales and skipped steps go to the summaries. msdn: the dense '
                             'layers\' filter gradient is written out for its norm instead of going straight into the update. '
                             'Not stored in checkpoints: a run resumes under the flag it is given.')
    parser.add_argument('--train-pairwise', action='store_true',
                        help='NON-REFERENCE: learn the pairwise dense layer of the CRF (dcnf only). The reference leaves it at '
                             'its initial draw (TF 1.3 has no gradient for scatter_nd_update); with this flag the loss is also '
                             'differentiated through the CRF matrix and the layer descends at 0.1, kept >= 0 (Liu et al. 2015).')
    parser.add_argument('--pairwise-texture', action='store_true',
                        help='NON-REFERENCE: a third pairwise similarity for the CRF (dcnf only), texture disparity over '
                             'local-binary-pattern histograms of the superpixels (Liu et al. 2015); the pairwise kernel is '
                             '[3,1], and a checkpoint with a [2,1] kernel is refused. Meant to go with --train-pairwise: '
                             'without it the layer keeps its initial draw, as the reference\'s does.')
    parser.add_argument('--unary', default='patch', choices=['patch', 'fcsp'],
                        help='NON-REFERENCE unless patch: the form of the unary part (dcnf only). patch: the reference\'s, the '
                             'conv stack over 48 overlapping 100 x 100 patches per image. fcsp: the convs once over the whole '
                             'image, the last feature map averaged inside every superpixel, then the dense head (Liu et al. '
                             '2015, DCNF-FCSP); dense/kernel is [256,128], and a checkpoint of the other form is refused.')
    parser.add_argument('--superpixel', default=40, type=int, choices=[40, 20, 10],
                        help='NON-REFERENCE unless 40: the edge of the superpixels (dcnf only). 40: the reference\'s 6 x 8 depth '
                             'map per image. 20 and 10: 12 x 16 and 24 x 32, on the banded CRF likelihood (no epsilons; its '
                             'value is not comparable with the loss at 40). They need --unary fcsp and do not go with '
                             '--min-depth / --max-depth yet. No weight depends on the grid: a checkpoint trained at one '
                             'evaluates at another.')
    add_segmentation_args(parser)
    parser.add_argument('--seed', default=0, type=int, help='Shuffle-queue seed.')
    parser.add_argument('--tf-checkpoints', action='store_true',
                        help='Also write every checkpoint as a TensorFlow V2 bundle (model.ckpt-N.index/.data-*).')
    parser.add_argument('--trace-every', default=5000, type=int,
                        help='TraceHook period (src/ann3depth.py:105): the first step and every N-th global step.')
    parser.add_argument('--profiler', default='launches', choices=['launches', 'rocprofv3'],
                        help='What a traced step records: per-launch timings of the GEMM kernels (trace-N.json), or '
                             'also a rocprofv3 kernel + marker trace (the process is started under the profiler).')
    return parser.parse_args(argv)


if __name__ == '__main__':
    sys.exit(main())
