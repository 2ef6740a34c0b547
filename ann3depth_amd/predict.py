"""Prediction driver: restore an MSDN or DCNF checkpoint and write a depth map for every image file given.

    python -m ann3depth_amd.predict --model msdn|dcnf [--id r1 | --checkpoint PATH] [--superpixel 40|20|10]
        [--precision ...] [--batchsize B] [--upsample joint|bilinear|none] [--radius R --sigma-space S --sigma-range S]
        [--uncertainty] [--depths DIR --min-depth LO --max-depth HI] [--align MODE --align-to DIR] --out DIR IMAGE.png ...

Each image is read with png.imread (8-bit RGB; grey is replicated to three channels, alpha is dropped), consecutive
images of one size run together in batches of up to B through the replica's predict() on their uint8 pixels, and the
`fine` (msdn) or `crf` (dcnf) output is brought to the image's own size:
  joint     (default, NON-REFERENCE) joint bilateral upsampling under the image itself (ops.joint_bilateral_upsample,
            include/a3d_upsample.h): depth edges follow the image's edges;
  bilinear  ops.resize_bilinear_tf1, the legacy resize every other part of the project samples predictions with;
  none      the model's own grid (55 x 74; 6 x 8, 12 x 16 or 24 x 32).
Written per image: DIR/<stem>-depth.npy (float32, the values) and DIR/<stem>-depth.png (8 bits, min-max scaled per image
over its finite pixels with the rounding tools/data_preprocessor.py uses for depth PNGs, imresize.bytescale; a pixel that
is not finite becomes 0).  One JSON line on stdout names the files, their sizes and the count of non-finite pixels, and
for dcnf `singular_systems`.  Exit code 2, before a GPU is touched, when there is nothing to do (no checkpoint, no image,
an unreadable image) or the request is unsupported (an unknown model, more than one process, a --superpixel the
checkpoint's form cannot run).

dcnf is a probabilistic model, y ~ N(mu, A^-1 / 2) over the superpixels (NON-REFERENCE, include/a3d_posterior.h,
DCNFReplica.posterior); msdn has no distribution, so both flags are refused for it:
  --uncertainty   also writes <out>/<stem>-sigma.npy and .png: the field's standard deviation per superpixel, sqrt(var),
                  brought to the output size exactly as the depth map is (under --upsample joint by the same upsampler).
                  The depth files are the bytes they are without the flag.
  --depths DIR    depth completion: DIR/<stem>.npy, float32 [H, W] of any size, is a measured depth map with holes, a
                  pixel a hole where it is not finite or outside (--min-depth, --max-depth].  The field is conditioned on
                  the superpixels the file measures (at least half of their pixels, the replica's min_valid): they come
                  back as their block means, the others as the conditional mean, and sigma is 0 and the conditional
                  standard deviation.  A missing file, or one of another rank or dtype, exits 2 before any GPU work.
With either flag the JSON line gains `uncertainty`, `conditioned`, `observed_fraction` (the share of superpixels a file
measured; 0 without --depths) and `rejected_systems` (images whose system was not positive definite: NaN maps).

--segmentation slic [--slic-iters N --slic-compactness M] (NON-REFERENCE, dcnf, a checkpoint of --unary fcsp;
include/a3d_slic.h; the training driver's three flags, not listed by --help): the field runs over SLIC superpixels of the
resized image instead of square blocks.  The crf output is painted onto 240 x 320 by the labels, then --upsample bilinear
resizes that map to the image's size and --upsample none writes it as it is; the JSON line gains `segmentation`,
`slic_iters`, `slic_compactness`.  Refused with it, before any GPU work: --upsample joint (the default: name bilinear or
none), --uncertainty, --depths.

--align median|scale|affine --align-to DIR (NON-REFERENCE, both models, every --upsample; include/a3d_align.h; both flags
or neither): the models predict in the training data's normalised units, depth up to an affine map per image.  DIR/<stem>.npy,
float32 [H, W] of any size, holds a few measured depths (a sparse LiDAR or Kinect map; a pixel is measured where it is finite
and inside (--min-depth, --max-depth]).  Each map at its output size is sampled at the measured map's pixels, the scale and
shift of ops.depth_align are fitted over the measured ones, and the map is written as s * map + b (ops.affine_apply); a
-sigma map is scaled by |s| alone.  Each entry of `files` gains `scale`, `shift`, `measured` (the pixels fitted on) and
`aligned` (false: the fit was refused, e.g. nothing measured, and the map is written as it is); the JSON line gains `align`,
`min_depth`, `max_depth`.  Exit code 2 before any GPU work: one flag without the other, --align-to with --depths (the
conditioned field already uses the measurements), a missing or unusable file, --min-depth >= --max-depth."""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import imresize, ops, png
from .evaluate import (OUTPUTS, add_shared_args, add_upsample_args, open_checkpoint, refuse_model, refuse_under_slic,
                       restore_replica)


def _say(msg):
    print(f'predict: {msg}', file=sys.stderr, flush=True)


def read_image(path):
    """Image file -> uint8 [H, W, 3]: RGB as it is, grey replicated, alpha dropped.  ValueError for anything else."""
    a = np.asarray(png.imread(path))
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0:
        raise ValueError(f'{path}: not an 8-bit image ({a.dtype}, shape {a.shape})')
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[2] in (2, 4):                          # grey + alpha, RGBA
        a = a[..., :-1]
    if a.shape[2] == 1:
        a = np.repeat(a, 3, axis=2)
    if a.shape[2] != 3:
        raise ValueError(f'{path}: {a.shape[2]} channels')
    return np.ascontiguousarray(a)


def depth_png(depth):
    """float32 [H, W] -> uint8 [H, W]: imresize.bytescale over the finite pixels (min -> 0, max -> 255, `+ 0.5` and
    truncated, as the preprocessor's depth PNGs are made); a pixel that is not finite becomes 0."""
    depth = np.asarray(depth, np.float32)
    ok = np.isfinite(depth)
    if not ok.any():
        return np.zeros(depth.shape, np.uint8)
    lo, hi = depth[ok].min(), depth[ok].max()
    img = imresize.bytescale(np.where(ok, depth, lo), cmin=lo, cmax=hi)
    img[~ok] = 0
    return img


def batches(images, B, also=None):
    """Runs of consecutive images of one size, at most B long: lists of indices.  also: a second list of arrays (the
    measured depth maps) whose sizes must agree within a run too."""
    def key(i):
        return (images[i].shape, None if also is None else also[i].shape)
    out = []
    for i in range(len(images)):
        if out and len(out[-1]) < B and key(out[-1][0]) == key(i):
            out[-1].append(i)
        else:
            out.append([i])
    return out


def read_depth(path):
    """A measured depth map: float32 [H, W], holes as they are.  ValueError for anything else."""
    a = np.load(path, allow_pickle=False)
    if a.dtype != np.float32 or a.ndim != 2 or a.size == 0:
        raise ValueError(f'not a float32 [H, W] array ({a.dtype}, shape {a.shape})')
    return np.ascontiguousarray(a)


def main(argv=None):
    args = parse_args(argv)
    if refuse_model(args, _say, 'can predict'):
        return 2
    if args.batchsize <= 0:
        _say(f'--batchsize {args.batchsize} must be positive.')
        return 2
    if refuse_under_slic(args, _say, (('--upsample joint', args.upsample == 'joint'), ('--uncertainty', args.uncertainty),
                                      ('--depths', bool(args.depths)))):
        return 2
    posterior = args.uncertainty or bool(args.depths)
    if posterior and args.model != 'dcnf':
        _say(f'--uncertainty and --depths read the distribution of the CRF of --model dcnf, y ~ N(mu, A^-1 / 2): '
             f'{args.model} is a regression without one.')
        return 2
    if args.depths and not (args.min_depth < args.max_depth):
        _say(f'--depths needs --min-depth < --max-depth (a pixel is measured inside ({args.min_depth}, {args.max_depth}]).')
        return 2
    if (args.align != 'none') != bool(args.align_to):
        _say('--align MODE and --align-to DIR go together: the mode of the fit, and the measured depth maps it is fitted to.')
        return 2
    if args.align_to and args.depths:
        _say('--align-to cannot go with --depths: the conditioned field already uses the measurements.')
        return 2
    if args.align_to and not (args.min_depth < args.max_depth):
        _say(f'--align-to needs --min-depth < --max-depth (a pixel is measured inside ({args.min_depth}, {args.max_depth}]).')
        return 2

    def no_images():
        if not args.images:
            _say('no images given.')
            return 2

    opened = open_checkpoint(args, _say, 'prediction', 'predict with untrained weights', no_images)
    if opened == 2:
        return 2
    upsample, _, ckpt = opened
    images = []
    for path in args.images:
        try:
            images.append(read_image(path))
        except Exception as e:                        # whatever a decoder makes of a file that is no image
            _say(f'cannot read {path}: {e}')
            return 2
    stems = [os.path.splitext(os.path.basename(p))[0] for p in args.images]
    if len(set(stems)) != len(stems):
        _say(f'two images share a file stem and would be written to one place: {sorted(s for s in set(stems) if stems.count(s) > 1)}')
        return 2
    measured = None
    if args.depths:
        measured = []
        for stem in stems:
            path = os.path.join(args.depths, stem + '.npy')
            try:
                measured.append(read_depth(path))
            except Exception as e:                    # a missing file, a pickle, a text file, another rank or dtype
                _say(f'--depths: cannot use {path}: {e}')
                return 2
    fit_to = None
    if args.align_to:
        fit_to = []
        for stem in stems:
            path = os.path.join(args.align_to, stem + '.npy')
            try:
                fit_to.append(read_depth(path))
            except Exception as e:
                _say(f'--align-to: cannot use {path}: {e}')
                return 2
    restored = restore_replica(args, ckpt, _say)
    if restored is None:
        return 2
    replica = restored[0]
    dev = replica.device
    os.makedirs(args.out, exist_ok=True)
    files, singular, rejected, observed = [], 0, 0, 0

    def to_size(grid, pixels, n):
        """[B, gh, gw] on the model's grid -> the n maps at the output size, as --upsample says."""
        H, W = pixels.shape[1:3]
        if upsample is not None:
            return upsample(grid[:n], pixels)
        if args.upsample == 'bilinear':
            return ops.resize_bilinear_tf1(grid[:n].reshape(n, grid.shape[1], grid.shape[2], 1),
                                           torch.empty((n, H, W, 1), device=dev)).view(n, H, W)
        return grid[:n]

    for idx in batches(images, args.batchsize, measured if fit_to is None else fit_to):
        n = len(idx)
        pixels = torch.from_numpy(np.stack([images[i] for i in idx])).to(dev)
        pred = replica.predict(pixels, n)[1]                       # fine (msdn) or crf (dcnf), [B, gh, gw]
        if args.model == 'dcnf':
            singular += int(replica.status[:n].sum().item())
            if replica.slic:
                pred = replica.depth_map(pred)                     # painted by the labels: [B, 240, 320]
        H, W = pixels.shape[1:3]
        sigma = None
        if posterior:                                  # from the z and r predict() left
            holes = None
            if measured is not None:
                holes = torch.from_numpy(np.stack([measured[i] for i in idx])[..., None]).to(dev)
            mean, var = replica.posterior(None, holes, n, (args.min_depth, args.max_depth) if holes is not None else None,
                                          want_var=args.uncertainty)
            rejected += int(replica.status[:n].sum().item())
            observed += int(replica.nobs[:n].sum().item())
            if holes is not None:
                pred = mean                                # without --depths the depth map stays predict()'s, byte for byte
            if var is not None:
                sigma = to_size(torch.sqrt(var), pixels, n)
        full = to_size(pred, pixels, n)
        fit = None
        if fit_to is not None:                         # the maps at output size, sampled at the measured maps' pixels
            coef, count, status = ops.depth_align(full, torch.from_numpy(np.stack([fit_to[i] for i in idx])).to(dev),
                                                  args.align, min_depth=args.min_depth, max_depth=args.max_depth)
            full = full.contiguous()
            ops.affine_apply(full, coef, out=full)         # in place
            if sigma is not None:
                by_scale = torch.stack([coef[:, 0].abs(), torch.zeros_like(coef[:, 0])], 1).contiguous()
                sigma = sigma.contiguous()
                ops.affine_apply(sigma, by_scale, out=sigma)
            fit = (coef.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy())
        full = full.cpu().numpy()
        if sigma is not None:
            sigma = sigma.cpu().numpy()
        for k, i in enumerate(idx):
            base = os.path.join(args.out, stems[i] + '-depth')
            np.save(base + '.npy', full[k])
            png.imsave(base + '.png', depth_png(full[k]))
            files.append({'image': args.images[i], 'image_size': [int(H), int(W)], 'npy': base + '.npy', 'png': base + '.png',
                          'size': [int(v) for v in full[k].shape], 'nonfinite': int((~np.isfinite(full[k])).sum())})
            if fit is not None:
                files[-1].update(scale=float(fit[0][k, 0]), shift=float(fit[0][k, 1]), measured=int(fit[1][k]),
                                 aligned=bool(fit[2][k] == 0))
            if sigma is not None:
                base = os.path.join(args.out, stems[i] + '-sigma')
                np.save(base + '.npy', sigma[k])
                png.imsave(base + '.png', depth_png(sigma[k]))
                files[-1].update(sigma_npy=base + '.npy', sigma_png=base + '.png')
    out = {'checkpoint': ckpt, 'global_step': replica.global_step, 'model': args.model, 'precision': args.precision,
           'output': OUTPUTS[args.model][1], 'upsample': args.upsample, 'files': files,
           'nonfinite': int(sum(f['nonfinite'] for f in files))}
    if upsample is not None:
        out.update(radius=upsample.radius, sigma_space=upsample.sigma_space, sigma_range=upsample.sigma_range)
    if args.model == 'dcnf':
        out.update(superpixel=args.superpixel, singular_systems=singular)
        if args.segmentation != 'grid':
            out.update(segmentation=args.segmentation, slic_iters=args.slic_iters, slic_compactness=args.slic_compactness)
    if posterior:
        out.update(uncertainty=bool(args.uncertainty), conditioned=measured is not None,
                   observed_fraction=observed / float(len(images) * replica.nsp), rejected_systems=rejected)
        if measured is not None:
            out.update(min_depth=args.min_depth, max_depth=args.max_depth)
    if fit_to is not None:
        out.update(align=args.align, min_depth=args.min_depth, max_depth=args.max_depth)
    print(json.dumps(out), flush=True)
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Depth maps for image files from an MSDN or DCNF checkpoint.')
    p.add_argument('images', nargs='*', type=str, help='8-bit PNG files (RGB or grey; alpha is dropped).')
    p.add_argument('--out', '-o', required=True, type=str, help='Directory for <stem>-depth.npy and <stem>-depth.png.')
    add_shared_args(p, 'model', 'batchsize', 'ckptdir', 'id', 'checkpoint', 'precision', 'superpixel', 'segmentation',
                    batchsize='Images of one size that run together.',
                    superpixel='NON-REFERENCE unless 40, dcnf: the edge of the superpixels (6 x 8, 12 x 16 or 24 x 32 depths per '
                               'image before upsampling); 20 and 10 need a checkpoint of --unary fcsp.')
    p.add_argument('--uncertainty', action='store_true',
                   help='NON-REFERENCE, dcnf: also write <stem>-sigma.npy / .png, the standard deviation of the CRF\'s field per '
                        'superpixel, brought to the output size as the depth map is.')
    p.add_argument('--depths', default='', type=str,
                   help='NON-REFERENCE, dcnf: depth completion. DIR/<stem>.npy (float32 [H, W], any size) is a measured depth '
                        'map with holes; the field is conditioned on the superpixels it measures.')
    p.add_argument('--min-depth', default=0., type=float, help='--depths: a pixel is measured if its value is > this ...')
    p.add_argument('--max-depth', default=float('inf'), type=float, help='... and <= this, and finite.')
    # NON-REFERENCE: --align MODE --align-to DIR (see the module docstring).  Kept out of --help: this driver's help text is
    # recorded word for word (tests/golden/predict_help.txt).
    p.add_argument('--align', default='none', choices=['none'] + list(ops.ALIGN_MODES), help=argparse.SUPPRESS)
    p.add_argument('--align-to', default='', type=str, metavar='DIR', help=argparse.SUPPRESS)
    add_upsample_args(p, ['joint', 'bilinear', 'none'], 'joint',
                      'How the prediction reaches the image\'s size: joint (NON-REFERENCE: joint bilateral upsampling under '
                      'the image), bilinear (the legacy resize), none (it stays on the model\'s grid).')
    return p.parse_args(argv)


if __name__ == '__main__':
    sys.exit(main())
