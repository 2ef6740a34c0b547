"""Generates tests/golden/loss_bits.json: the bits the four loss objectives (silog plain and masked, silog with the
gradient-matching term, berHu) gave at ONE commit, so that a change to their kernels that promises "same bits" is held to it
(tests/test_gpu_loss_bits.py replays every case).  Needs a GPU and a built checkout of the commit to record:

    python tests/golden/make_loss_bits.py [--commit HASH] [--out FILE]

Only the public ops.*_loss_fwd / _bwd are used.  The fixture is DATA: per case the loss words, the per-sample workspace words
ws[1 : 1 + K b] (a SHA-256 of them where there are more than WS_WORDS) and the ticket ws[0] as uint32, and SHA-256 digests
of dout and of the bf16 copy with its pitch columns.
Inputs come from rng.integers alone, scaled by exact powers of two or small divisors, so nothing rests on a floating-point
generator: finite outputs of which about half are <= 0 (their logarithms NaN, masked to 0), targets with exact zeros, and in
the masked cases about 30 % NaN targets and, from three samples on, one sample without a finite target.  Non-finite outputs
and infinities are pinned by the tests of each loss and stay out of this file."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, 'loss_bits.json')

# (b, npix): one pixel; fewer pixels than parts; a chunk of 257, one past a thread count; the last block's second round over
# the samples; a chunk of 1025, a second round of 4 x 256; the model's grid
SHAPES = [(1, 1), (3, 7), (2, 2049), (65, 37), (1, 8200), (5, 4070)]
BERHU_SHAPES = SHAPES + [(2, 4071)]                 # rows that start off the 16-byte grid
# (b, h, w): (1, 6, 1500) has a halo longer than a chunk and a second round
GRAD_SHAPES = [(1, 1, 1), (3, 1, 7), (2, 7, 1), (65, 2, 5), (1, 6, 1500), (5, 55, 74)]
PITCH_EXTRA = 3                                     # columns of the bf16 copy past npix, prefilled and left alone
FILL = 7.0
WS_WORDS = 64                                       # workspace words recorded one by one; more are recorded as a digest


def cases():
    """Every case as a dict of plain values; 'id' names it in the fixture and in the test."""
    out = []
    for masked in (0, 1):
        for b, npix in SHAPES:
            out.append(dict(id=f'silog-{"masked" if masked else "plain"}-{b}x{npix}', family='silog', masked=masked, b=b,
                            npix=npix))
    for masked in (0, 1):
        for b, npix in BERHU_SHAPES:
            out.append(dict(id=f'berhu-m{masked}-{b}x{npix}', family='berhu', masked=masked, fraction=0.2, b=b, npix=npix))
    for masked in (0, 1):
        for weight in (0.0, 0.5):
            for b, h, w in GRAD_SHAPES:
                out.append(dict(id=f'gradloss-m{masked}-w{weight}-{b}x{h}x{w}', family='gradloss', masked=masked, weight=weight,
                                b=b, h=h, w=w, npix=h * w))
    return out


def inputs(case):
    """(out, tgt) float32 [b, npix].  out: k / 1024, k in [-1024, 1024); tgt: k / 255, k in [0, 256), every 97th exactly 0."""
    b, npix = case['b'], case['npix']
    seed = int.from_bytes(hashlib.sha256(case['id'].encode()).digest()[:4], 'little')
    rng = np.random.default_rng(seed)
    o = (rng.integers(-1024, 1024, (b, npix)) / 1024).astype(np.float32)
    t = (rng.integers(0, 256, (b, npix)) / 255).astype(np.float32)
    t.reshape(-1)[::97] = 0
    if case['masked']:
        t[rng.integers(0, 10, (b, npix)) < 3] = np.nan
        if b >= 3:
            t[b // 2] = np.nan
    return o, t


def words(t, limit=None):
    """float32 tensor -> its words as one hex string, 8 digits each; of more than `limit` words, 'sha256:' and the digest of
    their bytes instead (the 65-sample cases' workspace words, which would otherwise make up most of the file)."""
    if limit is not None and t.numel() > limit:
        return 'sha256:' + digest(t)
    return ''.join(f'{v:08x}' for v in t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32))


def digest(t):
    """SHA-256 of a tensor's bytes (float32 or bfloat16)."""
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def measure(ops, case):
    """Runs the case's forward and backward on the GPU; what the fixture records of it."""
    import torch
    o, t = inputs(case)
    od, td = torch.from_numpy(o).cuda(), torch.from_numpy(t).cuda()
    b, npix, masked = case['b'], case['npix'], case['masked']
    dout = torch.full((b, npix), FILL, device='cuda')
    d16 = torch.full((b, npix + PITCH_EXTRA), FILL, device='cuda', dtype=torch.bfloat16)
    if case['family'] == 'silog':
        k, width = (3, 2) if masked else (2, 1)
        ws = (ops.silog_masked_ws if masked else ops.silog_ws)(b, 'cuda')
        loss = torch.full((width,), FILL, device='cuda')
        (ops.silog_masked_loss_fwd if masked else ops.silog_loss_fwd)(od, td, loss, ws)
        (ops.silog_masked_loss_bwd if masked else ops.silog_loss_bwd)(od, td, ws, dout, d16)
    elif case['family'] == 'berhu':
        k, width = 3, 4
        ws = ops.berhu_ws(b, 'cuda')
        loss = torch.full((width,), FILL, device='cuda')
        ops.berhu_loss_fwd(od, td, masked, case['fraction'], loss, ws)
        ops.berhu_loss_bwd(od, td, masked, case['fraction'], ws, dout, d16)
    else:
        k, width = 5, 4
        ws = ops.silog_grad_ws(b, 'cuda')
        loss = torch.full((width,), FILL, device='cuda')
        ops.silog_grad_loss_fwd(od, td, case['h'], case['w'], masked, case['weight'], loss, ws)
        ops.silog_grad_loss_bwd(od, td, case['h'], case['w'], masked, case['weight'], ws, dout, d16)
    torch.cuda.synchronize()
    return dict(loss=words(loss), ws=words(ws[1:1 + k * b], WS_WORDS), ticket=words(ws[:1]), dout_sha256=digest(dout),
                dout16_sha256=digest(d16))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--commit', help='hash of the commit that is recorded (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], check=True, capture_output=True,
                                           text=True).stdout.strip()
    sys.path.insert(0, ROOT)
    from ann3depth_amd import ops
    recorded = [dict(case, **measure(ops, case)) for case in cases()]
    with open(args.out, 'w') as f:
        json.dump({'commit': commit, 'cases': recorded}, f, indent=0)
        f.write('\n')
    print(f'{args.out}: {len(recorded)} cases of commit {commit}, {os.path.getsize(args.out) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
