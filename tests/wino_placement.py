"""The table behind tests/test_gpu_wino_placement.py and tests/test_wino_placement_cpu.py: every entry point of the Winograd
surfaces (include/a3d_wino.h, a3d_wino_grad.h, a3d_wino_bwd.h, a3d_wino1d.h, the 'fp32w' arithmetic of include/a3d.h) and the fused
momentum launch (include/a3d_optim.h), with its pointer operands in argument order, their element types, its image-side operand
and whether it takes a workspace; the placements each is swept over; what the headers let it refuse; the cases; and the sets of
outputs a non-finite input must reach, may reach and must not reach, from geometry alone.  No GPU and no library is needed here."""
import collections

import numpy as np

import wino1d_ref as W1
import wino_ref as W

Entry = collections.namedtuple('Entry', 'cname operands types image ws family')

U8 = {'argmax': 'u8'}
_BWD = ('x', 'dz', 'w', 'dw', 'db', 'dx')
_BWD_U = ('x', 'dz', 'U', 'dw', 'db', 'dx')
# family: 'w' F(2x2,3x3) (wino.hip), 'l' F(4,5) (wino1d.hip), 'o' the fused momentum launch (optim.hip)
ENTRIES = {
    'fwd': Entry('a3d_conv2d_fwd', ('x', 'w', 'bias', 'y'), {}, 'x', True, 'w'),
    'fwd_prepared': Entry('a3d_conv2d_fwd', ('x', 'U', 'bias', 'y'), {}, 'x', True, 'w'),
    'bwd_data': Entry('a3d_conv2d_bwd_data', ('dz', 'w', 'dx'), {}, 'dx', True, 'w'),
    'bwd_data_mask': Entry('a3d_conv2d_bwd_data', ('dz', 'w', 'dx', 'mask'), {}, 'dx', True, 'w'),
    'bwd_data_prepared': Entry('a3d_conv2d_bwd_data', ('dz', 'U', 'dx'), {}, 'dx', True, 'w'),
    'bwd_data_prepared_mask': Entry('a3d_conv2d_bwd_data', ('dz', 'U', 'dx', 'mask'), {}, 'dx', True, 'w'),
    'wg_bwd_filter': Entry('a3dwg_conv2d_bwd_filter', ('x', 'dz', 'dw'), {}, 'x', True, 'w'),
    'wg_bwd_filter_db': Entry('a3dwg_conv2d_bwd_filter', ('x', 'dz', 'dw', 'db'), {}, 'x', True, 'w'),
    'wb': Entry('a3dwb_conv2d_bwd', _BWD, {}, 'x', True, 'w'),
    'wb_prepared': Entry('a3dwb_conv2d_bwd', _BWD_U, {}, 'x', True, 'w'),
    'wb_mask': Entry('a3dwb_conv2d_bwd', _BWD + ('mask',), {}, 'x', True, 'w'),
    'wb_prepared_mask': Entry('a3dwb_conv2d_bwd', _BWD_U + ('mask',), {}, 'x', True, 'w'),
    'wb_pool': Entry('a3dwb_conv2d_bwd', _BWD + ('argmax', 'pool_y'), U8, 'x', True, 'w'),
    'wb_prepared_pool': Entry('a3dwb_conv2d_bwd', _BWD_U + ('argmax', 'pool_y'), U8, 'x', True, 'w'),
    'l_bwd_data': Entry('a3dl_conv2d_bwd_data', ('dz', 'w', 'dx'), {}, 'dx', True, 'l'),
    'l_bwd_data_mask': Entry('a3dl_conv2d_bwd_data', ('dz', 'w', 'dx', 'mask'), {}, 'dx', True, 'l'),
    'l_bwd_data_prepared': Entry('a3dl_conv2d_bwd_data', ('dz', 'U', 'dx'), {}, 'dx', True, 'l'),
    'l_bwd_data_prepared_mask': Entry('a3dl_conv2d_bwd_data', ('dz', 'U', 'dx', 'mask'), {}, 'dx', True, 'l'),
    'l_bwd_filter': Entry('a3dl_conv2d_bwd_filter', ('x', 'dz', 'dw', 'db'), {}, 'x', True, 'l'),
    'prepare_fwd': Entry('a3d_conv2d_fwd_prepare_filter', ('w', 'prepared'), {}, 'w', False, 'w'),
    'prepare_bwd_data': Entry('a3dw_conv2d_bwd_data_prepare_filter', ('w', 'prepared'), {}, 'w', False, 'w'),
    'l_prepare_bwd_data': Entry('a3dl_conv2d_bwd_data_prepare_filter', ('w', 'prepared'), {}, 'w', False, 'l'),
    'momentum': Entry('a3do_dense_bwd_filter_momentum', ('x', 'dz', 'var_w', 'accum_w', 'var_b', 'accum_b'), {}, 'x', False, 'o'),
}

# The eight host decisions between a 16-byte and a scalar transform kernel (csrc/wino.hip wino_input, wino_output, wino_dz,
# wino_bwd_transforms, wino_bwd_finish; csrc/wino1d.hip wino1d_input, wino1d_dz, wino1d_output) -> the operands whose address each
# reads, by the name they carry in the entries above.
DECISIONS = {
    'wino_input': ('x', 'dz'), 'wino_output': ('y', 'dx', 'mask'), 'wino_dz': ('dz',), 'wino_bwd_transforms': ('x', 'dz'),
    'wino_bwd_finish': ('dx', 'mask', 'pool_y', 'argmax'), 'wino1d_input': ('x', 'dz'), 'wino1d_dz': ('dz',),
    'wino1d_output': ('dx', 'mask'),
}

ELEMENT_BYTES = {'f32': 4, 'u8': 1}
ALONE, IMAGE, TOGETHER, WS_OFFSETS = 4, 8, {'f32': 12, 'u8': 1}, (16, 4)


def operand_type(entry, o):
    return ENTRIES[entry].types.get(o, 'f32')


def sweep(entry):
    """[(label, {operand: byte offset past a 256-byte boundary}, workspace byte offset)]; the first is the on-grid launch the
    others are compared with.  Each operand alone at +4 bytes, a byte operand alone at +1 too, the image-side operand alone at +8,
    all operands together (float32 +12, bytes +1), then the workspace at +16 and at +4 under on-grid operands."""
    e = ENTRIES[entry]
    out = [('on-grid', {}, 0)]
    for o in e.operands:
        if operand_type(entry, o) == 'u8':
            out.append((f'{o}+1', {o: 1}, 0))
        out.append((f'{o}+{ALONE}', {o: ALONE}, 0))
    out.append((f'{e.image}+{IMAGE}', {e.image: IMAGE}, 0))
    out.append(('all', {o: TOGETHER[operand_type(entry, o)] for o in e.operands}, 0))
    if e.ws:
        out += [(f'ws+{b}', {}, b) for b in WS_OFFSETS]
    return out


# What the headers say an entry point refuses, (C entry point, operand) -> the alignment in bytes asked of it.  Written from the
# headers, not from the code:
#   include/a3d.h "`ws`, where it is not NULL, must be 16-byte aligned"; a3d_wino_grad.h, a3d_wino_bwd.h, a3d_wino1d.h "ws: 16-byte
#   aligned";
#   a3d.h / a3d_wino.h / a3d_wino1d.h "into a caller-owned, 16-byte aligned buffer" (the prepared form, written and read);
#   a3d.h "a float32 tensor, a bias or an argmax row start at any multiple of its element size"; a3d_optim.h "the tensors need
#   4-byte alignment only": nothing else may be refused.
REFUSED = {
    **{(e.cname, 'ws'): 16 for e in ENTRIES.values() if e.ws},
    **{(e.cname, 'U'): 16 for e in ENTRIES.values() if 'U' in e.operands},
    **{(e.cname, 'prepared'): 16 for e in ENTRIES.values() if 'prepared' in e.operands},
}
# the words by which a3d_last_error names an operand that carries another name in the C argument list
NAMED_AS = {'ws': r'\bws\b', 'U': r'\bprepared filter\b', 'prepared': r'\bbuffer\b'}


def refused_operands(entry, offsets, ws_off):
    """the operands of this placement the headers let the entry point refuse, in argument order"""
    e = ENTRIES[entry]
    bad = [o for o in e.operands if REFUSED.get((e.cname, o)) and offsets.get(o, 0) % REFUSED[(e.cname, o)]]
    if e.ws and ws_off % REFUSED[(e.cname, 'ws')]:
        bad.append('ws')
    return bad


# ---------------------------------------------------------------------------------------------------------------- cases
def _pick(cases, *keys):
    out = []
    for key in keys:
        hit = [c for c in cases if c[:len(key)] == key]
        assert len(hit) == 1, (key, hit)
        out.append(hit[0])
    return out


# F(2x2,3x3), (n, h, w, c, k, padding, ldx, ldy) from W.CASES: VALID with an N tail, tiles that are mostly padding, pixel strides
# wider than the channels; and the scalar one
W_FLIP = _pick(W.CASES, (2, 6, 8, 32, 200, 'VALID'), (1, 2, 3, 8, 8, 'SAME'), (3, 13, 18, 32, 200, 'SAME', 40, 208))
W_SCALAR = _pick(W.CASES, (1, 9, 9, 5, 7, 'SAME'))
# the pool form, (case, h2, w2, pitch of the pooled map): the smallest odd and even unpooled extents tests/test_gpu_wino_bwd.py
# runs, and its scalar entry (a pooled map whose pixel stride is off the 16-byte grid)
POOL_CASE = (2, 5, 6, 8, 8, 'SAME', None, None)
POOL_FLIP = [(POOL_CASE, 11, 13, None), (POOL_CASE, 10, 12, None)]
POOL_SCALAR = [(POOL_CASE, 11, 13, 9)]
# F(4,5), (n, h, w, c, k, r, padding, ldx, ldy) from W1.CASES
L_FLIP = _pick(W1.CASES, (2, 3, 6, 8, 12, 5, 'SAME', 12, 16), (2, 7, 8, 8, 12, 5, 'VALID'), (2, 5, 9, 8, 12, 3, 'SAME'))
L_SCALAR = _pick(W1.CASES, (1, 9, 9, 6, 5, 5, 'VALID', 7, 9))
# the fused momentum launch, (m, k, n): no host decision reads an address there (the kernel takes any 4-byte address)
MOMENTUM = [(33, 130, 128), (5, 1000, 67)]


def flip_cases(entry):
    """the cases chosen to flip a decision: vectorised on the grid"""
    if entry == 'momentum':
        return []
    if 'pool' in entry:
        return POOL_FLIP
    return W_FLIP if ENTRIES[entry].family == 'w' else L_FLIP


def scalar_cases(entry):
    """the cases that are scalar wherever they lie"""
    if entry == 'momentum':
        return MOMENTUM
    if 'pool' in entry:
        return POOL_SCALAR
    return W_SCALAR if ENTRIES[entry].family == 'w' else L_SCALAR


def cases(entry):
    return flip_cases(entry) + scalar_cases(entry)


def channels_of(entry, case):
    """(c, k, ldx, ldy[, pitch of the pooled map]) of a case: what the host decisions test beside the addresses"""
    if entry == 'momentum':
        return case[1], case[2], case[1], case[2]
    extra = ()
    if 'pool' in entry:
        case, _, _, ldp = case
        extra = (ldp or case[3],)
    c, k = case[3], case[4]
    return (c, k, case[-2] or c, case[-1] or k) + extra


def vectorisable(entry, case):
    return all(v % 4 == 0 for v in channels_of(entry, case))


def case_id(case):
    if isinstance(case[0], tuple):
        return case_id(case[0]) + f'-pool{case[1]}x{case[2]}' + (f'ld{case[3]}' if case[3] else '')
    return 'x'.join(str(v) for v in case if v is not None)


# ---- the dirty workspace (part C): beside the cases above, the filter gradients at more than one split and bwd-data where the
# stream-K fix-up has work
W_SPLIT = (13, 13, 18, 256, 384, 'SAME', None, None)
# conv2d_1's shape at n = 1 is one split under the rule (9 k-tiles, W1.grad_splits); the uneven splits of W1.CASES are 6 + 6 + 5
# k-tiles at (2, 27, 37, 8, 12) and 7 + 7 + 7 + 5 at n = 3 of conv2d_1's shape: all three are run
L_SPLIT = _pick(W1.CASES, (1, 27, 37, 96, 256, 5, 'SAME'), (2, 27, 37, 8, 12, 5, 'SAME'), (3, 27, 37, 96, 256, 5, 'SAME'))


def streamk_shared_tiles(case):
    """the tiles of a plane of a3dl_conv2d_bwd_data's products that two stream-K shares meet in: the plane's tiles x nk (tile,
    k-tile) iterations, tile-major, are dealt to `blocks` contiguous shares, share b starting at b * total // blocks (sk_first,
    csrc/igemm.h); a share boundary inside a tile leaves that tile to the fix-up"""
    g = W1.bwd_data_geometry(*case[:7])
    total = g['tiles'] * g['nk']
    firsts = {b * total // g['blocks'] for b in range(1, g['blocks'])}
    return sorted({f // g['nk'] for f in firsts if f % g['nk']})


L_STREAMK = [c for c in W1.CASES if streamk_shared_tiles(c) and c[0] * c[1] * c[2] * max(c[3], c[4]) < 1 << 19]
L_STREAMK = [min((c for c in L_STREAMK if W1.bwd_data_geometry(*c[:7])['bn'] == bn), key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4])
             for bn in sorted({W1.bwd_data_geometry(*c[:7])['bn'] for c in L_STREAMK})]


def dirty_cases(entry):
    """the cases whose workspace is filled with NaN bytes before the call"""
    fam = ENTRIES[entry].family
    if 'pool' in entry:      # ... and conv2d_2 of the network at n = 3, as tests/test_gpu_wino_bwd.py pools it: a larger workspace
        return POOL_FLIP[:1] + POOL_SCALAR + [((3, 13, 18, 384, 256, 'SAME', None, None), 27, 37, None)]
    if fam == 'w':
        return W_FLIP + W_SCALAR + ([W_SPLIT] if entry.startswith(('wg_', 'wb')) else [])
    extra = L_SPLIT if entry == 'l_bwd_filter' else [c for c in L_STREAMK if c not in L_FLIP + L_SCALAR]
    return L_FLIP + L_SCALAR + extra


# ---------------------------------------------------------------------------------------------------------------- part D
# Non-finite inputs stay in their window.  A plant is (operand, image, row, column, channel, value).  NaN goes to an interior pixel
# of image 0, +Inf to a border pixel of the last image; with one image the two are two runs, so that no image holds two.
CLEAN_SHARE = 0.75

W_NONFINITE = [W_FLIP[2], W_SCALAR[0]]                                   # the 13 x 18 and the 9 x 9 maps
L_NONFINITE = [L_FLIP[1], L_SCALAR[0]]                                   # the 7 x 8 and the 9 x 9 maps
# a3dl_conv2d_bwd_data: an 8-column window and the r = 5 rows above it cover 40 of the 56 (7 x 8) or 81 (9 x 9) pixels of those
# maps, so no plant leaves three quarters of them clean; the 27 x 37 map of W1.CASES does
L_NONFINITE_BWD_DATA = _pick(W1.CASES, (2, 27, 37, 8, 12, 5, 'SAME'))
NONFINITE_ENTRIES = ('fwd', 'fwd_prepared', 'bwd_data', 'bwd_data_prepared', 'wg_bwd_filter_db', 'wb', 'wb_prepared', 'l_bwd_data',
                     'l_bwd_data_prepared', 'l_bwd_filter')


def nonfinite_cases(entry):
    if ENTRIES[entry].family == 'w':
        return W_NONFINITE
    return L_NONFINITE_BWD_DATA if entry.startswith('l_bwd_data') else L_NONFINITE


def plant_operands(entry):
    """the inputs of an entry a non-finite element is planted in, one at a time (never the filter: it reaches every output)"""
    return ('x',) if 'fwd' in entry else ('dz',) if 'bwd_data' in entry else ('x', 'dz')


def shapes(entry, case):
    """(n, h, w, c, k, r, s, pad_t, pad_l, ho, wo) of a case of either family"""
    if ENTRIES[entry].family == 'w':
        n, h, w, c, k, padding = case[:6]
        ho, wo, pt, pl = W.geometry(h, w, padding)
        return n, h, w, c, k, 3, 3, pt, pl, ho, wo
    n, h, w, c, k, r, padding = case[:7]
    ho, wo, pt, pl = W1.geometry(h, w, r, padding)
    return n, h, w, c, k, r, 5, pt, pl, ho, wo


def plants(entry, case, operand):
    """the runs of a case: [[plant, ...], ...] for the operand 'x' or 'dz'"""
    n, h, w, c, k, r, s, pt, pl, ho, wo = shapes(entry, case)
    hh, ww, ch = (h, w, c) if operand == 'x' else (ho, wo, k)
    nan = (operand, 0, hh // 2, ww // 2, ch // 2, float('nan'))
    inf = (operand, n - 1, hh - 1, 0, ch // 2, float('inf'))
    return [[nan, inf]] if n > 1 else [[nan], [inf]]


def _window_tiles(pos, tile, first, width, count):
    """the tiles t < count whose window [tile * t + first, tile * t + first + width) holds pos"""
    return [t for t in range(count) if tile * t + first <= pos < tile * t + first + width]


def conv_sets(src_hw, out_hw, taps, pads, tile, window, image, py, px, n):
    """(must, may) as boolean [n][oh][ow]: outputs of a correlation with `taps` = (r, s) at origin -pads whose receptive field
    holds source pixel (py, px) of `image`; and the other outputs of the tiles (tile = (rows, columns) of outputs, window = (rows,
    columns) of source pixels starting at tile * t - pads) whose window holds it"""
    (oh, ow), (r, s), (pt, pl) = out_hw, taps, pads
    must = np.zeros((n, oh, ow), bool)
    may = np.zeros((n, oh, ow), bool)
    for oy in range(oh):
        for ox in range(ow):
            must[image, oy, ox] = oy - pt <= py < oy - pt + r and ox - pl <= px < ox - pl + s
    for ti in _window_tiles(py, tile[0], -pt, window[0], -(-oh // tile[0])):
        for tj in _window_tiles(px, tile[1], -pl, window[1], -(-ow // tile[1])):
            may[image, tile[0] * ti:tile[0] * (ti + 1), tile[1] * tj:tile[1] * (tj + 1)] = True
    assert not (must & ~may).any(), 'an output the element reaches lies outside every window that holds it'
    return must, may & ~must


def nonfinite_sets(entry, case, run):
    """{output: (must, may, clean)} boolean arrays in the output's own shape (channels of a wider pixel stride excluded), for one
    run of plants(entry, case, .).  must: non-finite; may: either; clean: the bits of the run without the plants."""
    n, h, w, c, k, r, s, pt, pl, ho, wo = shapes(entry, case)
    fam = ENTRIES[entry].family
    out = {}

    def merge(name, shape, must, may):
        m0, a0 = out.get(name, (np.zeros(shape, bool), np.zeros(shape, bool)))
        out[name] = (m0 | must, a0 | may)

    for operand, image, py, px, ch, _ in run:
        if 'fwd' in entry or 'bwd_data' in entry or (entry.startswith('wb') and operand == 'dz'):
            fwd = 'fwd' in entry
            assert operand == ('x' if fwd else 'dz')
            src, dst, pads, chans = ((h, w), (ho, wo), (pt, pl), k) if fwd else ((ho, wo), (h, w), (r - 1 - pt, s - 1 - pl), c)
            if fam == 'w':
                must, may = conv_sets(src, dst, (3, 3), pads, (2, 2), (4, 4), image, py, px, n)
            else:      # the window's rows are a direct r x 1 convolution: a 1-row tile whose window is its receptive field
                must, may = conv_sets(src, dst, (r, 5), pads, (1, 4), (r, 8), image, py, px, n)
            name = 'y' if fwd else 'dx'
            rep = lambda a: np.repeat(a[..., None], chans, axis=-1)      # noqa: E731
            merge(name, (n,) + dst + (chans,), rep(must), rep(may))
        if 'bwd_filter' in entry or entry.startswith('wb'):
            must = np.zeros((r, s, c, k), bool)
            may = np.zeros((r, s, c, k), bool)
            dbm = np.zeros((k,), bool)
            for a in range(r):
                for b in range(s):
                    if operand == 'x':      # the tap (a, b) reaches x (py, px) from output (py + pt - a, px + pl - b)
                        must[a, b, ch, :] = 0 <= py + pt - a < ho and 0 <= px + pl - b < wo
                    else:                   # ... and output (py, px) reads x (py - pt + a, px - pl + b) through it
                        must[a, b, :, ch] = 0 <= py - pt + a < h and 0 <= px - pl + b < w
            if operand == 'x':
                may[:, :, ch, :] = True
            else:
                may[:, :, :, ch] = True
                dbm[ch] = True
            merge('dw', (r, s, c, k), must, may & ~must)
            merge('db', (k,), dbm, np.zeros((k,), bool))
            if entry.startswith('wb') and operand == 'x':      # the chain's dx does not read x
                merge('dx', (n, h, w, c), np.zeros((n, h, w, c), bool), np.zeros((n, h, w, c), bool))
    return {name: (must, may & ~must, ~(must | may)) for name, (must, may) in out.items()}


def clean_share(sets):
    total = sum(m.size for m, _, _ in sets.values())
    return sum(int(cl.sum()) for _, _, cl in sets.values()) / total


# ---------------------------------------------------------------------------------------------------------------- operands
def ternary_operands(case, seed=71):
    """x, w, bias, dz and a ReLU mask (laid out as x) of an F(2x2,3x3) case in {-1, 0, 1}: under W.headroom / the filter gradient's
    bound every value of the routes is exact, so the float64 oracle is the reference element for element"""
    n, h, w, c, k, padding = case[:6]
    ho, wo, _, _ = W.geometry(h, w, padding)
    rng = np.random.default_rng(seed)
    return dict(x=W.ternary(rng, (n, h, w, c)), w=W.ternary(rng, (3, 3, c, k)), bias=W.ternary(rng, (k,)),
                dz=W.ternary(rng, (n, ho, wo, k)), mask=W.ternary(rng, (n, h, w, c)))


def pool_operands(case, seed=72):
    """argmax bytes 0..3 and the pooled map (a third of its maxima not above zero) of a pool case"""
    (n, h, w, c, k, padding, _, _), h2, w2, ldp = case
    rng = np.random.default_rng(seed)
    arg = rng.integers(0, 4, (n, h, w, c)).astype(np.uint8)
    y = rng.standard_normal((n, h, w, c)).astype(np.float32)
    y[np.abs(y) < 0.4] = 0.0
    return arg, y


def unpool(dx, arg, y, h2, w2):
    """what a3d_maxpool2x2_bwd_idx(relu_mask = 1) writes from the pooled-size dx: each value, where its pooled maximum is above
    zero, at window position arg (0..3 = row-major in the 2x2 window), zeros elsewhere, the odd last row / column included"""
    n, h, w, c = dx.shape
    out = np.zeros((n, h2, w2, c), np.float64)
    g = np.where(y > 0, dx, 0.0)
    for pos in range(4):
        out[:, pos // 2:2 * h:2, pos % 2:2 * w:2] = np.where(arg == pos, g, 0.0)
    return out
