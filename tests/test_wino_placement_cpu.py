"""tests/wino_placement.py, the table behind tests/test_gpu_wino_placement.py, checked without a GPU: the shape of every entry's
sweep; that the cases chosen to flip a host decision are vectorised on the grid and that every decision's every operand is moved
alone by some entry; the refusal table against the headers' own words; the bound under which the ternary operands are exact; the
dirty-workspace cases (more than one split, uneven splits, stream-K tiles that two shares meet in); and the sets of outputs a
non-finite input must, may and must not reach — against the numpy restatements of the routes with the element planted, and
against the cap on the share of outputs a test may leave unchecked."""
import os
import re

import numpy as np
import pytest

import wino1d_ref as W1
import wino_grad_ref as WG
import wino_placement as P
import wino_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    return ' '.join(open(os.path.join(ROOT, 'include', name)).read().replace(' * ', ' ').split())


@pytest.mark.parametrize('entry', sorted(P.ENTRIES))
def test_the_sweep_of_every_entry(entry):
    e = P.ENTRIES[entry]
    sw = P.sweep(entry)
    assert sw[0] == ('on-grid', {}, 0)
    placements = [(offs, ws) for _, offs, ws in sw[1:]]
    for o in e.operands:
        assert ({o: 4}, 0) in placements, o
        assert (P.operand_type(entry, o) == 'u8') == (({o: 1}, 0) in placements), o
    assert e.image in e.operands and P.operand_type(entry, e.image) == 'f32' and ({e.image: 8}, 0) in placements
    assert ({o: 1 if P.operand_type(entry, o) == 'u8' else 12 for o in e.operands}, 0) in placements
    assert (({}, 16) in placements) == (({}, 4) in placements) == e.ws
    assert len({label for label, _, _ in sw}) == len(sw) == 1 + len(e.operands) + len(e.types) + 2 + 2 * e.ws
    for _, offs, ws in sw:
        assert all(0 < b < 256 and b % P.ELEMENT_BYTES[P.operand_type(entry, o)] == 0 and b % 16 for o, b in offs.items())
        assert set(offs) <= set(e.operands) and (not offs or ws == 0)
    assert ('argmax' in e.operands) == ('pool' in entry) and set(e.types) <= set(e.operands)


def test_the_entries_are_the_surfaces_the_headers_declare():
    """every C name is declared by a header and bound; the operands are named as the declaration names them"""
    from ann3depth_amd import _lib
    bound = {}
    for s in (_lib.SIGNATURES, _lib.WINO_SIGNATURES, _lib.WINO_GRAD_SIGNATURES, _lib.WINO_BWD_SIGNATURES, _lib.WINO1D_SIGNATURES,
              _lib.OPTIM_SIGNATURES):
        bound.update(s)
    alias = {'U': ('w', 'w_or_U'), 'w': ('w', 'w_or_U'), 'mask': ('relu_mask',), 'argmax': ('pool',), 'pool_y': ('pool',)}
    text = {h: header(h) for h in ('a3d.h', 'a3d_wino.h', 'a3d_wino_grad.h', 'a3d_wino_bwd.h', 'a3d_wino1d.h', 'a3d_optim.h')}
    for entry, e in P.ENTRIES.items():
        assert e.cname in bound, entry
        decl = [m.group(1) for t in text.values() for m in re.finditer(rf'\bint {e.cname}\(([^;]*)\);', t)]
        assert len(decl) == 1, entry
        names = [re.findall(r'\w+', a)[-1] for a in decl[0].split(',')]
        at = -1
        for o in e.operands:      # in argument order
            hits = [names.index(a) for a in alias.get(o, (o,)) if a in names]
            assert hits and hits[0] >= at, (entry, o, names)
            at = hits[0]
        assert e.ws == ('ws' in names), entry
    assert {e.cname for e in P.ENTRIES.values()} >= {'a3dwg_conv2d_bwd_filter', 'a3dwb_conv2d_bwd', 'a3dl_conv2d_bwd_data',
                                                     'a3dl_conv2d_bwd_filter', 'a3do_dense_bwd_filter_momentum'}
    assert sum('prepare_filter' in e.cname for e in P.ENTRIES.values()) == 3


def test_every_decision_is_flipped_by_one_operand_at_a_time():
    for entry in P.ENTRIES:
        for case in P.flip_cases(entry):
            assert P.vectorisable(entry, case), (entry, case)      # on the grid: the 16-byte kernels
        assert any(not P.vectorisable(entry, c) for c in P.cases(entry)), entry      # scalar wherever it lies
        assert P.flip_cases(entry) or entry == 'momentum'
    # the entries through which each decision is reached, and the operands whose address it reads
    reach = {'wino_input': ('fwd', 'bwd_data', 'wg_bwd_filter'), 'wino_output': ('fwd', 'bwd_data_mask'), 'wino_dz': ('wg_bwd_filter_db',),
             'wino_bwd_transforms': ('wb',), 'wino_bwd_finish': ('wb_mask', 'wb_pool'), 'wino1d_input': ('l_bwd_data', 'l_bwd_filter'),
             'wino1d_dz': ('l_bwd_filter',), 'wino1d_output': ('l_bwd_data_mask',)}
    assert set(reach) == set(P.DECISIONS) and len(P.DECISIONS) == 8
    for decision, operands in P.DECISIONS.items():
        for o in operands:
            moved = [e for e in reach[decision] if any(offs == {o: 4} for _, offs, _ in P.sweep(e)) and P.flip_cases(e)]
            assert moved, (decision, o)
    assert any(offs == {'argmax': 1} for _, offs, _ in P.sweep('wb_pool'))
    # the prepared and the per-call forms of an entry share their cases
    for entry in P.ENTRIES:
        if '_prepared' in entry:
            assert P.cases(entry) == P.cases(entry.replace('_prepared', ''))


def test_the_refusal_table_is_the_headers():
    h = {n: header(n) for n in ('a3d.h', 'a3d_wino.h', 'a3d_wino_grad.h', 'a3d_wino_bwd.h', 'a3d_wino1d.h', 'a3d_optim.h')}
    assert '`ws`, where it is not NULL, must be 16-byte aligned' in h['a3d.h']
    for name in ('a3d_wino_grad.h', 'a3d_wino_bwd.h', 'a3d_wino1d.h'):
        assert 'ws: 16-byte aligned' in h[name], name
    for name in ('a3d.h', 'a3d_wino.h', 'a3d_wino1d.h'):
        assert 'into a caller-owned, 16-byte aligned buffer' in h[name], name
    assert 'the tensors need 4-byte alignment only' in h['a3d_optim.h']
    assert 'an argmax row start at any multiple of its element size' in h['a3d.h'] or 'any multiple of its element size' in h['a3d.h']
    assert set(P.REFUSED.values()) == {16} and {o for _, o in P.REFUSED} == {'ws', 'U', 'prepared'}
    for entry, e in P.ENTRIES.items():
        for label, offs, ws in P.sweep(entry):
            bad = P.refused_operands(entry, offs, ws)
            want = [o for o in e.operands if o in ('U', 'prepared') and offs.get(o, 0) % 16] + (['ws'] if ws % 16 else [])
            assert bad == want, (entry, label)
        assert P.refused_operands(entry, {'argmax': 1} if 'argmax' in e.operands else {}, 16) == []
    assert set(P.NAMED_AS) == {o for _, o in P.REFUSED}


@pytest.mark.parametrize('case', P.W_FLIP + P.W_SCALAR + [P.POOL_CASE], ids=P.case_id)
def test_ternary_operands_keep_the_headroom_bounds(case):
    """forward and bwd-data under W.headroom, the filter gradient under WG.headroom: the float64 oracle is then the reference of
    every F(2x2,3x3) entry element for element"""
    t = P.ternary_operands(case)
    padding = case[5]
    stats = {}
    W.fwd(t['x'], t['w'], padding, stats)
    assert stats['max_v'] <= 4 and stats['max_u'] <= 9 / 4 and W.headroom(stats) < 2 ** 24
    W.bwd_data(t['dz'], t['w'], t['x'].shape, padding, stats)
    assert stats['channels'] == case[4] and W.headroom(stats) < 2 ** 24
    WG.bwd_filter(t['x'], t['dz'], padding, stats)
    assert stats['max_v'] <= 4 and stats['max_z'] <= 4 and WG.headroom(stats) < 2 ** 22
    assert abs(t['bias']).max() <= 1


def test_the_pool_reference():
    """P.unpool against the definition, window by window"""
    case = P.POOL_SCALAR[0]
    arg, y = P.pool_operands(case)
    n, h, w, c = arg.shape
    dx = np.random.default_rng(3).integers(-9, 10, (n, h, w, c)).astype(np.float64)
    got = P.unpool(dx, arg, y, case[1], case[2])
    assert got.shape == (n, 11, 13, c) and (got[:, -1] == 0).all() and (got[:, :, -1] == 0).all()
    for i in range(h):
        for j in range(w):
            win = got[:, 2 * i:2 * i + 2, 2 * j:2 * j + 2].reshape(n, 4, c)
            for pos in range(4):
                assert (win[:, pos] == np.where((arg[:, i, j] == pos) & (y[:, i, j] > 0), dx[:, i, j], 0)).all()
    assert (y <= 0).mean() > 0.25 and set(np.unique(arg)) == {0, 1, 2, 3}
    assert [(c[1] % 2, c[2] % 2) for c in P.POOL_FLIP] == [(1, 1), (0, 0)]


def test_the_dirty_workspace_cases():
    n, h, w, c, k, padding = P.W_SPLIT[:6]
    assert WG.splits(c, k, n * 7 * 9) > 1 and P.W_SPLIT in P.dirty_cases('wg_bwd_filter_db') and P.W_SPLIT in P.dirty_cases('wb_prepared')
    shares = []
    for case in P.L_SPLIT:
        n, h, w, c, k, r, padding = case[:7]
        shares.append(W1.ktile_shares(n * h * -(-w // 4), W1.grad_splits(r * c, k, n * h * -(-w // 4))))
        assert case in P.dirty_cases('l_bwd_filter')
    assert shares == [[9], [6, 6, 5], [7, 7, 7, 5]]      # one split, and the two uneven divisions among W1.CASES
    # bwd-data: a tile two stream-K shares meet in, at both product tiles that occur among W1.CASES
    assert {W1.bwd_data_geometry(*cs[:7])['bn'] for cs in W1.CASES} == {96, 128}
    assert [W1.bwd_data_geometry(*cs[:7])['bn'] for cs in P.L_STREAMK] == [96, 128]
    for cs in P.L_STREAMK:
        g = W1.bwd_data_geometry(*cs[:7])
        assert g['blocks'] > 1 and P.streamk_shared_tiles(cs) and cs in W1.CASES
        assert cs in P.dirty_cases('l_bwd_data') and cs in P.dirty_cases('l_bwd_data_prepared')
    # the rule itself on a hand-worked plane: 5 tiles x 2 k-tiles to 2 shares of 5 -> the boundary lies inside tile 2
    assert P.streamk_shared_tiles((2, 27, 37, 8, 12, 5, 'SAME')) == [2]
    assert P.streamk_shared_tiles((2, 7, 8, 8, 12, 5, 'VALID')) == []
    for entry, e in P.ENTRIES.items():
        if e.ws:
            assert set(P.cases(entry)) & set(P.dirty_cases(entry)), entry


# ---------------------------------------------------------------------------------------------------------------- part D
def planted(entry, case, run):
    """the outputs of the numpy restatement of the entry's route, clean and with the run's elements planted"""
    fam = P.ENTRIES[entry].family
    rng = np.random.default_rng(9)
    n, h, w, c, k, r, s, pt, pl, ho, wo = P.shapes(entry, case)
    ops = dict(x=rng.standard_normal((n, h, w, c)).astype(np.float32), dz=rng.standard_normal((n, ho, wo, k)).astype(np.float32),
               w=rng.standard_normal((r, s, c, k)).astype(np.float32))
    padding = case[5] if fam == 'w' else case[6]

    def route(o):
        out = {}
        if 'fwd' in entry:
            out['y'] = W.fwd(o['x'], o['w'], padding)
        if 'bwd_data' in entry or entry.startswith('wb'):
            out['dx'] = W.bwd_data(o['dz'], o['w'], o['x'].shape, padding) if fam == 'w' else W1.bwd_data(o['dz'], o['w'], o['x'].shape, padding)
        if 'bwd_filter' in entry or entry.startswith('wb'):
            out['dw'], out['db'] = WG.bwd_filter(o['x'], o['dz'], padding) if fam == 'w' else W1.bwd_filter(o['x'], o['dz'], r, padding)
        return out
    clean = route(ops)
    dirty = {name: a.copy() for name, a in ops.items()}
    for operand, image, py, px, ch, value in run:
        dirty[operand][image, py, px, ch] = value
    with np.errstate(invalid='ignore'):
        return clean, route(dirty)


RUNS = [(e, c, o, i) for e in P.NONFINITE_ENTRIES for c in P.nonfinite_cases(e) for o in P.plant_operands(e)
        for i in range(len(P.plants(e, c, o)))]


@pytest.mark.parametrize('entry,case,operand,i', RUNS, ids=lambda v: P.case_id(v) if isinstance(v, tuple) else str(v))
def test_the_geometric_sets(entry, case, operand, i):
    run = P.plants(entry, case, operand)[i]
    sets = P.nonfinite_sets(entry, case, run)
    n, h, w, c, k, r, s, pt, pl, ho, wo = P.shapes(entry, case)
    assert P.clean_share(sets) >= P.CLEAN_SHARE, P.clean_share(sets)
    assert len({image for _, image, *_ in run}) == len(run)                      # one planted element an image
    for op, image, py, px, ch, value in run:
        hh, ww = (h, w) if op == 'x' else (ho, wo)
        border = py in (0, hh - 1) or px in (0, ww - 1)
        assert border == np.isinf(value) and (border or np.isnan(value)) and image == (n - 1 if border else 0)
    clean, dirty = planted(entry, case, run)
    assert set(sets) == set(clean)
    for name, (must, may, keep) in sets.items():
        assert must.shape == clean[name].shape and not (must & may).any() and (must | may | keep).all()
        bad = ~np.isfinite(dirty[name])
        assert np.isfinite(clean[name]).all()
        assert bad[must].all(), f'{name}: an output the element reaches came out finite'
        assert not bad[keep].any() and (dirty[name][keep].view(np.uint32) == clean[name][keep].view(np.uint32)).all(), name
    assert sum(int(m.sum()) for m, _, _ in sets.values()) > 0


def test_the_named_maps_and_the_one_that_cannot():
    """the 13 x 18, 7 x 8 and 9 x 9 maps are the cases; a3dl_conv2d_bwd_data takes the 27 x 37 one, because an 8-column window and
    the 5 rows above it cover 40 of the 56 / 81 pixels of the small maps, whatever is planted"""
    assert [c[1:3] for c in P.W_NONFINITE] == [(13, 18), (9, 9)] and [c[1:3] for c in P.L_NONFINITE] == [(7, 8), (9, 9)]
    for case in P.L_NONFINITE:
        for run in P.plants('l_bwd_data', case, 'dz'):
            assert P.clean_share(P.nonfinite_sets('l_bwd_data', case, run)) < P.CLEAN_SHARE
    assert P.L_NONFINITE_BWD_DATA[0] in W1.CASES and P.L_NONFINITE_BWD_DATA[0][1:3] == (27, 37)
    assert set(P.NONFINITE_ENTRIES) >= {'fwd', 'bwd_data', 'wg_bwd_filter_db', 'wb', 'l_bwd_data', 'l_bwd_filter'}
    for entry in P.NONFINITE_ENTRIES:
        if 'U' in P.ENTRIES[entry].operands:
            assert entry.replace('_prepared', '') in P.NONFINITE_ENTRIES
