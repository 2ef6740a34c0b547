"""What the DCNF wrappers of ann3depth_amd.ops refuse, and with which exception: one table over the nine wrappers whose
argument checks ops._check_crf, ops._check_operands and ops._check_superpixels hold, times the ways a call can be wrong.
Every rejection comes before the library or a stream is touched, so CPU tensors do (only the two-device rows need a GPU:
it is the second device).  Shapes: 2 images of 2 x 3 superpixels of edge 2, 2 pairs.

TIGHTENED lists the rows that were laxer before the checks were written once, and what those calls did then."""
import pytest
import torch

from ann3depth_amd import ops

N, ROWS, COLS, SP, Q, K = 2, 2, 3, 2, 2, 2
P = ROWS * COLS


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def i32(*values):
    return torch.tensor(values, dtype=torch.int32)


def crf(**more):
    return dict(z=f32(N, P), y=f32(N, P), r=f32(N, Q), left=i32(0, 1), right=i32(1, 2), **more)


def crf_map():
    a = crf()
    del a['y']
    return a


def similarity(**more):
    return dict(x=f32(N, ROWS * SP, COLS * SP, 3), sp=SP, hist=f32(N, P, 256), **more, left=i32(0, 1), right=i32(1, 2),
                dense_w=f32(K + len(more), 1), dense_b=f32(1))


# wrapper -> (its good arguments, the operand that rank, dtype, contiguity and device defects hit, the operand that gets
# one image too many, the int32 operand)
WRAPPERS = {
    'crf_loss': (crf, 'z', 'r', 'left'),
    'crf_loss_grad': (crf, 'z', 'y', 'left'),
    'crf_loss_observed': (crf, 'z', 'r', 'right'),
    'crf_map': (crf_map, 'z', 'r', 'left'),
    'pair_similarity': (similarity, 'x', 'hist', 'left'),
    'pair_similarity3': (lambda: similarity(lbp_hist=f32(N, P, 256)), 'x', 'lbp_hist', 'right'),
    'superpixel_lbp_hist': (lambda: dict(x=f32(N, ROWS * SP, COLS * SP, 3), sp=SP, out=f32(N, P, 256)), 'x', 'out', None),
    'superpixel_mean_valid': (lambda: dict(x=f32(N, ROWS * SP, COLS * SP, 1), sp=SP, out=f32(N, P),
                                           count=torch.zeros((N, P), dtype=torch.int32)), 'x', 'out', 'count'),
    'pair_dense_bwd': (lambda: dict(sims=f32(N, Q, K), dr=f32(N, Q), dw=f32(K, 1), db=f32(1)), 'sims', 'dr', None),
}
DEFECTS = {'rank': ValueError, 'n': ValueError, 'unequal': ValueError, 'empty': ValueError, 'float64': TypeError,
           'int64': TypeError, 'strided': ValueError, 'devices': ValueError}
# (wrapper, defect) -> what the call did before this table existed
TIGHTENED = {
    ('crf_map', 'rank'): 'z [n, P, 1] was launched as [n, P]',
    ('crf_map', 'empty'): 'the library refused the launch (RuntimeError)',
}


def broken(name, defect):
    """The wrapper's good arguments with one defect, or None where the wrapper has no such operand."""
    make, main, partner, index = WRAPPERS[name]
    a = make()
    if defect == 'rank':
        a[main] = a[main].unsqueeze(-1)
    elif defect == 'n':
        a[partner] = torch.zeros((N + 1,) + tuple(a[partner].shape[1:]), dtype=a[partner].dtype)
    elif defect == 'unequal':
        if 'right' not in a:
            return None
        a['right'] = i32(1, 2, 0)
    elif defect == 'empty':
        if 'right' in a:
            a['left'] = a['right'] = i32()
            if 'r' in a:
                a['r'] = f32(N, 0)
        elif name == 'pair_dense_bwd':
            a['sims'], a['dr'] = f32(N, 0, K), f32(N, 0)
        else:
            return None
    elif defect == 'float64':
        a[main] = a[main].double()
    elif defect == 'int64':
        if index is None:
            return None
        a[index] = a[index].long()
    elif defect == 'strided':
        shape = tuple(a[main].shape)
        a[main] = torch.zeros(shape[:-1] + (2 * shape[-1],))[..., ::2]
        assert tuple(a[main].shape) == shape and not a[main].is_contiguous()
    elif defect == 'devices':
        a[main] = a[main].cuda()
    return a


ROWS_OF_THE_TABLE = [pytest.param(name, defect, marks=[pytest.mark.gpu] if defect == 'devices' else [],
                                  id=f'{name}-{defect}' + ('-tightened' if (name, defect) in TIGHTENED else ''))
                     for name in WRAPPERS for defect in DEFECTS if defect == 'devices' or broken(name, defect) is not None]


class ReachedTheLibrary(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    """The wrappers' first step after their checks is _lib.load(): here it launches nothing."""
    def load():
        raise ReachedTheLibrary
    monkeypatch.setattr(ops._lib, 'load', load)


@pytest.mark.parametrize('name', WRAPPERS)
def test_the_good_arguments_pass_every_check(no_library, name):
    with pytest.raises(ReachedTheLibrary):
        getattr(ops, name)(**WRAPPERS[name][0]())


@pytest.mark.parametrize('name,defect', ROWS_OF_THE_TABLE)
def test_a_wrong_argument_is_refused_before_the_library_is_touched(no_library, name, defect):
    with pytest.raises(DEFECTS[defect], match=name):
        getattr(ops, name)(**broken(name, defect))
