"""Scale-and-shift alignment without a GPU: the host reference of tests/align_ref.py (used by tests/test_gpu_align.py too)
against hand cases, and the --align refusals of the two inference drivers (exit code 2 before any GPU work)."""
from fractions import Fraction

import numpy as np
import pytest

import align_ref as R


def test_exact_least_squares_on_dyadic_values():
    p = (np.arange(12, dtype=np.float32).reshape(1, 3, 4) + 1) / np.float32(8)
    r = R.ref_align(p, 2 * p + np.float32(0.25), 'affine')
    assert r['coef'].tolist() == [[2.0, 0.25]] and r['count'].tolist() == [12] and r['status'].tolist() == [0]
    assert 1 < r['kappa'][0] < 100
    r = R.ref_align(p, 3 * p, 'scale')
    assert r['coef'].tolist() == [[3.0, 0.0]] and r['status'].tolist() == [0]
    # a constant prediction: the denominator of 'affine' is 0; 'scale' still fits
    c = np.full((1, 3, 4), 0.75, np.float32)
    r = R.ref_align(c, p, 'affine')
    assert r['coef'].tolist() == [[1.0, 0.0]] and r['status'].tolist() == [1] and r['count'].tolist() == [12]
    assert R.ref_align(c, p, 'scale')['status'].tolist() == [0]
    # one pixel: 'scale' and 'median' fit it, 'affine' needs two
    t = np.zeros((1, 3, 4), np.float32)
    t[0, 1, 2] = 4
    for mode, want in (('scale', [[4 / 0.75, 0.0]]), ('median', [[4 / 0.75, 0.0]]), ('affine', [[1.0, 0.0]])):
        r = R.ref_align(c, t, mode)
        assert r['count'].tolist() == [1] and r['coef'].tolist() == np.array(want, np.float32).tolist(), mode


def test_fl32_rounds_a_fraction_once():
    assert R.fl32(Fraction(1, 3)) == np.float32(1) / np.float32(3)
    tie = Fraction(1) + Fraction(1, 2 ** 24)                            # halfway between 1 and the next float32: to even
    assert R.fl32(tie) == np.float32(1) and R.fl32(tie + Fraction(1, 2 ** 60)) == np.nextafter(np.float32(1), np.float32(2))
    assert R.fl32(-tie) == np.float32(-1)
    assert np.isinf(R.fl32(Fraction(2) ** 128)) and R.fl32(Fraction(0)) == 0
    assert R.fl32(Fraction(float(np.finfo(np.float32).max))) == np.finfo(np.float32).max


def test_lower_median_of_odd_and_even_counts_ties_and_signed_zeros():
    f = np.float32
    assert R.lower_median(f([3, 1, 2])) == 2
    assert R.lower_median(f([4, 1, 3, 2])) == 2                         # rank (4 - 1) // 2 = 1: the lower one, no averaging
    assert R.lower_median(f([5, 5, 5, 1, 9, 5])) == 5
    assert R.lower_median(f([7])) == 7
    z = R.lower_median(f([0.0, -0.0]))                                  # -0 sorts before +0
    assert z == 0 and np.signbit(z)
    z = R.lower_median(f([0.0, -0.0, 0.0, -0.0, 1.0]))
    assert z == 0 and not np.signbit(z)
    assert R.lower_median(f([-1, -2, -3, 1e-45, 1e-40])) == -1
    k = R.order_key(f([-np.inf, -1, -1e-45, -0.0, 0.0, 1e-45, 1, np.inf]))
    assert (np.diff(k) > 0).all()
    assert all(R.key_value(v).tobytes() == x.tobytes() for v, x in zip(k, f([-np.inf, -1, -1e-45, -0.0, 0.0, 1e-45, 1, np.inf])))


def test_median_mode_and_its_refusals():
    t = np.float32([[[1, 2, 3, 4]]])
    p = np.float32([[[2, 4, 6, 8]]])
    r = R.ref_align(p, t, 'median')
    assert r['coef'].tolist() == [[0.5, 0.0]] and r['status'].tolist() == [0]
    assert R.ref_align(-p, t, 'median')['status'].tolist() == [1]                      # med(p) <= 0
    assert R.ref_align(-p, t, 'median')['coef'].tolist() == [[1.0, 0.0]]
    assert R.ref_align(np.float32([[[0, 0, 0, 1]]]), t, 'median')['status'].tolist() == [1]


def test_holes_and_nonfinite_predictions_are_left_out():
    t = np.float32([[[1, np.nan, 3, 0, 5, 20]]])                                        # NaN, 0 and (max_depth 10) 20: holes
    p = np.float32([[[1, 7, np.nan, 7, 5, 7]]])                                         # NaN on a valid pixel: left out
    for mode in R.MODES:
        r = R.ref_align(p, t, mode, max_depth=10.)
        assert r['count'].tolist() == [2] and r['status'].tolist() == [0], mode
        assert r['coef'].tolist() == [[1.0, 0.0]]
    rows = R.aligned_rows(p, t, np.float32([[2, 1]]), max_depth=10.)
    assert rows[0, 0] == 2 and rows[0, 10] == 1                                         # ... and counted in column 10
    assert rows[0, 3] == (2 * 1 + 1 - 1) ** 2 + (2 * 5 + 1 - 5) ** 2
    # a target of another size: the prediction is sampled at its pixels
    r = R.ref_align(np.float32([[[1, 2], [3, 4]]]), np.ones((1, 4, 4), np.float32), 'scale')
    assert r['count'].tolist() == [16]
    assert R.sampled(np.float32([[[1, 2], [3, 4]]]), 4, 4)[0, 0].tolist() == [1, 1.5, 2, 2]


def test_apply_is_two_float32_roundings():
    x = np.float32([[1 + 2 ** -23, np.nan, np.inf, -0.0]])
    y = R.apply(x, np.float32([[1 + 2 ** -23, 1]]))
    assert y[0, 0] == np.float32(np.float32(x[0, 0] * x[0, 0]) + np.float32(1))
    assert np.isnan(y[0, 1]) and np.isinf(y[0, 2])
    assert R.ulps(np.float32([1, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- the drivers' flags
def test_evaluate_takes_align_and_refuses_an_unknown_mode(capsys):
    from ann3depth_amd import evaluate, ops
    assert ops.ALIGN_MODES == ('median', 'scale', 'affine')
    assert evaluate.parse_args(['nyu']).align == 'none'
    for mode in ops.ALIGN_MODES:
        assert evaluate.parse_args(['--align', mode, 'nyu']).align == mode
    with pytest.raises(SystemExit) as e:
        evaluate.parse_args(['--align', 'log', 'nyu'])
    assert e.value.code == 2
    capsys.readouterr()


def test_predict_refuses_half_an_alignment_before_any_gpu_work(tmp_path, capsys):
    from ann3depth_amd import png, predict
    img = str(tmp_path / 'a.png')
    png.imsave(img, np.zeros((4, 5, 3), np.uint8))
    open(tmp_path / 'w.pt', 'wb').close()                               # a file is there; it is not read before the refusals
    out, to = str(tmp_path / 'out'), str(tmp_path / 'measured')
    base = ['--checkpoint', str(tmp_path / 'w.pt'), '--out', out]
    a = predict.parse_args(base + ['--align', 'affine', '--align-to', to, img])
    assert (a.align, a.align_to) == ('affine', to)
    assert predict.parse_args(base + [img]).align == 'none' and predict.parse_args(base + [img]).align_to == ''
    for model in ('msdn', 'dcnf'):
        assert predict.main(base + ['--model', model, '--align', 'affine', img]) == 2
        assert 'go together' in capsys.readouterr().err
        assert predict.main(base + ['--model', model, '--align-to', to, img]) == 2
        assert 'go together' in capsys.readouterr().err
        for lo, hi in (('2', '2'), ('3', '1')):
            assert predict.main(base + ['--model', model, '--align', 'scale', '--align-to', to, '--min-depth', lo,
                                        '--max-depth', hi, img]) == 2
            assert '--min-depth < --max-depth' in capsys.readouterr().err
        # a missing file, and one of another dtype, in the --depths message style
        assert predict.main(base + ['--model', model, '--align', 'median', '--align-to', to, img]) == 2
        assert '--align-to: cannot use' in capsys.readouterr().err
    (tmp_path / 'measured').mkdir()
    np.save(str(tmp_path / 'measured' / 'a.npy'), np.zeros((4, 5), np.float64))
    assert predict.main(base + ['--align', 'median', '--align-to', to, img]) == 2
    assert 'not a float32 [H, W] array' in capsys.readouterr().err
    assert predict.main(base + ['--model', 'dcnf', '--align', 'affine', '--align-to', to, '--depths', to, img]) == 2
    assert 'already uses the measurements' in capsys.readouterr().err
    assert predict.main(base + ['--model', 'msdn', '--align', 'affine', '--align-to', to, '--depths', to, img]) == 2
    assert 'regression without one' in capsys.readouterr().err          # --depths for msdn: refused as before
    with pytest.raises(SystemExit) as e:
        predict.parse_args(base + ['--align', 'log', '--align-to', to, img])
    assert e.value.code == 2
    capsys.readouterr()
    assert not (tmp_path / 'out').exists()
