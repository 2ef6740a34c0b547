"""CRF MAP inference without a GPU: the float64 reference of tests/crf_map_ref.py against hand-computed cases, the C
ABI's argument checks of a3d_crf_map, its presence in the header and the binding, and the evaluation CLI accepting
--model dcnf up to the checkpoint search."""
import ctypes
import os
import re

import numpy as np
import pytest

import crf_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('rows,cols', [(6, 8), (3, 4), (8, 8)])
def test_reference_with_no_pair_weights_returns_z(rows, cols):
    left, right = R.pairs(rows, cols)
    rng = np.random.default_rng(rows)
    z = rng.standard_normal((3, rows * cols)).astype(np.float32)
    y = R.solve(z, np.zeros((3, len(left)), np.float32), left, right)
    np.testing.assert_array_equal(y, z.astype(np.float64))
    np.testing.assert_array_equal(R.matrix(np.zeros(len(left)), rows * cols, left, right), np.eye(rows * cols))


def test_reference_two_nodes_one_pair_by_hand():
    """R = [[0, r], [r, 0]], A = [[1 + r, -r], [-r, 1 + r]], det = 1 + 2r, A^-1 = [[1 + r, r], [r, 1 + r]] / (1 + 2r)."""
    r, z = 0.75, np.array([[2.0, -1.0]])
    A = R.matrix([r], 2, [0], [1])
    np.testing.assert_array_equal(A, [[1.75, -0.75], [-0.75, 1.75]])
    y = R.solve(z, np.array([[r]]), [0], [1])
    want = np.array([(1 + r) * 2 - r, r * 2 - (1 + r)]) / (1 + 2 * r)          # [1.1, -0.1]
    np.testing.assert_allclose(y[0], want, rtol=1e-15)
    np.testing.assert_allclose(y[0], [1.1, -0.1], rtol=1e-14)
    # smoothing: the MAP depths lie between the unary outputs and keep their sum (rows of A sum to 1)
    assert y.sum() == pytest.approx(z.sum(), rel=1e-15)
    # r = -0.5 is the singular case the kernel must flag: A = [[.5, .5], [.5, .5]]
    np.testing.assert_array_equal(R.matrix([-0.5], 2, [0], [1]), [[0.5, 0.5], [0.5, 0.5]])


@pytest.mark.parametrize('rows,cols', [(6, 8), (3, 4), (8, 8)])
def test_reference_matrix_is_symmetric_with_unit_row_sums_and_is_the_oracles(rows, cols):
    left, right = R.pairs(rows, cols)
    rng = np.random.default_rng(cols)
    r = rng.uniform(-1.4, 1.4, len(left)).astype(np.float32)
    A = R.matrix(r, rows * cols, left, right)
    np.testing.assert_array_equal(A, A.T)
    np.testing.assert_allclose(A.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    if (rows, cols) == (6, 8):
        from oracle import dcnf as OD
        np.testing.assert_array_equal(A, OD.crf_matrix(r.astype(np.float64)))


def test_reference_scatter_lets_a_later_pair_overwrite_an_earlier_one():
    A = R.matrix([0.25, 2.0], 3, [0, 1], [1, 0])                                # the same edge twice
    np.testing.assert_array_equal(A, [[3.0, -2.0, 0.0], [-2.0, 3.0, 0.0], [0.0, 0.0, 1.0]])


def test_error_measures_on_known_perturbations():
    A = np.array([[2.0, 0.0], [0.0, 4.0]])
    z = np.array([2.0, 4.0])
    assert R.backward_error(A, [1.0, 1.0], z) == 0 and R.forward_error([1.0, 1.0], np.array([1.0, 1.0])) == 0
    # y_hat = [1, 1.5]: residual [0, 2]; ||A|| = 4, ||y_hat|| = 1.5, ||z|| = 4
    assert R.backward_error(A, [1.0, 1.5], z) == pytest.approx(2 / (4 * 1.5 + 4), rel=1e-15)
    assert R.forward_error([1.0, 1.5], np.array([1.0, 1.0])) == 0.5
    assert R.cond_inf(A) == 2.0 and R.U == 2.0 ** -24


# ---------------------------------------------------------------------------------------------- C ABI
def test_crf_map_is_declared_bound_and_documented():
    from ann3depth_amd import _lib, ops
    assert 'a3d_crf_map' in _lib.SIGNATURES and callable(ops.crf_map)
    header = open(os.path.join(ROOT, 'include', 'a3d.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int a3d_crf_map\(int n, int nsp, const float\* z, const float\* r, '
                  r'const int32_t\* left,\s*const int32_t\* right, int npairs,\s*float\* y, int32_t\* status, '
                  r'void\* stream\);', header, flags=re.S)
    assert m, 'include/a3d.h does not declare a3d_crf_map as specified'
    contract = m.group(1)
    assert 'src/models.py:136-143' in contract and 'NOT' in contract and 'NaN' in contract and 'status' in contract


def test_crf_map_rejects_bad_arguments_before_any_launch(lib):
    """A3D_EINVAL comes before any device work: these calls pass host pointers that a launch would fault on, and no
    GPU is needed."""
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def call(n=2, nsp=48, z=p, r=p, left=p, right=p, npairs=48, y=p, status=p):
        return lib.a3d_crf_map(n, nsp, z, r, left, right, npairs, y, status, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': -5}, {'nsp': 65}, {'npairs': 0}, {'npairs': -2}, {'z': None},
               {'r': None}, {'left': None}, {'right': None}, {'y': None}, {'y': None, 'status': None}):
        assert call(**kw) == -1, kw
    from ann3depth_amd import _lib
    assert 'crf_map' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written


# ---------------------------------------------------------------------------------------------- CLI
def test_cli_accepts_dcnf_up_to_the_checkpoint_search(tmp_path, capsys, monkeypatch):
    from ann3depth_amd import evaluate
    args = evaluate.parse_args(['--model', 'dcnf', '--resolution', 'record', '--predictions', 'p.npy', 'nyu'])
    assert args.model == 'dcnf' and args.resolution == 'record' and args.predictions == 'p.npy'
    assert evaluate.OUTPUTS['dcnf'] == ('unary', 'crf') and evaluate.OUTPUTS['msdn'] == ('coarse', 'fine')
    ck = tmp_path / 'ck'
    rc = evaluate.main(['--model', 'dcnf', '--ckptdir', str(ck), '--datadir', str(tmp_path), '--id', 'r1', 'nyu'])
    err = capsys.readouterr().err
    assert rc == 2 and 'no checkpoint' in err and os.path.join(str(ck), 'dcnf_r1') in err
    assert 'not implemented' not in err
    # a checkpoint but no test split: the search passed, the next refusal is the missing split (still no GPU touched)
    run = ck / 'dcnf_r1'
    run.mkdir(parents=True)
    (run / 'model.ckpt-3.pt').write_bytes(b'')
    (run / 'checkpoint').write_text('model_checkpoint_path: "model.ckpt-3.pt"\n')
    rc = evaluate.main(['--model', 'dcnf', '--ckptdir', str(ck), '--datadir', str(tmp_path), '--id', 'r1', 'nyu'])
    assert rc == 2 and 'test.tfrecords' in capsys.readouterr().err
    assert evaluate.main(['--model', 'nope', '--datadir', str(tmp_path), 'nyu']) == 2
    assert 'unknown model' in capsys.readouterr().err
    monkeypatch.setenv('WORLD_SIZE', '2')
    assert evaluate.main(['--model', 'dcnf', '--datadir', str(tmp_path), 'nyu']) == 2
    assert 'one process' in capsys.readouterr().err
