"""Evaluation on the test split without a GPU: the ordered test-split reader, the C ABI's argument checks of
a3d_depth_metrics, the float64 numpy reference of its per-image sums (used by tests/test_gpu_eval.py too) against
hand-computed cases, ops.summarize_depth_metrics, and the evaluation CLI's refusals (exit code 2)."""
import ctypes
import os

import numpy as np
import pytest

COLS = ('n', 'abs_rel', 'sq_rel', 'sq', 'log', 'log_sq', 'log10', 'delta1', 'delta2', 'delta3', 'nonfinite')


def ref_rows(pred, target, min_depth=0., max_depth=np.inf, clamp_lo=1e-3, clamp_hi=np.inf, magnitude=False):
    """float64 reference of a3d_depth_metrics for pred / target on the SAME grid [n, h, w] (a caller compares at another
    resolution by resampling pred with oracle.tf13_ops.resize_bilinear_tf1 first, which the kernel reproduces bit for
    bit).  Validity, clamp and the ratio of the delta counts in float32, as the kernel; the continuous terms in float64.
    magnitude=True: the sums of |term| instead (the scale a continuous column is compared at)."""
    p = np.asarray(pred, np.float32).reshape(len(pred), -1)
    t = np.asarray(target, np.float32).reshape(len(target), -1)
    rows = np.zeros((len(p), len(COLS)))
    f = np.abs if magnitude else (lambda v: v)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        valid = np.isfinite(t) & (t > np.float32(min_depth)) & (t <= np.float32(max_depth))
        bad = valid & ~np.isfinite(p)
        ok = valid & np.isfinite(p)
        for b in range(len(p)):
            q32 = np.minimum(np.maximum(p[b][ok[b]], np.float32(clamp_lo)), np.float32(clamp_hi))
            t32 = t[b][ok[b]]
            ratio = np.maximum(q32 / t32, t32 / q32)                      # float32, correctly rounded division
            q, tt = q32.astype(np.float64), t32.astype(np.float64)
            diff = q - tt
            d = np.log(q) - np.log(tt)
            rows[b] = [ok[b].sum(), (np.abs(diff) / tt).sum(), (diff * diff / tt).sum(), (diff * diff).sum(), f(d).sum(),
                       (d * d).sum(), np.abs(np.log10(q) - np.log10(tt)).sum(), (ratio < np.float32(1.25)).sum(),
                       (ratio < np.float32(1.5625)).sum(), (ratio < np.float32(1.953125)).sum(), bad[b].sum()]
    return rows


# ---------------------------------------------------------------------------------------------- ordered reader
def _write(root, n, u8=True, split='test', shape=(6, 8), dshape=(3, 4)):
    from ann3depth_amd import tfrecord
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    rng = np.random.default_rng(5)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', f'{split}.tfrecords')) as w:
        for i in range(n):
            if u8:     # the converter's form png_u8 / 255 - 0.5; pixel (0, 0) carries the record number
                img = rng.integers(0, 256, shape + (3,)).astype(np.float32)
                img[0, 0, 0] = i
                img = img / np.float32(255) - np.float32(.5)
                dep = np.full(dshape + (1,), i, np.float32) / np.float32(255) - np.float32(.5)
            else:      # arbitrary floats: staged as float32
                img = rng.standard_normal(shape + (3,)).astype(np.float32)
                img[0, 0, 0] = i + 0.25
                dep = np.full(dshape + (1,), i + 0.125, np.float32)
            w.write_example(img, dep)


def _number(pipe, slot, u8):
    if u8:
        assert pipe.kind[slot] == 3                     # both features staged as uint8 pixel values
        return int(pipe.images_u8[slot, 0, 0, 0])
    assert pipe.kind[slot] == 0
    return int(pipe.images[slot, 0, 0, 0] - 0.5 + 0.25)


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('threads', [1, 4])
def test_ordered_reader_yields_each_record_once_in_file_order(tmp_path, u8, threads):
    from ann3depth_amd import data
    _write(str(tmp_path), 13, u8=u8)
    inputs, targets = data.inputs(str(tmp_path), 'nyu', 4, 'test', shuffle=False, num_threads=threads)
    pipe = inputs.pipeline
    assert targets.pipeline is pipe and isinstance(pipe, data.OrderedBatch)
    pipe.allocate(alloc_u8=lambda shape: np.empty(shape, np.uint8))
    sizes, seen = [], []
    while True:
        try:
            slots = pipe.dequeue()
        except data.OutOfRangeError:
            break
        sizes.append(len(slots))
        seen += [_number(pipe, s, u8) for s in slots]
        for s in slots:                                  # the float32 the loader would have produced, on demand
            img = pipe.materialise(s, 0)
            assert img.dtype == np.float32 and img.shape == (6, 8, 3)
        pipe.release(slots)
    assert sizes == [4, 4, 4, 1]
    assert seen == list(range(13))
    with pytest.raises(data.OutOfRangeError):
        pipe.dequeue()
    pipe.close()


def test_ordered_reader_next_batch_stacks_short_last_batch(tmp_path):
    from ann3depth_amd import data
    _write(str(tmp_path), 13, u8=False)
    inputs, _ = data.inputs(str(tmp_path), 'nyu', 4, 'test', shuffle=False)
    pipe = inputs.pipeline
    got = []
    for want in (4, 4, 4, 1):
        img, dep = pipe.next_batch()
        assert img.shape == (want, 6, 8, 3) and dep.shape == (want, 3, 4, 1)
        got += [float(v) for v in dep[:, 0, 0, 0]]
    assert got == [i + 0.125 + 0.5 for i in range(13)]
    with pytest.raises(data.OutOfRangeError):
        pipe.next_batch()


def test_ordered_reader_with_a_pool_smaller_than_the_split(tmp_path):
    """More records than slots: readers must wait for released slots and still deliver in order."""
    from ann3depth_amd import data
    _write(str(tmp_path), 61, u8=True)
    inputs, _ = data.inputs(str(tmp_path), 'nyu', 2, 'test', shuffle=False, num_threads=3)
    pipe = inputs.pipeline
    pipe.allocate(alloc_u8=lambda shape: np.empty(shape, np.uint8))
    assert pipe.nslots < 61
    seen = []
    while True:
        try:
            slots = pipe.dequeue()
        except data.OutOfRangeError:
            break
        seen += [_number(pipe, s, True) for s in slots]
        pipe.release(slots)
    assert seen == list(range(61))


def test_default_inputs_still_shuffle_full_batches_only(tmp_path):
    from ann3depth_amd import data
    _write(str(tmp_path), 13, u8=False, split='train')
    inputs, _ = data.inputs(str(tmp_path), 'nyu', 4, epochs=1, seed=1)
    pipe = inputs.pipeline
    assert type(pipe) is data.ShuffleBatch
    sizes = []
    while True:
        try:
            img, _ = pipe.next_batch()
        except data.OutOfRangeError:
            break
        sizes.append(img.shape[0])
    assert sizes == [4, 4, 4]                            # the partial last batch is dropped


# ---------------------------------------------------------------------------------------------- C ABI checks
def test_depth_metrics_rejects_bad_arguments_before_any_launch(lib):
    """A3D_EINVAL / A3D_EWORKSPACE come before any device work: these calls pass host pointers that a launch would
    fault on, and no GPU is needed."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    need = lib.a3d_depth_metrics_ws_bytes(2, 55, 74)
    assert 0 < need <= 1 << 16
    assert lib.a3d_depth_metrics_ws_bytes(0, 55, 74) == 0
    assert lib.a3d_depth_metrics_ws_bytes(2, 0, 74) == 0
    assert lib.a3d_depth_metrics_ws_bytes(2, 480, 640) > need                  # more workgroups per image

    def call(n=2, ph=55, pw=74, pred=p, th=55, tw=74, tgt=p, u8=0, lo=0., hi=float('inf'), clo=1e-3, chi=float('inf'),
             rows=p, ws=p, ws_bytes=need):
        return lib.a3d_depth_metrics(n, ph, pw, pred, th, tw, tgt, u8, lo, hi, clo, chi, rows, ws, ws_bytes, None)
    EINVAL, EWORKSPACE = -1, -2
    for kw in ({'n': 0}, {'n': -3}, {'ph': 0}, {'pw': -1}, {'th': 0}, {'tw': 0}, {'pred': None}, {'tgt': None},
               {'rows': None}, {'lo': float('nan')}, {'chi': float('nan')}, {'clo': 2.0, 'chi': 1.0}):
        assert call(**kw) == EINVAL, kw
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert call(ws=None) == EWORKSPACE
    assert call(th=480, tw=640) == EWORKSPACE                                   # the workspace of the grid size is too small
    from ann3depth_amd import _lib
    assert 'workspace' in _lib.last_error()


# ---------------------------------------------------------------------------------------------- metrics on the host
def _summary(rows):
    from ann3depth_amd import ops
    return ops.summarize_depth_metrics(rows)


def test_reference_metrics_of_a_prediction_twice_the_target():
    rng = np.random.default_rng(0)
    t = rng.uniform(0.5, 10, (3, 5, 7)).astype(np.float32)
    s = _summary(ref_rows(2 * t, t))
    assert s['pixels'] == 105 and s['images'] == 3 and s['nonfinite'] == 0
    assert s['delta1'] == 0 and s['delta2'] == 0 and s['delta3'] == 0           # ratio 2 > 1.25^3
    assert s['abs_rel'] == pytest.approx(1, rel=1e-12)
    assert s['rmse_log'] == pytest.approx(np.log(2), rel=1e-12)
    assert s['log10'] == pytest.approx(np.log10(2), rel=1e-12)
    assert s['rmse_si'] == pytest.approx(0, abs=1e-6)                           # a global scale is forgiven
    assert s['sq_rel'] == pytest.approx(t.astype(np.float64).mean(), rel=1e-12)
    assert s['rmse'] == pytest.approx(np.sqrt((t.astype(np.float64) ** 2).mean()), rel=1e-12)


def test_reference_metrics_hand_computed():
    t = np.array([[[1.0, 2.0, 4.0, 0.0]]], np.float32)                          # the zero is not a valid target
    p = np.array([[[1.2, 3.0, np.nan, 5.0]]], np.float32)                       # NaN at a valid pixel: counted apart
    r = ref_rows(p, t)[0]
    assert r[0] == 2 and r[10] == 1
    assert r[1] == pytest.approx(np.float32(1.2) - 1 + 0.5, rel=1e-7)
    assert r[3] == pytest.approx((np.float32(1.2) - 1.0) ** 2 + 1.0, rel=1e-7)
    assert list(r[7:10]) == [1, 2, 2]                                           # 1.2 < 1.25; 1.5 < 1.5625
    d = np.log(np.float64(np.float32(1.2))) + np.log(1.5)
    assert r[4] == pytest.approx(d, rel=1e-12)
    # clamp: a negative prediction becomes clamp_lo; max_depth excludes the 4 and 2
    r = ref_rows(np.array([[[-1.0, 1.0, 1.0]]], np.float32), np.array([[[1.0, 2.0, 4.0]]], np.float32), max_depth=1.5)[0]
    assert r[0] == 1 and r[1] == pytest.approx(1 - np.float32(1e-3), rel=1e-7) and list(r[7:11]) == [0, 0, 0, 0]


def test_summary_handles_images_without_valid_pixels():
    t = np.ones((3, 2, 2), np.float32)
    t[1] = 0                                                                   # image 1: nothing valid
    p = np.ones((3, 2, 2), np.float32)
    p[2] *= np.float32(np.e)
    s = _summary(ref_rows(p, t))
    assert s['images'] == 3 and s['images_without_valid_pixels'] == 1 and s['pixels'] == 8
    assert s['delta1'] == 0.5 and s['rmse_log'] == pytest.approx(np.sqrt(0.5), rel=1e-6)
    assert s['rmse_si'] == pytest.approx(0, abs=1e-6)                           # images 0 and 2: constant d, none of image 1
    empty = _summary(np.zeros((2, len(COLS))))
    assert empty['pixels'] == 0 and empty['images_without_valid_pixels'] == 2
    assert np.isnan(empty['abs_rel']) and np.isnan(empty['rmse_si'])


def test_rmse_si_is_the_mean_over_images_of_the_per_image_variance():
    rows = np.zeros((2, len(COLS)))
    rows[0, [0, 4, 5]] = [2, 0.0, 2.0]            # d = +-1: variance 1
    rows[1, [0, 4, 5]] = [4, 4.0, 4.0]            # d = 1: variance 0
    assert _summary(rows)['rmse_si'] == pytest.approx(np.sqrt(0.5), rel=1e-12)
    assert _summary(rows)['rmse_log'] == pytest.approx(1.0, rel=1e-12)         # pooled: 6 / 6


# ---------------------------------------------------------------------------------------------- CLI refusals
def test_cli_refuses_without_a_checkpoint(tmp_path, capsys):
    from ann3depth_amd import evaluate
    _write(str(tmp_path), 3, split='test')
    rc = evaluate.main(['--ckptdir', str(tmp_path / 'ck'), '--datadir', str(tmp_path), '--id', 'r1', 'nyu'])
    assert rc == 2
    assert 'no checkpoint' in capsys.readouterr().err
    rc = evaluate.main(['--checkpoint', str(tmp_path / 'nothing.pt'), '--datadir', str(tmp_path), 'nyu'])
    assert rc == 2


def test_cli_refuses_dcnf_and_more_than_one_process(tmp_path, capsys, monkeypatch):
    from ann3depth_amd import evaluate
    assert evaluate.main(['--model', 'dcnf', '--datadir', str(tmp_path), 'nyu']) == 2
    assert 'dcnf' in capsys.readouterr().err.lower()
    monkeypatch.setenv('WORLD_SIZE', '2')
    assert evaluate.main(['--datadir', str(tmp_path), 'nyu']) == 2
    assert 'one process' in capsys.readouterr().err


def test_cli_refuses_without_a_test_split(tmp_path, capsys):
    from ann3depth_amd import evaluate
    _write(str(tmp_path), 3, split='train')                                     # a train split only
    run = tmp_path / 'ck' / 'msdn_r1'
    run.mkdir(parents=True)
    (run / 'model.ckpt-6.pt').write_bytes(b'')
    (run / 'checkpoint').write_text('model_checkpoint_path: "model.ckpt-6.pt"\n')
    rc = evaluate.main(['--ckptdir', str(tmp_path / 'ck'), '--datadir', str(tmp_path), '--id', 'r1', 'nyu'])
    assert rc == 2
    assert 'test.tfrecords' in capsys.readouterr().err
