"""feed.DeviceFeed driven directly over a real pipeline: a 5-record test split read in file order at B = 2, so the batches
are 2, 2 and 1 records (48x64x3 images, 6x8x1 depths, as tests/test_gpu_train.py writes its shards)."""
import collections
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def write_test_split(root, odd=None, n=5, seed=0):
    """n converter-form records; record `odd`, if any, holds one float that is no pixel value.  Returns what was stored."""
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'nyu'), exist_ok=True)
    stored = []
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'test.tfrecords')) as w:
        for i in range(n):
            img = rng.integers(0, 256, (48, 64, 3)).astype(np.float32) / np.float32(255) - np.float32(.5)
            dep = rng.integers(0, 256, (6, 8, 1)).astype(np.float32) / np.float32(255) - np.float32(.5)
            if i == odd:
                img[3, 4, 1] = np.nextafter(img[3, 4, 1], np.float32(1))
            w.write_example(img, dep)
            stored.append((img, dep))
    return stored


def open_feed(root, hook=None):
    """(feed, handed, released): the feed over the split, and the slot numbers its pipeline's dequeue() handed out and
    its release() got back, in order."""
    from ann3depth_amd import data, feed
    inputs, _ = data.inputs(root, 'nyu', batch_size=2, train_or_test='test', shuffle=False)
    pl = inputs.pipeline
    handed, released = [], []
    dequeue, release = pl.dequeue, pl.release

    def counting_dequeue():
        slots = dequeue()
        handed.extend(slots)
        return slots

    def counting_release(slots):
        released.extend(slots)
        release(slots)

    pl.dequeue, pl.release = counting_dequeue, counting_release
    f = feed.DeviceFeed(pl, 2, torch.device('cuda', torch.cuda.current_device()))
    f.start(hook)
    return f, handed, released


def host(t):
    """A batch tensor as the loader's float32: uint8 pixel values through data.expand_u8."""
    from ann3depth_amd import data
    a = t.cpu().numpy()
    return data.expand_u8(a) if a.dtype == np.uint8 else a


def test_batches_in_order_then_out_of_range_with_every_slot_released_once(tmp_path):
    from ann3depth_amd import data
    stored = write_test_split(str(tmp_path))
    hooked = []
    hook = lambda i, j: hooked.append((i, j))
    f, handed, released = open_feed(str(tmp_path), hook)
    try:
        first = 0
        for k, want_n in enumerate((2, 2, 1)):
            images, depths, n, i = f.take()
            torch.cuda.current_stream().synchronize()
            assert (n, i) == (want_n, k & 1)
            assert images.dtype == torch.uint8 and depths.dtype == torch.uint8        # converter-form records
            assert images.shape == (2, 48, 64, 3) and depths.shape == (2, 6, 8, 1)
            for which, t in enumerate((images, depths)):
                want = np.stack([stored[first + r][which] for r in range(n)]) + np.float32(.5)
                got = host(t[:n])
                assert got.dtype == np.float32
                np.testing.assert_array_equal(got, want)
            first += n
            assert f.due() is None                      # (b): nothing is due while a batch is out, not before the last either
            f.give_back(hook)
            assert (f.due() is None) == (k < 2)
        assert isinstance(f.due(), data.OutOfRangeError)
        with pytest.raises(data.OutOfRangeError) as e:
            f.take()
        assert e.value is f.due()
        assert hooked == [(0, 0), (1, 1), (0, 2)]       # (c): the dequeue for batch 3 raised before the hook
        assert len(handed) == 5 and collections.Counter(handed) == collections.Counter(released)     # (d)
        assert f.held == [[], []]
    finally:
        f.pipeline.close()


def test_the_batch_with_an_odd_record_arrives_as_float32_the_others_as_uint8(tmp_path):
    stored = write_test_split(str(tmp_path), odd=2)
    f, handed, released = open_feed(str(tmp_path))
    try:
        first = 0
        for k, want_n in enumerate((2, 2, 1)):
            images, depths, n, _ = f.take()
            torch.cuda.current_stream().synchronize()
            assert n == want_n
            assert images.dtype == (torch.float32 if k == 1 else torch.uint8)        # records 2 and 3 travel together
            assert depths.dtype == torch.uint8                                        # per feature: the depths are pixel values
            for which, t in enumerate((images, depths)):
                want = np.stack([stored[first + r][which] for r in range(n)]) + np.float32(.5)
                np.testing.assert_array_equal(host(t[:n]), want)
            first += n
            f.give_back()
        assert collections.Counter(handed) == collections.Counter(released) and len(handed) == 5
    finally:
        f.pipeline.close()
