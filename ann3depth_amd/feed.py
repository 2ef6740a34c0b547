"""The device feed: a data pipeline's batches in HBM, double-buffered, for the training op and the evaluation op alike."""
import ctypes

import numpy as np
import torch

from . import _lib, ops


class DeviceFeed:
    """The pipeline's staging pool is pinned memory; a dequeued batch is up to B slot numbers, DMA'd to HBM on a side
    stream into one of two device batch buffers.  Batch k+1 is in flight while batch k is being read, so host decode,
    PCIe transfer and the consumer's kernels overlap.

        images, depths, n, i = feed.take()      # batch k in buffer i = k & 1: B rows, the first n of them its records
        ...                                     # the consumer's work on the current stream
        feed.give_back()                        # buffer i is free for batch k + 2

    start() and give_back() are where batches are prefetched; both take an optional hook(i, j), which runs on the copy
    stream after the DMA of batch j into buffer i was issued and before the event that take() waits for is recorded: what
    it enqueues there travels under the batch's own event.  (The feed keeps no reference to it, so a consumer that passes
    a method of its own stays free of a reference cycle and gives its buffers back when it is dropped.)"""

    def __init__(self, pipeline, batchsize, device):
        self.pipeline = pipeline
        pipeline.allocate(lambda shape: torch.empty(shape, dtype=torch.float32).pin_memory().numpy(),
                          lambda shape: torch.empty(shape, dtype=torch.uint8).pin_memory().numpy())
        self.pool = (torch.from_numpy(pipeline.images), torch.from_numpy(pipeline.depths))      # pinned views
        # converter-written records are staged as uint8 pixel values (data.py): their own pinned pool and device buffers;
        # the resize kernel rebuilds the loader's float32 from them bit for bit
        self.pool_u8 = None
        if pipeline.images_u8 is not None:
            self.pool_u8 = (torch.from_numpy(pipeline.images_u8), torch.from_numpy(pipeline.depths_u8))
        self.dev = [tuple(torch.empty((batchsize,) + tuple(p.shape[1:]), device=device) for p in self.pool)
                    for _ in range(2)]
        self.dev_u8 = [tuple(torch.empty((batchsize,) + tuple(p.shape[1:]), device=device, dtype=torch.uint8) for p in self.pool)
                       for _ in range(2)] if self.pool_u8 is not None else None
        self.cur = [None, None]             # the (images, depths) tensors batch i was copied into: uint8 or float32 each
        self.copy_stream = torch.cuda.Stream(device=device)
        self.copied = [None, None]          # event: the DMA into buffer i finished
        self.consumed = [None, None]        # event: the consumer that read buffer i finished
        self.held = [[], []]                # pool slots buffer i was filled from
        self.k = 0                          # batches consumed
        self.end = None                     # (batch index, exception) once the pipeline ran dry

    def start(self, hook=None):
        """Put the first two batches in flight."""
        self._prefetch(0, hook)
        self._prefetch(1, hook)

    def _prefetch(self, j, hook=None):
        """Dequeue batch j and start its DMA into device buffer j & 1 on the copy stream."""
        if self.end is not None:
            return
        i = j & 1
        try:
            slots = self.pipeline.dequeue()
        except BaseException as e:          # raised to the caller when batch j would have been consumed
            self.end = (j, e)
            return
        if self.consumed[i] is not None:
            self.copy_stream.wait_event(self.consumed[i])
        pl = self.pipeline
        cur = []
        kinds = int(np.bitwise_and.reduce(pl.kind[slots])) if self.pool_u8 is not None else 0
        for which in (0, 1):                # images, depths: uint8 when EVERY record of the batch staged that feature so
            as_u8 = bool(kinds & (1 << which))
            if not as_u8 and self.pool_u8 is not None:
                for s in slots:
                    pl.materialise(s, which)                    # (a mixed batch: the uint8 records are expanded on the host)
            cur.append((self.dev_u8 if as_u8 else self.dev)[i][which])
        ids = (ctypes.c_int32 * len(slots))(*slots)
        with torch.cuda.stream(self.copy_stream):
            for which in (0, 1):
                src = (self.pool_u8 if cur[which].dtype == torch.uint8 else self.pool)[which]
                ops.check(_lib.load().a3d_h2d_gather(cur[which].data_ptr(), src.data_ptr(), ids, len(slots), len(src),
                                                     src[0].numel() * src.element_size(), self.copy_stream.cuda_stream),
                          'a3d_h2d_gather')                     # B copies from ONE call (no per-record host-language work)
            if hook is not None:
                hook(i, j)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.cur[i] = tuple(cur)
        self.copied[i] = ev
        self.held[i] = slots

    def redo(self, i, fn):
        """Run fn() on the copy stream once the copies into buffer i have finished, and let take() wait for it too: a
        fresh `copied` event behind what fn enqueued."""
        self.copied[i].synchronize()
        with torch.cuda.stream(self.copy_stream):
            fn()
            self.copied[i] = torch.cuda.Event()
            self.copied[i].record(self.copy_stream)

    def due(self):
        """The exception take() would raise now (the pipeline ran dry, or its reader failed, at or before batch k), or None."""
        return self.end[1] if self.end is not None and self.end[0] <= self.k else None

    def take(self):
        """Batch k on the current stream: (images, depths, n, buffer index)."""
        i = self.k & 1
        if self.end is not None and self.end[0] == self.k:
            raise self.end[1]
        torch.cuda.current_stream().wait_event(self.copied[i])
        return self.cur[i][0], self.cur[i][1], len(self.held[i]), i

    def give_back(self, hook=None):
        """The current stream's work so far is all that reads batch k: free its staging slots and refill its buffer."""
        i = self.k & 1
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.consumed[i] = ev
        self.copied[i].synchronize()        # issued a whole batch ago: the staging slots can go back to the readers
        self.pipeline.release(self.held[i])
        self.held[i] = []
        self.k += 1
        self._prefetch(self.k + 1, hook)    # into the buffer just read; the DMA waits for `consumed`
