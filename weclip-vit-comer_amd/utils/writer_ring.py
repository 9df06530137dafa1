"""The output ring every file-writing entry point shares: `depth` (device, pinned host) buffer pairs, ONE asynchronous copy and
one event per commit, and `writers` host threads that turn the host bytes into files.

    slot = ring.next_slot()                          # waits until the pair is free: at most `depth` jobs are in flight
    ring.carve(slot, [("pred", (H, W), torch.uint8), ...])
    ... kernels write slot.views["pred"] ...
    ring.commit(slot, job)                           # the copy, the event, and (slot, job) is queued
    ... a writer thread calls ring._write(slot, job), which waits for slot.copied and reads ring.host(slot, "pred") ...
    ring.finish()                                    # -> jobs written; raises the first exception of a writer

A subclass names its sections and directories and supplies `_write`: msc_flip_eval.WriterPool, predict.PredictWriterPool,
clip.cam_seeds.BucketWriter, train.PanelWriter.  The buffers only grow; nothing is allocated per job.  Importing needs no GPU."""
import math
import queue
import threading

import torch


class _Slot:
    """One buffer pair of the ring: `dev` the kernels write, `host` (pinned) the writers read, one event for the copy between."""

    def __init__(self, event):
        self.dev = self.host = None
        self.copied = event
        self.free = threading.Event()
        self.free.set()
        self.views = None


def _cuda_alloc(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _cuda_event():
    return torch.cuda.Event()


class WriterRing:
    """writers / depth: host threads and buffer pairs (default depth: two per writer).  alloc / event: the device side (tests
    pass host stand-ins).  `job` is whatever the subclass's `_write(slot, job)` takes: a name, a list of names, an iteration."""

    def __init__(self, writers=4, depth=None, alloc=_cuda_alloc, event=_cuda_event, thread_name="weclip-write"):
        self.writers = max(1, int(writers))
        self.depth = max(1, int(depth)) if depth else 2 * self.writers
        self._alloc = alloc
        self.slots = [_Slot(event()) for _ in range(self.depth)]
        self._next = 0
        self.jobs = queue.Queue(maxsize=self.depth)
        self.error = None
        self.written = 0
        self._lock = threading.Lock()
        self.threads = [threading.Thread(target=self._work, name=f"{thread_name}-{i}", daemon=True) for i in range(self.writers)]
        for t in self.threads:
            t.start()

    def next_slot(self, block=True):
        """The next slot of the ring once its writer has freed it.  block=False: queue.Full when it is still in flight."""
        slot = self.slots[self._next]
        if not slot.free.wait(None if block else 0):
            raise queue.Full(f"{type(self).__name__}: all {self.depth} buffers are in flight")
        self._next = (self._next + 1) % self.depth
        return slot

    def carve(self, slot, sections, align=4):
        """sections [(key, shape, dtype)] laid end to end, each starting at a multiple of `align` bytes: slot.views[key] on the
        device buffer, grown (with a quarter of headroom) when it is too small.  -> slot.used, the bytes `commit` copies."""
        spans, pos = {}, 0
        for key, shape, dtype in sections:
            end = pos + math.prod(shape) * dtype.itemsize     # (host time here delays the first launch of every job: keep it lean)
            spans[key] = (pos, end, tuple(shape), dtype)
            pos = -(-end // align) * align
        if slot.dev is None or slot.dev.numel() < pos:
            slot.dev, slot.host = self._alloc(int(pos * 1.25))
        slot.spans, slot.used = spans, pos
        slot.views = {key: self._view(slot.dev, span) for key, span in spans.items()}
        return pos

    @staticmethod
    def _view(buf, span):
        a, b, shape, dtype = span
        part = buf[a:b]
        return (part if dtype == torch.uint8 else part.view(dtype)).view(shape)

    def host(self, slot, key):
        """The section `key` of the slot's host buffer as a numpy array (a writer's view of it, after slot.copied)."""
        return self._view(slot.host, slot.spans[key]).numpy()

    def commit(self, slot, job):
        slot.free.clear()
        slot.host[:slot.used].copy_(slot.dev[:slot.used], non_blocking=True)
        slot.copied.record()
        self.jobs.put((slot, job))

    def _write(self, slot, job):
        raise NotImplementedError

    def _work(self):
        while True:
            item = self.jobs.get()
            try:
                if item is None:
                    return
                slot, job = item
                try:
                    self._write(slot, job)
                    with self._lock:
                        self.written += 1
                except BaseException as e:                                    # kept for finish(); the slot is freed either way
                    with self._lock:
                        if self.error is None:
                            self.error = e
                finally:
                    slot.free.set()
            finally:
                self.jobs.task_done()

    def finish(self):
        """Wait for every queued job, end the threads, raise the first writer exception.  -> number of jobs written."""
        self.jobs.join()
        for _ in self.threads:
            self.jobs.put(None)
        for t in self.threads:
            t.join()
        self.threads = []
        if self.error is not None:
            raise self.error
        return self.written

    def drain(self):
        """`finish()` for a caller that still has a collective to go through: -> the exception instead of raising it, or None."""
        try:
            self.finish()
        except BaseException as e:
            return e
        return None
