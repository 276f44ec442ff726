"""Pinned host memory between the device and the host, and the one rule for when a buffer may be overwritten.

PinnedPool    the free buffers: take(numel, dtype) / give(buf, event), the event behind a copy that still reads buf (an upload)
HarvestQueue  the device -> host copies in flight, oldest first: put(event, payload, buffers) / drain(wait)

Events are used through query() and synchronize() alone; without a device the buffers are plain host memory."""
import collections

import torch


class PinnedPool:
    def __init__(self, floor=1):
        self.floor = int(floor)      # a new buffer has at least this many elements
        self._free = []              # (buffer, the event that must have completed before it is taken again, or None)

    def __len__(self):
        return len(self._free)

    def __iter__(self):
        return (b for b, _ in self._free)

    def take(self, numel, dtype):
        """the first buffer of dtype with at least numel elements that nothing in flight reads, or a new one; it leaves the pool"""
        for i, (buf, ev) in enumerate(self._free):
            if buf.dtype == dtype and buf.numel() >= numel and (ev is None or ev.query()):
                del self._free[i]
                return buf
        return torch.empty(max(int(numel), self.floor), dtype=dtype, pin_memory=torch.cuda.is_available())

    def give(self, buf, event=None):
        self._free.append((buf, event))


class HarvestQueue:
    def __init__(self, pool):
        self.pool = pool
        self._q = collections.deque()      # (event, or None: nothing to wait for; payload; the pool's buffers the copy fills)

    def __len__(self):
        return len(self._q)

    def __iter__(self):      # the payloads in flight
        return (p for _, p, _ in self._q)

    def put(self, event, payload, buffers=()):
        self._q.append((event, payload, tuple(buffers)))

    def drain(self, wait=False):
        """Yields the payloads of the entries whose copies have completed, oldest first, and stops at the first that has not
        (wait=True: waits for each, yields all).  An entry's buffers return to the pool when the consumer comes back for the
        next payload: it has read its numpy views of them by then."""
        while self._q and (self._q[0][0] is None or wait or self._q[0][0].query()):
            event, payload, buffers = self._q.popleft()
            if event is not None and wait:
                event.synchronize()
            yield payload
            for b in buffers:
                self.pool.give(b)
