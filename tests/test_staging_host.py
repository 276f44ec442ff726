"""CPU: hybridgl_amd/staging.py -- the pinned pool and the harvest queue that decide when a staging buffer may be overwritten --
with events whose completion the test sets."""
import torch

from hybridgl_amd.staging import HarvestQueue, PinnedPool


class Event:
    def __init__(self, done=False):
        self.done, self.waits = done, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.waits += 1
        self.done = True


def test_drain_stops_at_an_incomplete_head_and_keeps_the_order():
    q = HarvestQueue(PinnedPool())
    evs = [Event(), Event(True), None, Event(True)]
    for k, ev in enumerate(evs):
        q.put(ev, k)
    assert len(q) == 4 and q and list(q) == [0, 1, 2, 3]
    assert list(q.drain()) == [] and len(q) == 4      # later entries are complete, the head is not
    evs[0].done = True
    evs[3].done = False
    assert list(q.drain()) == [0, 1, 2] and list(q) == [3]      # an entry without an event is complete
    assert list(q.drain()) == [] and len(q) == 1
    evs[3].done = True
    assert list(q.drain()) == [3] and not q and len(q) == 0
    assert all(ev.waits == 0 for ev in evs if ev is not None)


def test_drain_wait_synchronises_every_entry_once():
    q = HarvestQueue(PinnedPool())
    evs = [Event(), Event(True), None, Event()]
    for k, ev in enumerate(evs):
        q.put(ev, k)
    assert list(q.drain(wait=True)) == [0, 1, 2, 3] and not q
    assert [ev.waits for ev in evs if ev is not None] == [1, 1, 1]
    assert list(q.drain(wait=True)) == []


def test_a_buffer_in_flight_returns_after_its_payload_was_consumed():
    pool = PinnedPool()
    q = HarvestQueue(pool)
    a, b = pool.take(10, torch.int32), pool.take(10, torch.float64)
    q.put(Event(True), "first", (a, b))
    q.put(None, "empty")
    assert len(pool) == 0 and pool.take(10, torch.int32).data_ptr() != a.data_ptr()
    d = q.drain()
    assert next(d) == "first"
    assert len(pool) == 0 and pool.take(10, torch.int32).data_ptr() != a.data_ptr()      # the consumer still reads its views
    assert next(d) == "empty"
    assert {x.data_ptr() for x in pool} == {a.data_ptr(), b.data_ptr()}
    assert list(d) == [] and len(pool) == 2
    assert pool.take(10, torch.int32) is a and pool.take(3, torch.float64) is b


def test_a_buffer_given_with_an_event_waits_for_it():
    pool = PinnedPool()
    buf, ev = pool.take(100, torch.int32), Event()
    pool.give(buf, ev)
    other = pool.take(100, torch.int32)
    assert other.data_ptr() != buf.data_ptr() and len(pool) == 1 and ev.waits == 0
    ev.done = True
    assert pool.take(100, torch.int32) is buf and len(pool) == 0


def test_take_matches_dtype_and_size_and_honours_the_floor():
    pool = PinnedPool()
    small, wide = pool.take(0, torch.int32), pool.take(7, torch.float64)
    assert small.numel() == 1 and wide.numel() == 7 and small.dtype == torch.int32      # floor=1: max(numel, 1)
    pool.give(small)
    pool.give(wide)
    got = pool.take(5, torch.int32)      # `small` is too short, `wide` is of another dtype
    assert got.dtype == torch.int32 and got.numel() == 5 and len(pool) == 2
    assert pool.take(7, torch.float64) is wide and pool.take(1, torch.int32) is small and len(pool) == 0
    pool.give(got)
    assert pool.take(6, torch.int32) is not got and pool.take(2, torch.int32) is got      # the first that is large enough
    big = PinnedPool(floor=4096)
    assert big.take(10, torch.int32).numel() == 4096 and big.take(5000, torch.int32).numel() == 5000
    assert got.is_pinned() == torch.cuda.is_available()


def test_two_takes_never_share_storage():
    pool = PinnedPool()
    a = pool.take(16, torch.int32)
    pool.give(a)
    b, c = pool.take(16, torch.int32), pool.take(16, torch.int32)
    assert b is a and c.data_ptr() != b.data_ptr() and len(pool) == 0
