"""CPU: the bookkeeping of HybridGLPipeline.run(on_overflow="rescue") (hybridgl_amd/rescue.py) on fake snapshot totals.  The
driver below calls the ledger exactly where run() does: open a group, judge the stage-end snapshot recorded a group ago,
judge the total on the new group's read-back, and at the end of the loader judge what is left."""
import random
import sys

import pytest

from hybridgl_amd.rescue import LIMIT, Decision, RescueLedger


def drive(n_groups, stage_totals, read_totals=None, base=0):
    """run()'s calls for a loader of n_groups.  stage_totals[g] / read_totals[g]: the counters' total (relative to the last
    clear) a snapshot behind CLIP stage g / on the read-back of group g would show if the loop got there in split precision;
    a rescue clears the counters, so later totals are taken from the tables minus nothing -- the tables describe
    overflowing STAGES: total = base + number of listed stages at or before that point since the last clear.
    Returns (ledger, log) with log entries ("open", g), ("commit", [g]), ("rescue", [g...]), and the largest in-flight count."""
    led = RescueLedger(base)
    log, peak = [], 0
    groups = iter(range(1, n_groups + 1))
    cleared_at = 0      # stages of groups <= cleared_at no longer count

    def total(table, upto):
        return base_now[0] + sum(1 for g in table if cleared_at < g <= upto)

    base_now = [base]
    snaps = []          # gids whose stage-end snapshot is enqueued and not judged
    prev = None

    def rescue(d):
        nonlocal cleared_at, prev, snaps
        if d.pull_next:
            nxt = next(groups, None)
            if nxt is not None:
                led.open(nxt)
                log.append(("open", nxt))
        ids = led.in_flight()
        log.append(("rescue", ids))
        assert led.rescued(0) == ids
        cleared_at, prev, snaps = ids[-1], None, []
        base_now[0] = 0

    for g in groups:
        led.open(g)
        log.append(("open", g))
        peak = max(peak, len(led.in_flight()))
        assert len(led.in_flight()) <= LIMIT
        redone = False
        while snaps:
            h = snaps.pop(0)
            d = led.stage_end(h, total(stage_totals, h))
            if d.kind == "rescue":
                rescue(d)
                redone = True
                break
            log.append(("commit", d.groups))
        if not redone and read_totals is not None:
            # the read-back of group g sees the stage-end state of g - 2 plus its own proposal stage (and, by chance, the CLIP
            # stage beside it: the ledger must not care)
            d = led.read_back(total(stage_totals, g - 2) + sum(1 for x in read_totals if x == g))
            if d.kind == "rescue":
                rescue(d)
                redone = True
        if redone:
            continue
        if prev is not None:
            snaps.append(prev)
        prev = g
    if prev is not None:
        snaps.append(prev)
    while snaps:
        h = snaps.pop(0)
        d = led.stage_end(h, total(stage_totals, h))
        if d.kind == "rescue":
            rescue(d)
            break
        log.append(("commit", d.groups))
    return led, log, peak


def test_clean_run_commits_every_group_in_order_and_never_holds_more_than_three():
    led, log, peak = drive(7, stage_totals=[])
    assert led.committed == [1, 2, 3, 4, 5, 6, 7] and led.in_flight() == [] and led.events == 0
    assert peak == LIMIT == 3
    assert [e for e in log if e[0] == "rescue"] == []
    # group g commits while g + 2 is the newest: one group later than its snapshot was enqueued
    assert log[:6] == [("open", 1), ("open", 2), ("open", 3), ("commit", [1]), ("open", 4), ("commit", [2])]


def test_a_nonzero_total_at_the_start_is_the_baseline_not_an_overflow():
    led, _, _ = drive(4, stage_totals=[], base=5)
    assert led.committed == [1, 2, 3, 4] and led.events == 0


def test_a_fourth_group_cannot_be_opened_and_commits_cannot_skip():
    led = RescueLedger()
    for g in (1, 2, 3):
        led.open(g)
    with pytest.raises(RuntimeError):
        led.open(4)
    with pytest.raises(ValueError):
        led.stage_end(2, 0)            # the oldest in flight is 1
    assert led.stage_end(1, 0) == Decision("commit", [1])
    led.open(4)
    assert led.stage_end(2, 0) == Decision("commit", [2])
    with pytest.raises(ValueError):
        led.open(4)                    # out of order
    with pytest.raises(ValueError):
        led.open(2)                    # committed already


def test_moved_total_reruns_exactly_the_groups_in_flight_oldest_first_and_empties_the_pipeline():
    # the CLIP stage of group 3 overflows; its snapshot is judged while 3, 4, 5 are in flight
    led, log, peak = drive(8, stage_totals=[3])
    assert ("rescue", [3, 4, 5]) in log and led.events == 1 and led.rescued_groups == [3, 4, 5]
    assert led.committed == [1, 2, 3, 4, 5, 6, 7, 8] and peak <= LIMIT
    at = log.index(("rescue", [3, 4, 5]))
    assert log[at + 1] == ("open", 6)                      # the loop goes on with the next group ...
    assert log[at + 2] == ("open", 7)                      # ... and an empty pipeline: nothing to judge when 6 and 7 open
    assert log[at + 3] == ("open", 8) and log[at + 4] == ("commit", [6])


def test_payloads_and_the_oldest_checkpoint_are_what_a_rerun_needs():
    led = RescueLedger()
    led.open(1, "units-1")
    led.open(2, "units-2")
    assert led.oldest_checkpoint() is None                 # nothing logged yet: nothing to roll back
    led.checkpoint(1, "cp-1")
    led.checkpoint(2, "cp-2")
    led.open(3, "units-3")
    d = led.stage_end(1, 4)
    assert d == Decision("rescue", [1, 2, 3]) and not d.pull_next
    assert [led.payload(g) for g in d.groups] == ["units-1", "units-2", "units-3"]
    assert led.oldest_checkpoint() == "cp-1"
    assert led.rescued(0) == [1, 2, 3] and led.in_flight() == [] and led.base == 0
    led.open(4)
    assert led.stage_end(4, 0) == Decision("commit", [4])


def test_read_back_commits_nothing_and_pulls_the_next_group():
    led = RescueLedger()
    led.open(1)
    led.open(2)
    assert led.read_back(0) == Decision("commit", []) and led.in_flight() == [1, 2]
    d = led.read_back(9)
    assert d.kind == "rescue" and d.groups == [1, 2] and d.pull_next


def test_read_back_detection_gives_the_decision_the_stage_end_would_have_given():
    """An overflow in CLIP stage 3 may or may not be on the read-back of group 4 (the two run side by side): seen there or only
    in stage 3's own snapshot, the same groups are done again and the same groups commit in split precision."""
    late = drive(8, stage_totals=[3])
    early = drive(8, stage_totals=[3], read_totals=[])                       # read-backs in use, none sees it
    seen = RescueLedger()
    # by hand: groups 1..4 open, 1 and 2 committed, read-back of 4 moved
    for g in (1, 2, 3):
        seen.open(g)
    assert seen.stage_end(1, 0).kind == "commit"
    seen.open(4)
    assert seen.stage_end(2, 0).kind == "commit"
    d = seen.read_back(1)
    assert d.kind == "rescue" and d.pull_next and d.groups == [3, 4]
    seen.open(5)
    assert seen.in_flight() == [3, 4, 5] == late[0].rescued_groups == early[0].rescued_groups
    # an overflow of proposal stage 4 itself: always on its read-back, and in the snapshot behind CLIP stage 3
    led, log, _ = drive(8, stage_totals=[3], read_totals=[4])
    assert led.rescued_groups == [3, 4, 5] and led.events == 1


def test_moved_total_at_the_end_of_the_run_is_handled():
    for n, bad, want in ((5, 5, [5]), (5, 4, [4, 5]), (5, 3, [3, 4, 5]), (1, 1, [1]), (2, 1, [1, 2])):
        led, log, _ = drive(n, stage_totals=[bad])
        assert led.rescued_groups == want, (n, bad, led.rescued_groups)
        assert led.committed == list(range(1, n + 1)) and led.in_flight() == []
        assert log[-1] == ("rescue", want)


def test_every_group_overflowing_reruns_every_group_once():
    led, log, peak = drive(5, stage_totals=[1, 2, 3, 4, 5])
    assert led.rescued_groups == [1, 2, 3, 4, 5] and led.committed == [1, 2, 3, 4, 5] and peak <= LIMIT
    assert [e[1] for e in log if e[0] == "rescue"] == [[1, 2, 3], [4, 5]]


def test_the_same_event_sequence_gives_the_same_decisions():
    rng = random.Random(11)
    for _ in range(200):
        n = rng.randint(1, 12)
        bad = sorted(rng.sample(range(1, n + 1), rng.randint(0, min(n, 3))))
        rb = sorted(rng.sample(range(1, n + 1), rng.randint(0, min(n, 2)))) if rng.random() < 0.5 else None
        a, b = drive(n, bad, rb), drive(n, bad, rb)
        assert a[1] == b[1] and a[0].committed == b[0].committed == list(range(1, n + 1))
        assert a[2] <= LIMIT
        assert a[0].in_flight() == []
        # what is done again is made of whole groups, each once, in order
        r = a[0].rescued_groups
        assert r == sorted(set(r))
        for g in bad:
            assert g in r, (n, bad, rb, r)      # an overflowing CLIP stage never commits in split precision


def test_the_module_needs_no_gpu_and_no_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; import importlib.util as u, os; "
            "s = u.spec_from_file_location('rescue', os.path.join('hybridgl_amd', 'rescue.py')); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); assert m.RescueLedger().in_flight() == []")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
