"""Bookkeeping of HybridGLPipeline.run(on_overflow="rescue"): groups as transactions.  Pure Python, no GPU, no torch.

The fp16 range counters are process-wide and the proposal stage of group g+1 runs beside the CLIP stage of group g, so a
moved total cannot be pinned on one stage.  The ledger therefore knows only three things: which groups of the loop are IN
FLIGHT (opened and not yet committed, at most LIMIT = 3), when a group COMMITS, and what is DONE AGAIN when a total moved.

Two kinds of totals reach it, both sums of the three words of ops.split_overflow_snapshot:

  stage_end(gid, total)  a snapshot the loop recorded behind the CLIP stage of group gid, at a point of the device's work
                         that is the same in every run: the CLIP stages up to gid and the proposal stages up to gid + 1
                         have ended, nothing later has begun.  Unchanged: group gid commits.  Moved: every group in flight is
                         done again.
  read_back(total)       a snapshot that rode on the proposal-count read-back of the NEWEST group.  It proves the end of no
                         CLIP stage (the one beside it may be half way), so it commits nothing; and because it may or may
                         not have seen an overflow of that CLIP stage, a moved total must lead to the decision the next
                         stage_end would have led to: the groups in flight AND the loop's next group are done again
                         (Decision.pull_next: the caller opens that group first, without running it).  Judge every older
                         stage_end before a read_back.

Every decision is a function of the totals alone -- no clock, no event.query() -- so the same sequence of calls gives the
same decisions, and two runs of the same input commit the same groups in the same precision."""

LIMIT = 3


class Decision:
    """kind "commit": `groups` = the ids just committed (possibly none).  kind "rescue": `groups` = the ids in flight, oldest
    first -- roll back to the checkpoint of the first, clear the counters, re-run them in f32, then call rescued();
    pull_next: open() the loop's next group (when there is one) before doing so."""
    __slots__ = ("kind", "groups", "pull_next")

    def __init__(self, kind, groups, pull_next=False):
        self.kind, self.groups, self.pull_next = kind, list(groups), bool(pull_next)

    def __eq__(self, other):
        return isinstance(other, Decision) and (self.kind, self.groups, self.pull_next) == (other.kind, other.groups, other.pull_next)

    def __repr__(self):
        return f"Decision({self.kind!r}, {self.groups!r}, pull_next={self.pull_next})"


class RescueLedger:
    def __init__(self, base_total=0):
        self.base = int(base_total)     # the total at the last clean check
        self._open = []                 # [gid, payload, checkpoint] of the groups in flight, oldest first
        self.committed = []             # ids in the order they committed
        self.events = 0                 # moved totals met
        self.rescued_groups = []        # ids re-run in f32, in order

    # ---- what is in flight -----------------------------------------------------------------------------------------------
    def open(self, gid, payload=None):
        """group gid enters the loop (before its proposal stage).  payload: what a re-run needs (its loader units)."""
        if len(self._open) >= LIMIT:
            raise RuntimeError(f"rescue ledger: {LIMIT} groups are already in flight; judge the oldest stage_end first")
        if self._open and gid <= self._open[-1][0] or self.committed and gid <= self.committed[-1]:
            raise ValueError(f"rescue ledger: group {gid} opened out of order")
        self._open.append([gid, payload, None])

    def checkpoint(self, gid, cp):
        """cp: the pipeline's state before anything of group gid was logged (taken before its CLIP stage)"""
        for e in self._open:
            if e[0] == gid:
                e[2] = cp
                return
        raise KeyError(gid)

    def in_flight(self):
        return [e[0] for e in self._open]

    def payload(self, gid):
        return next(e[1] for e in self._open if e[0] == gid)

    def oldest_checkpoint(self):
        """the checkpoint to roll back to: that of the oldest group in flight that has one (a group without one has logged
        nothing yet, and neither has any group after it)"""
        for e in self._open:
            if e[2] is not None:
                return e[2]
        return None

    # ---- totals ----------------------------------------------------------------------------------------------------------
    def _moved(self, pull_next=False):
        self.events += 1
        return Decision("rescue", self.in_flight(), pull_next)

    def stage_end(self, gid, total):
        if not self._open or self._open[0][0] != gid:
            raise ValueError(f"rescue ledger: stage_end of group {gid}, the oldest in flight is "
                             f"{self._open[0][0] if self._open else None} (commits happen in order)")
        if int(total) != self.base:
            return self._moved()
        self.committed.append(self._open.pop(0)[0])
        return Decision("commit", [gid])

    def read_back(self, total):
        if int(total) == self.base:
            return Decision("commit", [])
        return self._moved(pull_next=True)

    def rescued(self, total_after=0):
        """the groups in flight have been re-run in f32 on an idle device and the counters cleared: they commit, the loop goes
        on with an empty pipeline"""
        ids = self.in_flight()
        self.committed += ids
        self.rescued_groups += ids
        self._open = []
        self.base = int(total_after)
        return ids
