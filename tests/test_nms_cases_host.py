"""CPU checks of the NMS test cases (tests/nms_cases.py) and of the reference they are judged by.

* `greedy_nms` (one float32 IoU row per kept candidate) against oracle/sam_oracle.py:nms (the K x K matrix) on every family at
  K <= 1100, and against a deliberately naive pure-Python loop over np.float32 scalars at K <= 200.
* the generator: clusters suppress at least 40 % of the valid candidates at every K of the device grid and nearly always hold
  rescued candidates, every chain keeps exactly the members its construction promises, every exact-threshold pair has a
  float32 IoU equal to the float32 threshold, every coordinate lies in [0, 2896].
"""
import time

import numpy as np
import pytest

import nms_cases as N
from oracle import sam_oracle as S

F32 = np.float32
HOST_K = [1, 2, 14, 63, 65, 70, 200, 449, 513, 1100]
GRID_K = N.K_BITS + N.K_SERIAL + N.K_LARGE


def oracle(c):
    sel = np.nonzero(c.keep)[0]
    return sel[S.nms(c.boxes[sel].astype(np.int64), c.scores[sel], c.thr)].tolist() if len(sel) else []


def before(sj, j, si, i):
    """the ranking as a predicate: NaN first, then descending score, the index on ties"""
    nj, ni = sj != sj, si != si
    if nj or ni:
        return nj and (not ni or j < i)
    return sj > si or (sj == si and j < i)


def naive_nms(c):
    """selection by repeated maximum, scalar np.float32 arithmetic, O(K^2): shares no code with greedy_nms"""
    todo = [i for i in range(len(c.keep)) if c.keep[i]]
    kept, dead = [], set()
    while todo:
        i = todo[0]
        for j in todo[1:]:
            if before(c.scores[j], j, c.scores[i], i):
                i = j
        todo.remove(i)
        if i in dead:
            continue
        kept.append(i)
        a = [F32(v) for v in c.boxes[i]]
        for j in todo:
            b = [F32(v) for v in c.boxes[j]]
            iw = max(min(a[2], b[2]) - max(a[0], b[0]), F32(0))
            ih = max(min(a[3], b[3]) - max(a[1], b[1]), F32(0))
            inter = iw * ih
            union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = inter / union
            assert type(iou) is F32
            if iou > F32(c.thr):
                dead.add(j)
    return kept


@pytest.mark.parametrize("K", HOST_K)
def test_reference_equals_the_oracle_and_the_naive_loop(K):
    names = set()
    for c in N.cases_for(K):
        got = N.run(c)
        assert got == oracle(c), (K, c.name)
        if K <= 200:
            assert got == naive_nms(c), (K, c.name)
        assert c.boxes.min(initial=0) >= 0 and c.boxes.max(initial=0) <= N.LIMIT
        assert (c.boxes[:, 2:] >= c.boxes[:, :2]).all()
        if c.must_keep is not None:
            assert set(c.must_keep) <= set(got) and not set(c.must_drop) & set(got), (K, c.name)
        names.add(c.name.split("@")[0].split("[")[0])
    if K >= 200:
        assert names >= {"clusters", "chain", "long_chain", "exact_threshold", "degenerate", "keep_none", "keep_valid65"} \
            | {f"ties_{p}" for p in N.TIE_PATTERNS}, names


def test_every_coordinate_of_the_device_grid_lies_in_the_exact_domain():
    assert 2 * N.LIMIT ** 2 < 2 ** 24
    for K in GRID_K:
        for thr in (None, 0.7):
            for c in N.cases_for(K, thr):
                assert c.boxes.shape == (K, 4) and c.boxes.min(initial=0) >= 0 and c.boxes.max(initial=0) <= N.LIMIT, (K, c.name)
                assert c.scores.shape == (K,) and c.scores.dtype == F32 and c.keep.shape == (K,) and c.keep.dtype == np.uint8


def test_clusters_suppress_two_in_five_and_hold_rescued_candidates():
    """the condition of the family, at every (K, seed, threshold) the device tests use; printed with -s"""
    for K in GRID_K:
        for thr in (0.5, 0.7):
            c = N.clusters(K, thr)
            t0 = time.perf_counter()
            kept = N.run(c)
            dt = time.perf_counter() - t0
            valid = int(c.keep.sum())
            frac = 1 - len(kept) / valid
            res = N.rescued(c, kept) if K <= 4097 else -1
            print(f"clusters K={K} thr={thr}: valid {valid}, suppressed {valid - len(kept)} ({frac:.0%}), rescued {res}, {dt:.2f} s")
            if K >= 64:
                assert frac >= 0.4, (K, thr, frac)
            if 128 <= K <= 4097:
                assert res >= 1, (K, thr)
            assert dt < 2.0, (K, thr, dt)           # (the largest reference call of the device tests)


@pytest.mark.parametrize("thr", [0.5, 0.7, 0.75])
def test_chains_keep_what_they_promise(thr):
    s, w = N.chain_geometry(thr)
    assert F32(w - s) / F32(w + s) > F32(thr) and not F32(w - 2 * s) / F32(w + 2 * s) > F32(thr)
    for K in (13, 66, 132, 201, 450, 512, 514, 1025):
        for ranks in N.chains_that_fit(K):
            if not ranks:
                continue
            c = N.chain(ranks, K, thr)
            kept = N.run(c)
            members = sum(len(p) for p in ranks)
            assert len(c.must_keep) + len(c.must_drop) == members
            assert sorted(set(range(K)) - set(kept)) == sorted(c.must_drop), (K, ranks)      # the fillers are all kept
            order = N.rank_order(c.scores, c.keep).tolist()
            assert [order.index(i) for i in kept] == sorted(order.index(i) for i in kept)    # kept order = rank order
            for p in ranks:                                                                  # the members sit at their ranks
                assert [order[r] in kept for r in p] == [i % 2 == 0 for i in range(len(p))]
            assert N.rescued(c, kept) == sum((len(p) - 1) // 2 for p in ranks) >= len(ranks)
    for K in (2, 3, 64, 65, 129, 513, 2801, 4097):
        c = N.long_chain(K, thr)
        kept = N.run(c)
        order = N.rank_order(c.scores, c.keep)
        assert kept == order[0::2].tolist() and sorted(kept) == sorted(c.must_keep)
        if K <= 513:
            assert N.rescued(c, kept) == (K - 1) // 2
    assert all(p[-1] < 16390 for p in N.RANKS_A + N.RANKS_B)
    assert N.chains_that_fit(16390) == [N.RANKS_A, N.RANKS_B]


def test_the_largest_chain_case_runs_through_the_reference():
    for ranks, thr in zip(N.chains_that_fit(16390), (0.7, 0.5)):
        c = N.chain(ranks, 16390, thr, dups=8)
        t0 = time.perf_counter()
        kept = set(N.run(c))
        assert time.perf_counter() - t0 < 2.0
        assert set(c.must_keep) <= kept and not set(c.must_drop) & kept
        assert len(kept) < 16390 // 4


@pytest.mark.parametrize("thr", sorted(N.EXACT))
def test_exact_threshold_pairs_are_exact_in_float32(thr):
    seam = 0
    for ra, rb, a, b, over in N.exact_pairs(thr):
        iou = N.iou_row(np.array(a, F32), np.array([b], F32))[0]
        assert iou.dtype == F32
        if over:
            assert iou > F32(thr)
        else:
            assert iou == F32(thr) and not iou > F32(thr)
        seam += ra < 64 <= rb
    assert seam >= 2
    c = N.exact_threshold(thr)
    kept = N.run(c)
    assert sorted(set(range(len(c.keep))) - set(kept)) == sorted(c.must_drop) and len(c.must_drop) == 4


def test_ties_and_keep_patterns_are_what_they_say():
    for K in (64, 129, 512, 1024):
        c = N.ties(K, "zero_one")
        assert set(np.unique(c.scores)) == {0.0, 1.0}
        c = N.ties(K, "signed_zero")
        assert np.signbit(c.scores[c.scores == 0]).any() and not np.signbit(c.scores[c.scores == 0]).all()
        c = N.ties(K, "nan_inf")
        assert np.isnan(c.scores).any() and np.isposinf(c.scores).any() and np.isneginf(c.scores).any()
        assert N.rank_order(c.scores, c.keep)[0] == np.nonzero(np.isnan(c.scores))[0][0]
        c = N.ties(K, "duplicates")
        assert len(c.must_drop) == 9 and c.must_keep[0] < min(c.must_drop) and len(N.run(c)) == K - 9
        if K >= 68:
            c = N.ties(K, "seam")
            sc = c.scores[N.rank_order(c.scores, c.keep)]
            assert sc[60] == sc[63] == sc[64] == sc[67] and sc[59] > sc[60] and (K == 68 or sc[67] > sc[68])
            if K >= 516:
                assert sc[508] == sc[511] == sc[512] == sc[515] and sc[507] > sc[508]
        kp = {c.name: c for c in N.keep_patterns(K)}
        assert not kp["keep_none"].keep.any() and N.run(kp["keep_none"]) == []
        assert N.run(kp["keep_last_only"]) == [K - 1] and N.run(kp["keep_first_only"]) == [0]
        bad = kp["keep_invalid_nan_high"]
        inv = bad.keep == 0
        assert np.isnan(bad.scores[inv]).any() and np.nanmin(bad.scores[inv]) > np.nanmax(bad.scores[~inv])
        assert not set(N.run(bad)) & set(np.nonzero(inv)[0].tolist())
        for v in N.VALID_COUNTS:
            assert (f"keep_valid{v}" in kp) == (v < K)
            if v < K:
                assert int(kp[f"keep_valid{v}"].keep.sum()) == v
    d = N.degenerate()
    kept = N.run(d)
    assert {3, 4, 5, 6, 7, 12} <= set(kept)                # empty boxes, identical ones included, are never suppressed
    assert (0 in kept) != (11 in kept) and (8 in kept) != (9 in kept)
