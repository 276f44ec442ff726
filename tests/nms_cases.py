"""Deterministic candidate lists for the greedy box NMS (csrc/sam_nms.hip: nms_segments_kernel with its LDS and serial bodies,
nms_rank / nms_mask / nms_scan_kernel) and the reference they are judged by, plain numpy, no GPU code.

`greedy_nms` is the reference: a loop over the ranked candidates that computes, for every kept one, ONE row of IoUs in float32,
operation by operation as torchvision's CPU kernel does -- inter / (area_a + area_b - inter), nothing fused -- and suppresses
where iou > np.float32(thr).  (torchvision compares the float IoU with the threshold as a double; that is the same decision
for every threshold whose float32 value is not above it: 0.5, 0.7 and 0.75 here.)  The ranking is descending score, NaN first,
the original index on ties.  It never builds a K x K matrix, so it also serves the lists of more than 16384 candidates.

Domain: every coordinate lies in [0, LIMIT = 2896].  Then every width, height, area and sum of two areas is an integer of at
most 2 * 2896^2 < 2^24 and exact in float32: whether the device code contracts `wa * ha + wb * hb` into a fused multiply-add
(the library is built with -ffp-contract=on) cannot change any value, let alone a decision, inside this domain.

Every family aims at ONE mechanism of the kernels and names its cases so that a failure names the mechanism:
clusters (long suppression chains: dead boxes that must not suppress), chain (a suppressor, a dead middle and a survivor at
chosen RANKS: the 64-row blocks and the removed[] words between them), exact_threshold (the strict `>`), ties (the index as
tie-break, signed zeros, infinities, NaNs), degenerate (zero areas, 0/0), keep_patterns (invalid candidates take no rank; the
word count follows the valid count).  tests/test_nms_cases_host.py checks generator and reference on the CPU,
tests/test_gpu_nms_paths.py runs the device code.
"""
from collections import namedtuple

import numpy as np

LIMIT = 2896
F32 = np.float32

# boxes int32 [K,4] XYXY, scores float32 [K], keep uint8 [K]; must_keep / must_drop: original indices whose fate the
# construction promises (None: the reference alone decides)
Case = namedtuple("Case", "name boxes scores keep thr must_keep must_drop")


def _case(name, boxes, scores, keep, thr, must_keep=None, must_drop=None):
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    assert boxes.min(initial=0) >= 0 and boxes.max(initial=0) <= LIMIT, name
    return Case(name, boxes, np.ascontiguousarray(scores, dtype=F32), np.ascontiguousarray(keep, dtype=np.uint8), float(thr),
                None if must_keep is None else tuple(int(i) for i in must_keep),
                None if must_drop is None else tuple(int(i) for i in must_drop))


# ------------------------------------------------------------------------------------------------------------ the reference
def rank_order(scores, keep):
    """original indices of the valid candidates in ranking order: descending score, NaN first, the index on ties (+0.0 and
    -0.0 are equal)"""
    sel = np.nonzero(np.asarray(keep))[0]
    sc = np.asarray(scores, dtype=np.float64)[sel]
    nan = np.isnan(sc)
    return sel[np.lexsort((sel, -np.where(nan, 0.0, sc), ~nan))]      # last key first; lexsort is stable


def iou_row(a, b):
    """float32 IoU of box a [4] with boxes b [n,4] (both float32), step by step: no fused operation, 0/0 -> NaN"""
    iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), F32(0))
    ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), F32(0))
    inter = iw * ih
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def greedy_nms(boxes_i32, scores_f32, keep_u8, thr):
    """-> the kept candidates as original indices, in kept (= ranking) order"""
    order = rank_order(scores_f32, keep_u8)
    b = np.asarray(boxes_i32).astype(F32)[order]
    t = F32(thr)
    rem = np.arange(len(order))               # ranks still alive, ascending
    kept = []
    while rem.size:
        r, rest = rem[0], rem[1:]
        kept.append(int(order[r]))
        iou = iou_row(b[r], b[rest])
        assert iou.dtype == F32
        rem = rest[~(iou > t)]
    return kept


def run(case):
    return greedy_nms(case.boxes, case.scores, case.keep, case.thr)


def rescued(case, kept):
    """how many kept candidates are overlapped by more than thr by a higher-ranked DEAD candidate: each one survives only
    because a dead box suppresses nothing (O(valid^2): for the host test's sizes)"""
    order = rank_order(case.scores, case.keep)
    b = case.boxes.astype(F32)[order]
    alive = np.isin(order, np.asarray(kept, dtype=np.int64))
    n = 0
    for r in np.nonzero(alive)[0]:
        if r and bool(((iou_row(b[r], b[:r]) > F32(case.thr)) & ~alive[:r]).any()):
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------------ geometry
PLACED_H = 420                      # rows 0 .. PLACED_H: the boxes a family places by hand; below: the filler grid
FILL, PITCH = 8, 11
FILL_COLS = (LIMIT - FILL) // PITCH + 1
FILL_ROWS = (LIMIT - PLACED_H - FILL) // PITCH + 1


def fillers(n, dups=1):
    """n boxes of 8 x 8 on a grid of pitch 11 below the placed rows: pairwise disjoint -- or, with dups > 1, in groups of
    `dups` identical boxes (the lists of more than 4097 candidates: heavy suppression keeps the reference fast)"""
    cell = np.arange(n) // dups
    assert n == 0 or cell[-1] < FILL_COLS * FILL_ROWS
    x0, y0 = (cell % FILL_COLS) * PITCH, PLACED_H + (cell // FILL_COLS) * PITCH
    return np.stack([x0, y0, x0 + FILL, y0 + FILL], 1).astype(np.int32)


def assemble(name, K, placed, thr, seed, dups=1, must_keep_ranks=(), must_drop_ranks=()):
    """placed {rank: box} among fillers, scores K - rank (distinct, descending with the rank), the ranks dealt to the
    original indices by a seeded permutation, every candidate valid"""
    by_rank = fillers(K, dups)
    for r, box in placed.items():
        assert 0 <= r < K and max(box[1], box[3]) < PLACED_H - FILL
        by_rank[r] = box
    index_of_rank = np.random.default_rng([K, seed, 77]).permutation(K)
    boxes = np.empty((K, 4), dtype=np.int32)
    scores = np.empty(K, dtype=F32)
    boxes[index_of_rank] = by_rank
    scores[index_of_rank] = K - np.arange(K)
    return _case(name, boxes, scores, np.ones(K, np.uint8), thr, index_of_rank[list(must_keep_ranks)],
                 index_of_rank[list(must_drop_ranks)])


def chain_geometry(thr):
    """(step s, width w) of sliding boxes: neighbours overlap by (w - s) / (w + s) > thr, boxes two apart by
    (w - 2s) / (w + 2s) <= thr, both in float32"""
    s, t = 1, F32(thr)
    for w in range(2, 200):
        if F32(w - s) / F32(w + s) > t and not F32(max(w - 2 * s, 0)) / F32(w + 2 * s) > t:
            return s, w
    raise ValueError(thr)


CHAIN_H, CHAIN_PITCH, CHAIN_ROW = 10, 14, 2800      # a chain's strip; chains longer than CHAIN_ROW (even) wrap into more strips


def chain_box(strip, i, thr):
    s, w = chain_geometry(thr)
    return [i * s, strip * CHAIN_PITCH, i * s + w, strip * CHAIN_PITCH + CHAIN_H]


# the rank tuples of the issue in two sets of disjoint ranks (a chain per tuple; members alternate kept / dead)
RANKS_A = [(10, 11, 12), (63, 64, 65), (0, 130, 131), (447, 448, 449), (509, 510, 511), (1022, 1023, 1024),
           (16383, 16384, 16385)]
RANKS_B = [(0, 64, 128), (511, 512, 513), (60, 70, 126, 129, 200)]


def chain(positions, K, thr, seed=0, dups=1, name=None):
    """one chain per rank tuple of `positions`: its members sit at those RANKS, each in a strip of its own; the even members
    are kept (the first suppresses the second, which is dead when the third's turn comes), the odd ones dropped"""
    placed, keep_r, drop_r = {}, [], []
    for c, ranks in enumerate(positions):
        assert list(ranks) == sorted(set(ranks)) and ranks[-1] < K and not set(ranks) & set(placed)
        for i, r in enumerate(ranks):
            placed[r] = chain_box(c, i, thr)
            (keep_r if i % 2 == 0 else drop_r).append(r)
    name = name or "chain[" + " ".join("-".join(map(str, p)) for p in positions) + f"]@{thr}"
    return assemble(name, K, placed, thr, seed, dups, keep_r, drop_r)


def chains_that_fit(K):
    return [[p for p in ranks if p[-1] < K] for ranks in (RANKS_A, RANKS_B)]


def long_chain(K, thr, seed=0):
    """ONE chain of K members and no filler: kept = the even ranks"""
    assert K <= CHAIN_ROW * (PLACED_H - FILL) // CHAIN_PITCH and CHAIN_ROW % 2 == 0
    placed = {r: chain_box(r // CHAIN_ROW, r % CHAIN_ROW, thr) for r in range(K)}
    return assemble(f"long_chain@{thr}", K, placed, thr, seed, 1, range(0, K, 2), range(1, K, 2))


# exact IoU = thr in float32: `nested` H x 10 against hb x 10 inside it (hb / H); `shifted` two w x 10 boxes d apart
# ((w - d) / (w + d)); 70 / 100 and 14 / 20 round to the float32 of 0.7
EXACT = {0.5: dict(H=10, hb=5, w=30, d=10), 0.75: dict(H=20, hb=15, w=70, d=10), 0.7: dict(H=10, hb=7, w=17, d=3)}
EXACT_MIN_K = 70


def exact_pairs(thr):
    """[(rank a, rank b, box a, box b, b is suppressed)]: pairs at exactly thr (kept: `>` is strict) and the same pairs with
    one more column of overlap (dropped); one of each across the 63 | 64 rank seam"""
    g = EXACT[thr]
    out = []
    for p, (ra, rb, kind, over) in enumerate([(0, 1, "nested", 0), (2, 3, "nested", 1), (4, 5, "shifted", 0), (6, 7, "shifted", 1),
                                              (63, 64, "nested", 0), (62, 65, "shifted", 1), (61, 66, "shifted", 0),
                                              (60, 67, "nested", 1)]):
        x = 200 * p
        if kind == "nested":
            a, b = [x, 0, x + 10, g["H"]], [x, 0, x + 10, g["hb"] + over]
        else:
            a, b = [x, 0, x + g["w"], 10], [x + g["d"] - over, 0, x + g["d"] - over + g["w"], 10]
        out.append((ra, rb, a, b, bool(over)))
    return out


def exact_threshold(thr, K=EXACT_MIN_K, seed=0):
    assert K >= EXACT_MIN_K
    pairs = exact_pairs(thr)
    placed = {r: box for ra, rb, a, b, _ in pairs for r, box in ((ra, a), (rb, b))}
    keep_r = [ra for ra, *_ in pairs] + [rb for _, rb, _, _, over in pairs if not over]
    return assemble(f"exact_threshold@{thr}", K, placed, thr, seed, 1, keep_r, [rb for _, rb, _, _, over in pairs if over])


def cluster_boxes(K, seed):
    """K // 6 seed boxes (sides 8 .. 300) in a 1000 x 1000 field; every candidate is a seed with each edge moved by up to
    +-12 % of the seed's width"""
    rng = np.random.default_rng([K, seed, 11])
    ns = max(K // 6, 1)
    wh = rng.integers(8, 301, size=(ns, 2))
    xy = (rng.random((ns, 2)) * (1000 - wh)).astype(np.int64)
    seeds = np.concatenate([xy, xy + wh], 1)
    pick = rng.integers(0, ns, size=K)
    jit = np.rint(rng.uniform(-0.12, 0.12, size=(K, 4)) * wh[pick, :1]).astype(np.int64)
    b = np.clip(seeds[pick] + jit, 0, LIMIT)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])           # (a flat seed's jitter may cross its edges: zero height at the least)
    return b.astype(np.int32)


def distinct_scores(K, rng):
    return ((rng.permutation(K) + 1) / F32(K + 1)).astype(F32)


# seeds at which clusters() meets its condition (>= 40 % of the valid candidates suppressed at K >= 64) for both thresholds;
# the host test asserts it for every K of the device grid
CLUSTER_SEED = {}


def clusters(K, thr, seed=None):
    seed = CLUSTER_SEED.get(K, 0) if seed is None else seed
    rng = np.random.default_rng([K, seed, 12])
    keep = rng.random(K) > 0.1
    keep[0] = True
    return _case(f"clusters@{thr}", cluster_boxes(K, seed), distinct_scores(K, rng), keep, thr)


TIE_PATTERNS = ("all_equal", "zero_one", "seam", "signed_zero", "inf", "nan_inf", "duplicates")


def ties(K, pattern, thr=0.7, seed=0):
    """equal scores: the original index decides.  None where the pattern needs more candidates."""
    rng = np.random.default_rng([K, seed, 13, TIE_PATTERNS.index(pattern)])
    boxes = cluster_boxes(K, seed + 1)
    keep = np.ones(K, np.uint8)
    name = f"ties_{pattern}"
    if pattern == "all_equal":
        return _case(name, boxes, np.ones(K, F32), keep, thr)
    if pattern == "zero_one":                           # the second NMS: 1 for a mask the clean-up left unchanged
        return _case(name, boxes, (rng.random(K) < 0.7).astype(F32), keep, thr)
    if pattern == "seam":                               # equal scores on either side of ranks 63 | 64 and 511 | 512
        if K < 68:
            return None
        sc = distinct_scores(K, rng)
        order = rank_order(sc, keep)
        for lo, hi in ((60, 68), (508, 516)):
            if hi <= K:
                sc[order[lo:hi]] = sc[order[hi - 1]]
        return _case(name, boxes, sc, keep, thr)
    if pattern == "signed_zero":                        # +0.0 == -0.0: neither ranks before the other but by index
        return _case(name, boxes, rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], F32), size=K), keep, thr)
    if pattern in ("inf", "nan_inf"):
        sc = distinct_scores(K, rng)
        u = rng.random(K)
        sc[u < 0.2] = np.inf
        sc[(u >= 0.2) & (u < 0.4)] = -np.inf
        if pattern == "nan_inf":
            sc[(u >= 0.4) & (u < 0.6)] = np.nan
        return _case(name, boxes, sc, keep, thr)
    if pattern == "duplicates":                         # ten copies of one box at equal scores: the lowest index survives
        if K < 10:
            return None
        b = fillers(K)
        dup = np.sort(rng.choice(K, size=10, replace=False))
        b[dup] = [500, 100, 560, 160]
        return _case(name, b, np.full(K, 0.5, F32), keep, thr, dup[:1], dup[1:])
    raise ValueError(pattern)


DEGENERATE = [[0, 0, 2000, 2000],                                   # contains all the others
              [5, 5, 5, 40], [5, 5, 40, 5],                         # zero width, zero height
              [7, 7, 7, 7], [7, 7, 7, 7],                           # identical and empty: 0 / 0, neither is suppressed
              [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0],             # the box of an empty mask
              [10, 10, 60, 60], [12, 12, 62, 62],                   # IoU 0.85
              [100, 100, 150, 180], [0, 0, 1990, 1995],             # (the last: 0.99 with the container)
              [300, 300, 300, 300], [20, 20, 20, 50]]


def degenerate(K=len(DEGENERATE), thr=0.7, seed=0):
    """the list above, repeated cyclically up to K (so the real boxes also meet exact duplicates of themselves)"""
    assert K >= len(DEGENERATE)
    rng = np.random.default_rng([K, seed, 14])
    boxes = np.array(DEGENERATE, np.int32)[np.arange(K) % len(DEGENERATE)]
    return _case("degenerate", boxes, distinct_scores(K, rng), np.ones(K, np.uint8), thr)


VALID_COUNTS = (64, 65, 512, 513)


def keep_patterns(K, thr=0.7, seed=0):
    rng = np.random.default_rng([K, seed, 15])
    boxes = cluster_boxes(K, seed + 2)
    sc = distinct_scores(K, rng)
    one = lambda i: np.eye(1, K, i, dtype=np.uint8)[0]
    out = [_case("keep_none", boxes, sc, np.zeros(K, np.uint8), thr), _case("keep_last_only", boxes, sc, one(K - 1), thr),
           _case("keep_first_only", boxes, sc, one(0), thr)]
    keep = rng.random(K) < 0.6
    bad = sc.copy()                                     # invalid candidates with NaN or the highest scores take no rank
    inv = np.nonzero(~keep)[0]
    bad[inv[::2]] = np.nan
    bad[inv[1::2]] = 10 + inv[1::2]
    out.append(_case("keep_invalid_nan_high", boxes, bad, keep, thr))
    for v in VALID_COUNTS:
        if v < K:                                       # the word count follows the valid count, not K
            k = np.zeros(K, np.uint8)
            k[rng.choice(K, size=v, replace=False)] = 1
            out.append(_case(f"keep_valid{v}", boxes, bad, k, thr))
    return out


BIG = 4097          # above: only heavy-suppression lists (the reference's loop runs once per KEPT candidate)


def cases_for(K, thr=None):
    """every family that fits K candidates -> [Case]; thr: one threshold for all (the segmented launch takes one per call)"""
    big = K > BIG
    out = [clusters(K, t) for t in ((0.5, 0.7) if thr is None else (thr,))]
    for ranks, t in zip(chains_that_fit(K), (0.7, 0.5)):
        if ranks:
            out.append(chain(ranks, K, thr or t, dups=8 if big else 1))
    if K >= 2 and not big:
        out.append(long_chain(K, thr or 0.7))
    if K >= EXACT_MIN_K and not big:
        out += [exact_threshold(t, K) for t in (sorted(EXACT) if thr is None else (thr,))]
    for p in ("zero_one", "nan_inf") if big else TIE_PATTERNS:
        c = ties(K, p, thr or (0.5 if big else 0.7))
        if c is not None:
            out.append(c)
    if K >= len(DEGENERATE) and not big:
        out.append(degenerate(K, thr or 0.7))
    return out + keep_patterns(K, thr or 0.7)


# the K of the device grid, by the route that serves them
K_BITS = [1, 2, 63, 64, 65, 127, 128, 129, 448, 449, 511, 512]      # hgl_nms: nms_segments_kernel<true>, the LDS body
K_SERIAL = [513, 1023, 1024]                                        # hgl_nms: nms_segments_kernel<false>, the serial body
K_LARGE = [1025, 4097, 16390]                                       # hgl_nms_large alone; the last: W = 257 words a row
