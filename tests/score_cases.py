"""Cases, probes, float64 reference, margins, checker and a planted float32 implementation for the per-sentence scoring
(csrc/scoring.hip: score_lists_body + score_blend_body under score_sentence_kernel, grp_score_kernel and grp_sweep_score_kernel,
and calc_score_kernel), plain numpy, no GPU code.

The operation is Hybridgl_main.py:153-196,225-228: text ensemble r * sentence + (1 - r) * noun phrase, the mean of the other
nouns' features, two vectors of cosine logits, their soft-maxes over the proposals, the pure arg-max, the top-k1 / top-k2 lists,
per list-1 entry the relation sum over the boxes (utils.py:240-268), its soft-max, the blend with the coherence score and the
final arg-max.

`reference` is the yardstick: everything in float64 from the float32 inputs (r, alpha and logit_scale are the float32 values
the C ABI carries; 1 - r and 1 - alpha are exact differences of those).  The comparisons inside the relations are part of the
operation's definition and are exact here: a centre is x + w / 2 (compared as 2 x + w in integers), areas and the intersection
of "within" are integers.  The orders are torch's: a NaN is larger than every number, the first of equal maxima wins, top-k is
descending with the lowest index first among equals.  No other nouns: the mean is the zero vector, its norm 0, every negative
logit NaN.  A NaN logit makes the whole soft-max NaN; which proposals torch.topk then returns is not defined by the operation,
and the reference answers final = -1 (`check` then leaves idx[1] alone).

`check` -- the tolerance.  NaN positions of both logit vectors must be equal.  Elsewhere, with u = 2^-24,
    |got - ref| <= C u |logit_scale|,   C = 72.
|cos| <= 1 and, by Cauchy-Schwarz, the sum of the absolute values of the E products of two unit vectors is <= 1, so a rounding of
relative size u in a term, or in a partial sum of terms, moves the cosine by at most u times the absolute values below it.  C
counts the roundings of an implementation that sums the E terms DIRECTLY in float32: a chain per lane, E <= 1152 elements strided
over 64 lanes (at most 18 per lane, 17 adds), then six levels over the lanes.  Per logit, in units of u |logit_scale|:
    4   per term: x / |x|, * logit_scale, t / |t|, the product
   23   the sum: a term passes through at most 17 + 6 adds, each rounding at most u times the absolute sum below it
   26   the two norms, 13 each: the square (1) and the same 23 adds on positive terms, halved by the square root, + its own rounding
   13   the text vector: the ensemble is two products, one add and the rounding of 1 - r (3.5) relative to r |s_i| + (1 - r) |n_i|,
        not to |t_i|: times kappa = (r |s| + (1 - r) |n|) / |t| <= 2; the mean of n_other <= 5 rows is 4 adds and a division (5),
        times kappa = sum |o_k| / |sum o_k| <= 2.5 (both norm ratios; tests/test_score_cases_host.py asserts them for every case).
        A perturbation of t moves t / |t| by no more than its relative size.
   66 in all; the six left to 72 cover the second-order terms ((1 + u)^66) and fused or unfused multiply-adds.
C u |logit_scale| is 4.3e-4 at logit_scale = 100: well under the 1e-3 the existing GPU tests allow there (the project's own
ceiling).  C is a bound for the operation and is not fitted to the device code.
Indices: idx[0] and idx[1] must equal the reference's wherever `decided` says the reference alone decides them -- and the tables
below are built so that this is everywhere (asserted, not skipped, by tests/test_score_cases_host.py).

`margins` / `decided`.  With B = C u |logit_scale| (what a logit may move):
    pure        the gap of the two largest logits must exceed 2 B
    list        soft-max is monotone, so a list is decided by the logits: the gaps between ranks j and j + 1 for j < k (order and
                boundary; of list 2 only the boundary, and only when the relation sum runs over it) must exceed 2 B + 32 u
                (the 32 u: two soft-max values must differ by more than the float32 roundings of exp and the division)
    final       p_i = 1 / sum_j exp(l_j - l_i) moves by at most the factor exp(2 B), + 32 u for float32's own soft-max.  A relation
                term is a product of two such values with an exact 0 / 1 (or, for "within", three more roundings), all terms are
                >= 0, at most 16 are added: ts_i moves by at most rho ts_i, rho = 4 B + 96 u.  Its soft-max tf moves by at most
                2 rho max ts + 16 u, the blend v_i = (1 - alpha) tf_i + alpha gem_i by
                    tol = (1 - alpha) (2 rho max ts + 16 u) + 4 u (1 + |v_i|);
                the gap of the two largest v must exceed 2 tol.
A gap of exactly 0 is a tie.  Where it is exact by construction for ANY implementation (duplicated proposals, E = 1 where
every cosine is +-1, a probe whose blend is a one-hot gem), the case says so (has_ties) and the tie rule decides; anywhere else a
zero gap is undecided.  One tie needs no saying: alpha = 0 with every relation sum exactly 0 (each term has an exact 0 factor
in any implementation) -- all blends are 1 / k1 and list 1's first entry wins.

tests/test_score_cases_host.py checks this module on the CPU, tests/test_gpu_score_paths.py runs the device code.
"""
import os
import re
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORING_HIP = os.path.join(ROOT, "hybridgl_amd", "csrc", "scoring.hip")

C_BOUND = 72
U = 2.0 ** -24
RELAWORDS = ("none", "left", "right", "up", "down", "big", "small", "within")


# ------------------------------------------------------------------------------------------------------------- the constants
def constants(path=SCORING_HIP):
    """MAXK, UE, MQ as csrc/scoring.hip declares them, LANES (the stride of a lane over a feature row in score_lists_body) and
    THREADS (the stride of a thread over the proposals in its soft-max and arg-max loops)"""
    src = open(path).read()
    out = {}
    m = re.findall(r"^constexpr\s+int\s+MAXK\s*=\s*(\d+)\s*;", src, flags=re.M)
    if len(m) != 1:
        raise ValueError(f"{path}: {len(m)} declarations of MAXK")
    out["MAXK"] = int(m[0])
    body = src[src.index("void score_lists_body("):src.index("int score_blend_body(")]
    m = re.findall(r"constexpr\s+int\s+UE\s*=\s*(\d+)\s*,\s*MQ\s*=\s*(\d+)\s*;", body)
    if len(m) != 1:
        raise ValueError(f"{path}: {len(m)} declarations of UE, MQ in score_lists_body")
    out["UE"], out["MQ"] = int(m[0][0]), int(m[0][1])
    m = set(re.findall(r"for \(int i0 = lane; i0 < E; i0 \+= (\d+) \* UE\)", body))
    if len(m) != 1:
        raise ValueError(f"{path}: lane strides {sorted(m)} in score_lists_body")
    out["LANES"] = int(m.pop())
    m = set(re.findall(r"for \(int n = t; n < N; n \+= (\d+)\)", body))
    if len(m) != 1:
        raise ValueError(f"{path}: thread strides {sorted(m)} in score_lists_body")
    out["THREADS"] = int(m.pop())
    return out


CONST = constants()
MAXK, UE, MQ, LANES, THREADS = (CONST[k] for k in ("MAXK", "UE", "MQ", "LANES", "THREADS"))
TRIP = LANES * UE                   # elements of a feature row per trip of a wave
ROUND = (THREADS // LANES) * MQ     # masks per round of the workgroup


# ------------------------------------------------------------------------------------------------------------------- the cases
# kind: "random"; "tie" (dup: proposals dup[1:] are copies of dup[0], which holds the best row); "nan_gem" (the coherence score
# of list 1's second entry is NaN); "nan_row" (a NaN in one feature row: only idx[0] is defined); "probe1" / "probe2" / "rel"
# (below).  j: the probe's rank; dup: the tied proposals.
Case = namedtuple("Case", "name N E k1 k2 r alpha n_other rela has_other scale seed kind j dup")


def _c(name, N, E, k, r, alpha, n_other, rela, has_other, seed=0, scale=100.0, kind="random", j=0, dup=()):
    return Case(name, N, E, k[0], k[1], r, alpha, n_other, rela, has_other, scale, seed, kind, j, dup)


CASES = [
    # ---- the width of a feature row: 64 lanes, UE elements per lane and trip
    _c("E=1: every cosine is +-1", 5, 1, (3, 6), 0.5, 0.6, 1, "none", False, kind="tie"),
    _c("E=63: lanes-1", 17, 63, (3, 6), 0.5, 0.6, 1, "left", True),
    _c("E=64: lanes", 17, 64, (3, 6), 0.3, 0.6, 2, "right", False),
    _c("E=65: lanes+1", 17, 65, (3, 6), 0.5, 0.0, 1, "up", True),
    _c("E=80", 20, 80, (3, 6), 1.0, 0.6, 5, "down", True),
    _c("E=511: trip-1", 17, 511, (3, 6), 0.5, 0.6, 0, "big", False),
    _c("E=512: trip", 17, 512, (3, 6), 0.0, 0.6, 1, "small", True),
    _c("E=513: trip+1", 17, 513, (3, 6), 0.5, 1.0, 2, "within", False),
    _c("E=577: trip+lanes+1", 17, 577, (3, 6), 0.3, 0.6, 5, "within", True),
    _c("E=768: a half second trip", 33, 768, (3, 6), 0.5, 0.6, 1, "left", False),
    _c("E=1024: two trips", 17, 1024, (3, 6), 0.5, 0.6, 2, "big", True),
    _c("E=1100: a third, partial trip", 17, 1100, (3, 6), 0.3, 0.0, 1, "right", True),
    # ---- the number of proposals: 4 waves, MQ masks per wave, 256 threads
    _c("N=1", 1, 80, (3, 6), 0.5, 0.6, 1, "left", True),
    _c("N=2: k=17 clamps", 2, 65, (17, 17), 0.5, 0.6, 2, "big", False),
    _c("N=3: k=16 clamps", 3, 80, (16, 16), 0.0, 0.0, 1, "small", True),
    _c("N=4: waves", 4, 65, (16, 1), 0.5, 0.6, 0, "none", False),
    _c("N=5: waves+1", 5, 80, (2, 16), 1.0, 0.6, 5, "up", True),
    _c("N=15: round-1, k=17 clamps", 15, 65, (17, 17), 0.5, 0.6, 1, "down", False),
    _c("N=16: round", 16, 80, (16, 16), 0.3, 0.6, 2, "left", True),
    _c("N=17: round+1", 17, 80, (16, 16), 0.5, 0.6, 1, "within", True),
    _c("N=33: two rounds+1", 33, 65, (16, 1), 0.5, 0.0, 1, "right", True),
    _c("N=64", 64, 80, (2, 16), 0.5, 0.6, 2, "small", True),
    _c("N=255: threads-1", 255, 80, (1, 1), 0.5, 0.6, 1, "none", False),
    _c("N=256: threads", 256, 65, (3, 6), 1.0, 1.0, 0, "big", False),
    _c("N=257: threads+1", 257, 577, (16, 16), 0.5, 0.6, 5, "left", True),
    _c("N=300", 300, 65, (16, 16), 0.0, 0.6, 1, "up", False),
    # ---- exact ties by duplicated proposals (oracle.cases.tie_case): a wave's share of a round, the stride of the threads
    _c("tie N=17 (0,16): two rounds of one wave", 17, 80, (3, 6), 0.5, 0.6, 1, "none", False, kind="tie", dup=(0, 16)),
    _c("tie N=17 (15,16): last of a round, first of the next", 17, 65, (16, 16), 0.5, 0.6, 1, "left", True, kind="tie", dup=(15, 16)),
    _c("tie N=257 (0,64,256): one thread twice, a lane twice", 257, 80, (3, 6), 0.5, 0.6, 2, "big", False, kind="tie", dup=(0, 64, 256)),
    _c("tie N=257 (70,256): the later thread holds the lower index", 257, 65, (16, 16), 0.5, 0.6, 1, "small", True, kind="tie",
       dup=(70, 256)),
    # ---- NaN
    _c("NaN coherence score in list 1", 17, 80, (3, 6), 0.5, 0.6, 1, "none", False, kind="nan_gem"),
    _c("NaN in a feature row", 17, 80, (3, 6), 0.5, 0.6, 1, "none", False, kind="nan_row"),
]

# ---- probes: idx[1] is the only window onto the lists and the blend
#   probe1   alpha = 1 and gem one-hot on the proposal of rank j of the reference's positive order: the final index is that
#            proposal exactly when j < k1, else list 1's first entry (all blends are 0: a tie)
#   probe2   alpha = 0, has_other, "left", a small logit_scale; with W = list 1's second entry and q = the proposal of rank j of
#            the negative order, W and the proposals of negative rank < j have their centre at x = 12, q, list 1's first entry
#            and those of rank > j at 12.5: only W has a non-zero relation sum, and that exactly when q (or, then with it, a
#            proposal behind it) is in list 2.  The final index is W exactly when j < k2, else list 1's first entry.  This needs
#            the first two entries of list 1 at negative ranks >= k2: the seed is chosen for it.
#   rel      alpha = 0, small logit_scale, boxes designed so that the half pixel, the equal areas or the nesting decide
PROBE_BASES = [
    _c("probe1 N=33 k1=16", 33, 80, (16, 6), 0.5, 1.0, 1, "left", True, kind="probe1"),
    _c("probe1 N=5 k1=3", 5, 65, (3, 6), 0.5, 1.0, 1, "none", False, kind="probe1"),
    _c("probe1 N=3 k1=16 clamps", 3, 80, (16, 16), 0.5, 1.0, 1, "none", False, kind="probe1"),
    _c("probe2 N=33 k2=16", 33, 80, (3, 16), 0.5, 0.0, 1, "left", True, scale=10.0, kind="probe2"),
    _c("probe2 N=33 k2=6", 33, 65, (3, 6), 0.5, 0.0, 2, "left", True, scale=10.0, kind="probe2"),
    _c("probe2 N=257 k2=1", 257, 80, (2, 1), 0.5, 0.0, 1, "left", True, scale=10.0, kind="probe2"),
]


def _probes():
    out = []
    for b in PROBE_BASES:
        k = min(b.k1 if b.kind == "probe1" else b.k2, b.N)
        for j in range(min(k + 1, b.N)):
            out.append(b._replace(name=f"{b.name} j={j}", j=j))
    for w in RELAWORDS:
        for ho in (False, True):
            out.append(_c(f"rel {w}{' other' if ho else ''}", 6, 64, (4, 4), 0.5, 0.0, 1, w, ho, scale=5.0, kind="rel"))
    return out


PROBES = _probes()
ALL = CASES + PROBES


def case_id(c):
    return c.name.replace(" ", "_")


# seeds: the first of 0, 1, 2, ... at which the reference alone decides every index of the case (and, for probe2, at which the
# first two entries of list 1 lie at negative ranks >= k2); 0 where not listed.  tests/test_score_cases_host.py asserts the
# condition, not how the seed was found.
SEEDS = {"N=3: k=16 clamps": 2, "tie N=17 (0,16): two rounds of one wave": 1, "tie N=17 (15,16): last of a round, first of the next": 1,
         "tie N=257 (70,256): the later thread holds the lower index": 1, "probe2 N=33 k2=16": 2, "probe2 N=33 k2=6": 1}


def seed_of(c):
    key = c.name.split(" j=")[0]
    return SEEDS.get(key, c.seed)


Inputs = namedtuple("Inputs", "hybrid sent nphr others r boxes gem scale k1 k2 alpha rela has_other")


def _random_inputs(c):
    rng = np.random.default_rng([seed_of(c), c.N, c.E, 7])
    hybrid = rng.standard_normal((c.N, c.E)).astype(F32)
    sent = rng.standard_normal(c.E).astype(F32)
    nphr = rng.standard_normal(c.E).astype(F32)
    others = rng.standard_normal((c.n_other, c.E)).astype(F32) if c.n_other else None
    boxes = np.concatenate([rng.integers(0, 50, (c.N, 2)), rng.integers(1, 30, (c.N, 2))], axis=1).astype(np.int64)
    gem = (0.5 * rng.standard_normal(c.N)).astype(F32)
    return Inputs(hybrid, sent, nphr, others, F32(c.r), boxes, gem, F32(c.scale), c.k1, c.k2, F32(c.alpha), c.rela, c.has_other)


def _rel_boxes(word, order):
    """[N,4] for a rel probe: W = order[1] is the only proposal the relation holds for (against every other one); "within": W
    nested in order[0], order[2] touching W, the others disjoint"""
    N = len(order)
    b = np.zeros((N, 4), dtype=np.int64)
    W = order[1]
    for rank, n in enumerate(order):
        y, h = 3 + 2 * rank, 4 + (rank % 3)
        if word in ("left", "right"):      # centres 12 and 12.5: integer halves would make them equal
            b[n] = (12, y, 1, h) if (n == W) == (word == "right") else (11, y, 2, h)
        elif word in ("up", "down"):
            b[n] = (y, 12, h, 1) if (n == W) == (word == "down") else (y, 11, h, 2)
        elif word == "big":                # 25 against 24 = 6 x 4 = 8 x 3
            b[n] = (y, y, 5, 5) if n == W else ((y, 2, 6, 4) if rank % 2 else (y, 2, 8, 3))
        elif word == "small":              # 23 against 24
            b[n] = (y, y, 23, 1) if n == W else ((y, 2, 6, 4) if rank % 2 else (y, 2, 8, 3))
        elif word == "within":
            b[n] = [(0, 0, 20, 20), (2, 2, 4, 4), (6, 2, 4, 4), (30, 30, 3, 3)][rank] if rank < 4 else (40 + 10 * rank, 0, 5, 5)
        else:
            b[n] = (y, y, h, h)
    return b


def inputs(c):
    """the operands of case or probe c"""
    x = _random_inputs(c)
    if c.kind == "random" or (c.kind == "tie" and not c.dup):
        return x
    if c.kind == "tie":         # the best row to dup[0], then copies of it (feature row, box, coherence score) to dup[1:]
        best = reference(x).pure
        hybrid, boxes, gem = x.hybrid.copy(), x.boxes.copy(), x.gem.copy()
        for a in (hybrid, boxes, gem):
            a[[best, c.dup[0]]] = a[[c.dup[0], best]]
            a[list(c.dup[1:])] = a[c.dup[0]]
        return x._replace(hybrid=hybrid, boxes=boxes, gem=gem)
    if c.kind == "nan_row":
        hybrid = x.hybrid.copy()
        hybrid[5, 4] = np.nan
        return x._replace(hybrid=hybrid)
    ref = reference(x)
    if c.kind == "nan_gem":
        gem = x.gem.copy()
        gem[ref.order1[1]] = np.nan
        return x._replace(gem=gem)
    if c.kind == "probe1":
        gem = np.zeros(c.N, dtype=F32)
        gem[ref.order1[c.j]] = 1.0
        return x._replace(gem=gem)
    if c.kind == "probe2":
        T, W, q = ref.order1[0], ref.order1[1], ref.order2[c.j]
        rank2 = np.empty(c.N, dtype=np.int64)
        rank2[ref.order2] = np.arange(c.N)
        boxes = x.boxes.copy()
        for n in range(c.N):
            near = n == W or (rank2[n] < c.j and n != T)
            boxes[n, 0], boxes[n, 2] = (11, 2) if near else (12, 1)
        return x._replace(boxes=boxes)
    if c.kind == "rel":
        return x._replace(boxes=_rel_boxes(c.rela, ref.order1))
    raise ValueError(c.kind)


# --------------------------------------------------------------------------------------------------------------- the reference
def first_max(v):
    """torch.argmax's order: the first NaN, else the first of the maxima"""
    v = np.asarray(v, dtype=F64)
    n = np.isnan(v)
    return int(np.flatnonzero(n)[0]) if n.any() else int(np.argmax(v))


def _softmax64(l):
    with np.errstate(all="ignore"):
        if np.isnan(l).any():
            return np.full(l.shape, np.nan)
        e = np.exp(l - l.max())
        return e / e.sum()


def relation64(bi, bj, si, sj, rela):
    """utils.py:240-268 with exact comparisons"""
    xi, yi, wi, hi = (int(v) for v in bi)
    xj, yj, wj, hj = (int(v) for v in bj)
    if rela == "left":
        return si * sj * F64(2 * xi + wi < 2 * xj + wj)
    if rela == "right":
        return si * sj * F64(2 * xi + wi > 2 * xj + wj)
    if rela == "up":
        return si * sj * F64(2 * yi + hi < 2 * yj + hj)
    if rela == "down":
        return si * sj * F64(2 * yi + hi > 2 * yj + hj)
    if rela == "big":
        return si * sj * F64(wi * hi > wj * hj)
    if rela == "small":
        return si * sj * F64(wi * hi < wj * hj)
    if rela == "within":
        x1 = max(xi, xj)
        x2 = max(x1, min(xi + wi, xj + wj))
        y1 = max(yi, yj)
        y2 = max(y1, min(yi + hi, yj + hj))
        with np.errstate(all="ignore"):
            return si * sj * F64((x2 - x1) * (y2 - y1)) / F64(wi * hi)
    return si


Ref = namedtuple("Ref", "tpos tneg clip neg p pn order1 order2 k1 k2 top1 top2 ts v pure final alpha scale has_other")


def cosine_logits(img, txt, scale):
    """float64 [N,T]: calculate_score (model/backbone.py:74-87)"""
    img, txt = np.asarray(img, dtype=F64), np.asarray(txt, dtype=F64)
    with np.errstate(all="ignore"):
        a = img / np.sqrt((img * img).sum(1, keepdims=True))
        b = txt / np.sqrt((txt * txt).sum(1, keepdims=True))
        return F64(F32(scale)) * (a @ b.T)


def reference(x):
    """x: Inputs -> Ref, everything float64.  order1 / order2: all N proposals in list order (empty where the soft-max is NaN);
    top1 / top2 their first k1 / k2 (k clamped to N); ts, v: relation sums and blends of top1; final = -1 where not defined"""
    h = np.asarray(x.hybrid, dtype=F64)
    N = h.shape[0]
    r, alpha = F64(F32(x.r)), F64(F32(x.alpha))
    tpos = r * np.asarray(x.sent, dtype=F64) + (1.0 - r) * np.asarray(x.nphr, dtype=F64)
    n_other = 0 if x.others is None else len(x.others)
    tneg = np.asarray(x.others, dtype=F64).sum(0) / n_other if n_other else np.zeros_like(tpos)
    lg = cosine_logits(h, np.stack([tpos, tneg]), x.scale)
    clip, neg = lg[:, 0], lg[:, 1]
    pure = first_max(clip)
    p, pn = _softmax64(clip), _softmax64(neg)
    idx = np.arange(N)
    order1 = np.lexsort((idx, -p)) if not np.isnan(p).any() else np.zeros(0, dtype=np.int64)
    order2 = np.lexsort((idx, -pn)) if not np.isnan(pn).any() else np.zeros(0, dtype=np.int64)
    k1, k2 = min(int(x.k1), N), min(int(x.k2), N)
    top1, top2 = order1[:k1], order2[:k2]
    none = dict(ts=np.zeros(0), v=np.zeros(0), final=-1)
    if len(top1) == 0 or (x.has_other and len(top2) == 0):
        return Ref(tpos, tneg, clip, neg, p, pn, order1, order2, k1, k2, top1, top2, pure=pure, alpha=alpha, scale=F64(F32(x.scale)),
                   has_other=bool(x.has_other), **none)
    ts = np.zeros(k1)
    for a, i in enumerate(top1):
        over, sj = (top2, pn) if x.has_other else (top1, p)
        for j in over:
            ts[a] += relation64(x.boxes[i], x.boxes[j], p[i], sj[j], x.rela)
    with np.errstate(all="ignore"):
        mx = np.nanmax(ts) if not np.isnan(ts).all() else 0.0
        e = np.exp(ts - mx)
        tf = e / e.sum()
        v = tf * (1.0 - alpha) + alpha * np.asarray(x.gem, dtype=F64)[top1]
    return Ref(tpos, tneg, clip, neg, p, pn, order1, order2, k1, k2, top1, top2, ts, v, pure, int(top1[first_max(v)]), alpha,
               F64(F32(x.scale)), bool(x.has_other))


# ----------------------------------------------------------------------------------------------------------------- the margins
def logit_bound(scale):
    return C_BOUND * U * abs(float(scale))


def margins(ref):
    """name -> (gaps, what a gap must exceed): the decisions of the module's docstring"""
    B = logit_bound(ref.scale)
    N = len(ref.clip)
    out = {}
    if np.isnan(ref.clip).any() or N == 1:
        out["pure"] = (np.zeros(0), 2 * B)          # the first NaN: nothing to move
    else:
        s = np.sort(ref.clip)
        out["pure"] = (np.array([s[-1] - s[-2]]), 2 * B)
    if ref.final < 0:
        return out
    l1 = ref.clip[ref.order1]
    n1 = min(ref.k1, N - 1)                         # the pairs (0, 1) .. (k1 - 1, k1): order and, where k1 < N, the boundary
    out["list1"] = (l1[:n1] - l1[1:n1 + 1], 2 * B + 32 * U)
    if ref.has_other:
        l2 = ref.neg[ref.order2]
        out["list2"] = (l2[ref.k2 - 1:ref.k2] - l2[ref.k2:ref.k2 + 1] if ref.k2 < N else np.zeros(0), 2 * B + 32 * U)
    v = ref.v
    best = first_max(v)
    if np.isnan(v[best]) or len(v) == 1:
        out["final"] = (np.zeros(0), 0.0)           # a NaN blend wins: nothing to move
    elif ref.alpha == 0 and not ref.ts.any():
        out["final"] = (np.zeros(0), 0.0)           # every relation term has an exact 0 factor: all blends are 1 / k1, the first wins
    else:
        rho = 4 * B + 96 * U
        tol = (1.0 - ref.alpha) * (2 * rho * np.nanmax(np.abs(ref.ts)) + 16 * U) + 4 * U * (1 + abs(v[best]))
        out["final"] = (np.array([v[best] - np.delete(v, best).max()]), 2 * tol)
    return out


def decided(ref, ties=False):
    """{"pure": bool, "final": bool}: the reference alone decides the index.  ties: a gap of exactly 0 is an exact tie for
    every implementation (the case says so) and the tie rule decides it"""
    m = margins(ref)

    def ok(name):
        if name not in m:
            return True
        g, need = m[name]
        return bool(np.all((g > need) | ((g == 0) if ties else False)))
    return dict(pure=ok("pure"), final=ok("list1") and ok("list2") and ok("final"))


def has_ties(c):
    return c.kind in ("tie", "probe1", "probe2", "rel") or c.E == 1


# ----------------------------------------------------------------------------------------------------------------- the checker
def logit_ratios(got, want, scale):
    """|got - want| / (C u |logit_scale|) elementwise; 0 where both are NaN, inf where one is"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    with np.errstate(all="ignore"):
        r = np.abs(got - want) / logit_bound(scale)
    r = np.where(gn & wn, 0.0, r)
    return np.where(gn != wn, np.inf, r)


def check_indices(idx, ref, ties=False, what=""):
    """idx [2] equals the reference's pure and final index wherever the reference alone decides them"""
    d = decided(ref, ties)
    if d["pure"]:
        assert int(idx[0]) == ref.pure, f"{what}: pure index {int(idx[0])}, reference {ref.pure}"
    if d["final"] and ref.final >= 0:
        assert int(idx[1]) == ref.final, f"{what}: final index {int(idx[1])}, reference {ref.final} (list 1 {ref.top1.tolist()})"


def check(got, ref, ties=False, what=""):
    """got: (idx [2], score_clip [N], score_neg [N]).  Asserts the module's docstring; returns the worst ratio of a logit's
    error to the bound"""
    idx, clip, neg = got
    worst = 0.0
    for name, g, w in (("score_clip", clip, ref.clip), ("score_neg", neg, ref.neg)):
        r = logit_ratios(g, w, ref.scale)
        bad = np.flatnonzero(~(r <= 1.0))
        assert bad.size == 0, (f"{what}: {name} of proposals {bad.tolist()[:8]} misses the bound: ratio {r[bad].tolist()[:8]}, got "
                               f"{np.asarray(g, dtype=F64)[bad].tolist()[:8]}, reference {w[bad].tolist()[:8]}")
        worst = max(worst, float(r.max()))
    check_indices(idx, ref, ties, what)
    return worst


# --------------------------------------------------------------------------------------------- a float32 implementation, planted
# "mean_plus_one" (the other nouns' sum divided by n_other + 1) is listed apart: the mean is normalised before it is used, so
# the error cannot be seen in any output -- the host test shows it ACCEPTED on every case.
DEFECTS = ("tail_twice", "store_neighbour", "tie_high", "nan_low", "k2_for_list1", "list_short", "list_long", "used_not_skipped",
           "int_half", "alpha_swapped", "wrong_list")
INVISIBLE = ("mean_plus_one",)


def _rel32(bi, bj, si, sj, rela, int_half):
    f = F32
    half = (lambda v: f(int(v) // 2)) if int_half else (lambda v: f(v) / f(2))
    if rela == "left":
        return si * sj * f((f(bi[0]) + half(bi[2])) < (f(bj[0]) + half(bj[2])))
    if rela == "right":
        return si * sj * f((f(bi[0]) + half(bi[2])) > (f(bj[0]) + half(bj[2])))
    if rela == "up":
        return si * sj * f((f(bi[1]) + half(bi[3])) < (f(bj[1]) + half(bj[3])))
    if rela == "down":
        return si * sj * f((f(bi[1]) + half(bi[3])) > (f(bj[1]) + half(bj[3])))
    if rela == "big":
        return si * sj * f(int(bi[2]) * int(bi[3]) > int(bj[2]) * int(bj[3]))
    if rela == "small":
        return si * sj * f(int(bi[2]) * int(bi[3]) < int(bj[2]) * int(bj[3]))
    if rela == "within":
        x1 = max(int(bi[0]), int(bj[0]))
        x2 = max(x1, min(int(bi[0] + bi[2]), int(bj[0] + bj[2])))
        y1 = max(int(bi[1]), int(bj[1]))
        y2 = max(y1, min(int(bi[1] + bi[3]), int(bj[1] + bj[3])))
        with np.errstate(all="ignore"):
            return si * sj * f(x2 - x1) * f(y2 - y1) / f(int(bi[2]) * int(bi[3]))
    return si


def planted(x, defect=None):
    """(idx [2], score_clip, score_neg) of a direct float32 implementation -- and, per `defect`, one of the errors a scoring
    kernel can make"""
    f = F32
    with np.errstate(all="ignore"):
        hybrid = np.asarray(x.hybrid, dtype=f)
        N, E = hybrid.shape
        r, alpha, scale = f(x.r), f(x.alpha), f(x.scale)
        tpos = (r * x.sent + (f(1) - r) * x.nphr).astype(f)
        n_other = 0 if x.others is None else len(x.others)
        tneg = np.zeros(E, dtype=f)
        for o in (x.others if n_other else ()):
            tneg = (tneg + o).astype(f)
        if n_other:
            tneg = (tneg / f(n_other + (defect == "mean_plus_one"))).astype(f)

        def ext(a):      # a row as the batched loads see it without their guard: the clamped last element once more
            if defect == "tail_twice" and E % TRIP:
                return np.concatenate([a, a[..., -1:]], axis=-1)
            return a

        H = ext(hybrid)
        ni = np.sqrt((H * H).sum(1, dtype=f))

        def logits(t):
            t = ext(t)
            nt = np.sqrt((t * t).sum(dtype=f))
            return ((scale * (H / ni[:, None])) * (t / nt)).sum(1, dtype=f)

        clip, neg = logits(tpos), logits(tneg)
        if defect == "store_neighbour" and N >= 2 and N % ROUND:
            clip[N - 2], neg[N - 2] = clip[N - 1], neg[N - 1]

        def argmax(v, skip=()):
            best = -1
            for n in range(len(v)):
                if n in skip:
                    continue
                if best < 0:
                    best = n
                    continue
                a, b = v[n], v[best]
                an, bn = np.isnan(a), np.isnan(b)
                if an or bn:
                    if defect == "nan_low":
                        better = bn and not an
                    else:
                        better = an and not bn
                    if an and bn:
                        better = defect == "tie_high"
                else:
                    better = a > b or (a == b and defect == "tie_high")
                if better:
                    best = n
            return best

        def softmax(l):
            if np.isnan(l).any():
                return np.full(l.shape, np.nan, dtype=f)
            e = np.exp(l - l.max())
            return (e / e.sum(dtype=f)).astype(f)

        pure = argmax(clip)
        p, pn = softmax(clip), softmax(neg)

        def topk(v, k):
            k += (defect == "list_long") - (defect == "list_short")
            k = max(1, min(k, N))
            out = []
            for _ in range(k):
                out.append(argmax(v, () if defect == "used_not_skipped" else out))
            return out

        top1 = topk(p, x.k2 if defect == "k2_for_list1" else x.k1)
        top2 = topk(pn, x.k2)
        ts = np.zeros(len(top1), dtype=f)
        for a, i in enumerate(top1):
            other = bool(x.has_other) != (defect == "wrong_list")
            over, sj = (top2, pn) if other else (top1, p)
            for j in over:
                ts[a] = f(ts[a] + _rel32(x.boxes[i], x.boxes[j], p[i], sj[j], x.rela, defect == "int_half"))
        e = np.exp(ts - (np.nanmax(ts) if not np.isnan(ts).all() else f(0))).astype(f)
        tf = (e / e.sum(dtype=f)).astype(f)
        g = np.asarray(x.gem, dtype=f)[top1]
        if defect == "alpha_swapped":
            v = tf * alpha + (f(1) - alpha) * g
        else:
            v = tf * (f(1) - alpha) + alpha * g
        return np.array([pure, top1[argmax(v)]], dtype=np.int32), clip, neg


# ------------------------------------------------------------------------------------------------------------ refs for the fused entries
# (N, H, W, E, k1, k2, S, seed): whole refs for ops.score_ref / score_group / score_group_sweep; the coherence scores the device
# pooled (want_scores) are the reference's gem input
RefCase = namedtuple("RefCase", "name N H W E k1 k2 S seed")
REF_CASES = [
    RefCase("N=257 E=577 k=(16,16)", 257, 64, 64, 577, 16, 16, 2, 0),
    RefCase("N=3 k=16 clamps", 3, 40, 50, 80, 16, 16, 3, 0),
    RefCase("E=1100", 17, 64, 96, 1100, 3, 6, 3, 0),
]
REF_WORDS = (("left", "left", 1, True), ("big", "middle", 2, True), ("none", "none", 0, False))    # relaword, dirflag, n_other, has_other
BLACK = {"big": 1.95, "small": 1.5}
# the sweep: k1 in {1, 2, 16} x k2 in {1, 16} under ONE r (lists built once to (16, 16): the prefix property), and the ends of r / alpha
SWEEP = ([(0.5, a, k1, k2) for (k1, k2), a in zip(((1, 1), (1, 16), (2, 1), (2, 16), (16, 1), (16, 16)), (0.6, 0.0, 1.0, 0.6, 0.0, 1.0))]
         + [(0.0, 0.6, 3, 6), (1.0, 1.0, 2, 16), (0.0, 0.0, 16, 1), (1.0, 0.6, 1, 1)])
REF_SEEDS = {"E=1100": 1}


def ref_inputs(rc):
    """numpy operands of a ref: hybrid, text [4 S, E], boxes, masks, and per sentence a dict (rows of text, words, heat-map)"""
    from hybridgl_amd.synth import boxes_from_masks, synth_heatmap, synth_masks
    seed = REF_SEEDS.get(rc.name, rc.seed)
    rng = np.random.default_rng([seed, rc.N, rc.E, 11])
    masks = synth_masks(rc.N, rc.H, rc.W, 900 + rc.N)
    sents = []
    for s in range(rc.S):
        rela, dirflag, n_other, has_other = REF_WORDS[s % len(REF_WORDS)]
        sents.append(dict(sentence_row=4 * s, noun_phrase_row=4 * s + 1, other_row0=4 * s + 2, n_other=n_other, dirflag=dirflag,
                          relaword=rela, has_other_nouns=has_other, black=BLACK.get(rela, 1.8),
                          imgattn=synth_heatmap(rc.H, rc.W, 950 + 10 * rc.N + s)))
    return dict(hybrid=rng.standard_normal((rc.N, rc.E)).astype(F32), text=rng.standard_normal((4 * rc.S, rc.E)).astype(F32),
                boxes=boxes_from_masks(masks), masks=masks.astype(np.uint8), target=masks[rc.N // 2].astype(np.uint8), sentences=sents)


def ref_sentence_inputs(q, s, gem, scale, r, k1, k2, alpha):
    """Inputs of sentence s of the ref q (ref_inputs) under one configuration, with the coherence scores `gem`"""
    t = q["sentences"][s]
    others = q["text"][t["other_row0"]:t["other_row0"] + t["n_other"]] if t["n_other"] else None
    return Inputs(q["hybrid"], q["text"][t["sentence_row"]], q["text"][t["noun_phrase_row"]], others, F32(r), q["boxes"],
                  np.asarray(gem, dtype=F32), F32(scale), k1, k2, F32(alpha), t["relaword"], t["has_other_nouns"])
