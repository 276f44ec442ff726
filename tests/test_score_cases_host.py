"""CPU: tests/score_cases.py itself -- the constants it reads from csrc/scoring.hip, the edges its cases sit on, that its
reference alone decides every index of every case, probe and ref (the condition the GPU test rests on: asserted, never skipped),
its reference against the reference program's own outputs (tests/golden/scoring*.npz) and the numpy oracle, and its checker
against planted errors (each rejected on at least one case, the same implementation without the error accepted on all).
Run with -s for which cases catch which error."""
import os
import warnings

import numpy as np
import pytest

import score_cases as SC
from oracle import clip_oracle as O

IDS = [SC.case_id(c) for c in SC.ALL]


@pytest.fixture(scope="module")
def world():
    """per case and probe: (case, operands, reference)"""
    out = []
    for c in SC.ALL:
        x = SC.inputs(c)
        out.append((c, x, SC.reference(x)))
    return out


def test_constants_parse_from_scoring_hip():
    k = SC.constants()
    assert set(k) == {"MAXK", "UE", "MQ", "LANES", "THREADS"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    assert k["LANES"] == 64 and k["THREADS"] == 256 and k["THREADS"] % k["LANES"] == 0
    assert SC.TRIP == k["LANES"] * k["UE"] and SC.ROUND == k["THREADS"] // k["LANES"] * k["MQ"]
    assert max(max(c.k1, c.k2) for c in SC.ALL) == k["MAXK"] + 1      # (17, 17) appears, and only where N clamps it:
    assert all(min(c.k1, c.N) <= k["MAXK"] and min(c.k2, c.N) <= k["MAXK"] for c in SC.ALL)


def test_cases_sit_on_the_edges_their_names_claim():
    L, T, R, W = SC.LANES, SC.TRIP, SC.ROUND, SC.THREADS // SC.LANES
    rand = [c for c in SC.CASES]
    E = {c.E for c in rand}
    assert {1, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T} <= E
    assert any(T < e < 2 * T and e % L == 1 for e in E)             # a second trip whose first batch alone is live, one lane of it
    assert any(T < e < 2 * T and e % L == 0 for e in E)             # a second trip with whole batches only
    assert any(e > 2 * T and e % L for e in E)                      # a third trip, partial
    assert any(e < L for e in E if e > 1) and any(L < e < T and e % L for e in E)
    assert max(E) <= 18 * L                                         # the chain length the bound's count assumes
    N = {c.N for c in rand}
    assert {1, 2, 3} <= N and all(n < W for n in (1, 2, 3))         # waves without a mask
    assert {W, W + 1, R - 1, R, R + 1, 2 * R + 1, SC.THREADS - 1, SC.THREADS, SC.THREADS + 1} <= N
    assert any(n > SC.THREADS + 1 for n in N) and L in N
    for c in SC.ALL:
        for word, v in (("N", c.N), ("E", c.E)):
            if f"{word}=" in c.name:
                assert f"{word}={v}" in c.name.replace(":", " ").split(), c.name
    named = {c.name.split(":")[0]: c for c in rand}
    assert named[f"E={T - 1}"].name.endswith("trip-1") and named[f"E={T + 1}"].name.endswith("trip+1")
    assert named[f"E={T + L + 1}"].name.endswith("trip+lanes+1") and named[f"E={L + 1}"].name.endswith("lanes+1")
    assert named[f"N={R - 1}"].name.startswith(f"N={R - 1}: round-1") and named[f"N={R + 1}"].name.endswith("round+1")
    assert named[f"N={SC.THREADS + 1}"].name.endswith("threads+1")
    ks = {(c.k1, c.k2) for c in rand}
    assert ks >= {(1, 1), (3, 6), (16, 16), (16, 1), (2, 16), (17, 17)}
    assert all(c.N < 17 for c in rand if (c.k1, c.k2) == (17, 17))
    assert any(c.N > 16 and c.k1 == 16 for c in rand) and any(c.N < 16 and c.k1 == 16 for c in rand)      # boundary at 16; clamp
    assert {float(np.float32(c.r)) for c in rand} == {float(np.float32(v)) for v in (0, 1, 0.5, 0.3)}
    assert {c.alpha for c in rand} == {0.0, 1.0, 0.6} and {c.n_other for c in rand} == {0, 1, 2, 5}
    assert {(c.rela, c.has_other) for c in SC.ALL} >= {(w, h) for w in SC.RELAWORDS for h in (False, True)}
    assert all(not c.has_other for c in SC.ALL if c.n_other == 0)   # a relation sum over an all-NaN list is not defined
    # the ties: at N = round + 1 and N = threads + 1; a wave's two rounds, the seam of two rounds, one thread's two proposals,
    # one lane's two proposals of the top-k scan, a later thread holding the lower index
    dups = {(c.N, c.dup) for c in rand if c.dup}
    assert {n for n, _ in dups} == {R + 1, SC.THREADS + 1}
    assert any(d[1] - d[0] == R for n, d in dups if n == R + 1) and any(d == (R - 1, R) for n, d in dups if n == R + 1)
    assert any(d[0] + SC.THREADS in d and (d[1] - d[0]) % L == 0 and d[1] < SC.THREADS for n, d in dups if n == SC.THREADS + 1)
    assert any(d[-1] >= SC.THREADS and d[0] % SC.THREADS > d[-1] % SC.THREADS for n, d in dups if n == SC.THREADS + 1)


def test_boxes_hold_what_the_relations_can_get_wrong(world):
    half = equal_area = nested = disjoint = touching = 0
    for c, x, ref in world:
        b = x.boxes
        cx2 = 2 * b[:, 0] + b[:, 2]
        half += int(np.any(np.abs(cx2[:, None] - cx2[None, :]) == 1))           # centres half a pixel apart
        a = b[:, 2] * b[:, 3]
        equal_area += int(len(set(a.tolist())) < len(a) and c.kind == "rel" and c.rela in ("big", "small"))
        if c.kind == "rel" and c.rela == "within":
            o = ref.order1
            B = lambda k: b[o[k]]
            nested += int(B(1)[0] >= B(0)[0] and B(1)[0] + B(1)[2] <= B(0)[0] + B(0)[2])
            touching += int(B(1)[0] + B(1)[2] == B(2)[0])
            disjoint += int(B(3)[0] > B(0)[0] + B(0)[2])
    assert half and equal_area and nested and disjoint and touching
    assert any((x.boxes[:, 2] % 2 == 1).any() and (x.boxes[:, 3] % 2 == 1).any() for _, x, _ in world)


@pytest.mark.parametrize("k", range(len(SC.ALL)), ids=IDS)
def test_the_reference_alone_decides_every_index(world, k):
    """the condition of the GPU test: no case, no probe is undecided; a zero gap occurs only where the case declares exact ties"""
    c, x, ref = world[k]
    d = SC.decided(ref, SC.has_ties(c))
    m = {n: (g.tolist(), need) for n, (g, need) in SC.margins(ref).items()}
    assert d["pure"] and d["final"], (c.name, m)
    if not SC.has_ties(c):
        assert SC.decided(ref, False) == d
    if c.kind != "nan_row":
        assert ref.final >= 0 and ref.final in ref.top1
        assert len(ref.top1) == min(c.k1, c.N) and len(ref.top2) == (min(c.k2, c.N) if c.n_other else 0)
    else:
        assert ref.final == -1 and ref.pure == 5 and np.isnan(ref.clip[5])
    # the conditioning the bound's count assumes for the two text vectors
    s, n, r = x.sent.astype(np.float64), x.nphr.astype(np.float64), float(x.r)
    assert (r * np.linalg.norm(s) + (1 - r) * np.linalg.norm(n)) / np.linalg.norm(ref.tpos) <= 2.0
    if x.others is not None:
        o = x.others.astype(np.float64)
        assert np.linalg.norm(o, axis=1).sum() / np.linalg.norm(o.sum(0)) <= 2.5
    assert np.isnan(ref.neg).all() == (c.n_other == 0) or c.kind == "nan_row"


def test_probes_say_what_they_are_built_to_say(world):
    seen = set()
    for c, x, ref in world:
        base = SC.reference(SC._random_inputs(c))
        if c.kind == "probe1":      # the proposal of rank j wins exactly when it is in list 1
            k1 = min(c.k1, c.N)
            assert ref.final == (base.order1[c.j] if c.j < k1 else base.order1[0]), c.name
            assert x.alpha == 1 and x.gem.sum() == 1 and x.gem[base.order1[c.j]] == 1
            seen.add(("probe1", c.j < k1))
        elif c.kind == "probe2":    # list 1's second entry wins exactly when the proposal of negative rank j is in list 2
            k2 = min(c.k2, c.N)
            rank2 = np.empty(c.N, dtype=np.int64)
            rank2[base.order2] = np.arange(c.N)
            assert rank2[base.order1[0]] >= k2 and rank2[base.order1[1]] > k2, c.name
            assert ref.final == (base.order1[1] if c.j < k2 else base.order1[0]), c.name
            assert np.array_equal(ref.order1, base.order1) and np.array_equal(ref.order2, base.order2)
            assert (np.count_nonzero(ref.ts) == 1 and ref.ts[1] > 0) if c.j < k2 else not ref.ts.any()
            assert x.alpha == 0 and x.scale <= 10
            seen.add(("probe2", c.j < k2))
        elif c.kind == "rel":
            plain = SC.reference(x._replace(rela="none"))
            assert plain.final == ref.order1[0]
            if c.rela != "none":    # the relation, not the soft-max alone, decides
                assert ref.final == ref.order1[1] != plain.final, c.name
                g, need = SC.margins(ref)["final"]
                assert g[0] > 50 * need, (c.name, g, need)      # a wide margin
            seen.add(("rel", c.rela, c.has_other))
    assert {("probe1", True), ("probe1", False), ("probe2", True), ("probe2", False)} <= seen
    assert len([s for s in seen if s[0] == "rel"]) == 2 * len(SC.RELAWORDS)


# ---- the reference against the reference program's own outputs --------------------------------------------------------------
def golden_inputs(case, gem, scale, rela, has_other):
    hybrid, t_pos, t_neg, masks, boxes, attn, gt = case
    return SC.Inputs(hybrid, t_pos[0], t_pos[0], t_neg, np.float32(0.5), boxes, gem, np.float32(scale), 3, 6, np.float32(0.6), rela,
                     has_other)


def test_reference_reproduces_the_goldens(golden_dir):
    from oracle.cases import NAN_PLAN, TAIL_CASES, TIE_PLAN, nan_case, tail_case, tie_case
    g = np.load(os.path.join(golden_dir, "scoring.npz"))
    ls = float(g["cs_logit_scale"])
    H, W, N = (int(v) for v in g["tail_hw"])
    for ci, (rela, dirflag, has_other) in enumerate(TAIL_CASES):
        ref = SC.reference(golden_inputs(tail_case(ci, N, 32, H, W), g[f"tail{ci}_gem"], ls, rela, has_other))
        assert [ref.pure, ref.final] == [int(v) for v in g[f"tail{ci}_idx"]], ci
        assert SC.logit_ratios(g[f"tail{ci}_sc"], ref.clip, ls).max() <= 1 and SC.logit_ratios(g[f"tail{ci}_sn"], ref.neg, ls).max() <= 1
    black = lambda rela: 1.95 if rela == "big" else (1.5 if rela == "small" else 1.8)
    t = np.load(os.path.join(golden_dir, "scoring_ties.npz"))
    for step, (ci, dup, rela, dirflag, has_other) in enumerate(TIE_PLAN):
        case = tie_case(ci, dup)
        gem = O.coherence_scores(case[5], case[3], dirflag, black(rela))
        ref = SC.reference(golden_inputs(case, gem, ls, rela, has_other))
        assert [ref.pure, ref.final] == [int(v) for v in t[f"t{step}_idx"]], step
    n = np.load(os.path.join(golden_dir, "scoring_nan.npz"))
    for step, (kind, rela, dirflag, has_other) in enumerate(NAN_PLAN):
        case = nan_case(kind)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gem = O.coherence_scores(case[5], case[3], dirflag, black(rela))
            ref = SC.reference(golden_inputs(case, gem, ls, rela, has_other))
        assert ref.pure == int(n[f"n{step}_idx"][0]), (step, kind)
        if kind.startswith("nan_row"):      # NaN features: only the pure-CLIP index is defined (oracle/cases.py)
            assert ref.final == -1
        else:
            assert ref.final == int(n[f"n{step}_idx"][1]), (step, kind)
    # calculate_score's own golden
    assert SC.logit_ratios(g["cs_out"], SC.cosine_logits(g["cs_img"], g["cs_txt"], ls), ls).max() <= 1


def oracle_answer(x):
    """oracle.clip_oracle.score_sentence behind the text glue of Hybridgl_main.py:146-165 in float32"""
    f = np.float32
    ens = (f(x.r) * x.sent + f(1 - f(x.r)) * x.nphr).astype(f)
    other = np.zeros_like(ens)
    for o in (x.others if x.others is not None else ()):
        other = other + o
    if x.others is not None:
        other = (other / f(len(x.others))).astype(f)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        ip, ifin, sc, sn = O.score_sentence(x.hybrid, ens, other, x.boxes, x.gem, float(x.scale), x.k1, x.k2, float(x.alpha), x.rela,
                                            x.has_other)
    return np.array([ip, ifin]), sc, sn


@pytest.mark.parametrize("k", range(len(SC.ALL)), ids=IDS)
def test_reference_agrees_with_the_numpy_oracle(world, k):
    """(numpy's matrix product does not sum every row in the same order -- the rows of a remainder block go another way -- so
    the oracle's logits of two COPIES of a proposal can differ in the last bit and its arg-max can name either copy: with
    duplicated proposals the oracle's indices are compared up to the copies.  The device code treats every row alike and is
    held to the lowest index.)"""
    c, x, ref = world[k]
    idx, sc, sn = oracle_answer(x)
    if c.dup:
        idx = np.array([c.dup[0] if int(v) in c.dup else int(v) for v in idx])
        assert ref.pure == c.dup[0]
    SC.check((idx, sc, sn), ref, SC.has_ties(c), c.name)


# ---- the checker against planted errors -------------------------------------------------------------------------------------
def test_check_accepts_a_direct_float32_implementation_and_rejects_each_planted_error(world):
    caught = {d: [] for d in SC.DEFECTS}
    worst = 0.0
    for c, x, ref in world:
        worst = max(worst, SC.check(SC.planted(x), ref, SC.has_ties(c), c.name))
        for d in SC.INVISIBLE:
            SC.check(SC.planted(x, d), ref, SC.has_ties(c), f"{c.name} {d}")
        for d in SC.DEFECTS:
            try:
                SC.check(SC.planted(x, d), ref, SC.has_ties(c), c.name)
            except AssertionError:
                caught[d].append(c.name)
    print(f"direct float32 / bound, worst: {worst:.3f} (C = {SC.C_BOUND})")
    for d, names in caught.items():
        print(f"{d:18s} caught by {len(names):3d}: {'; '.join(names[:6])}{' ...' if len(names) > 6 else ''}")
    assert all(caught.values()), {d: len(v) for d, v in caught.items()}
    assert 0 < worst <= 1
    # where each one must show: the probes and edges built for it
    assert any(n.startswith("probe1") for n in caught["list_short"]) and any(n.startswith("probe1") for n in caught["list_long"])
    assert any(n.startswith("probe2") for n in caught["list_short"]) and any(n.startswith("probe2") for n in caught["list_long"])
    assert any(n.startswith("probe1") for n in caught["k2_for_list1"]) and any(n.startswith("probe2") for n in caught["wrong_list"])
    assert any(n.startswith("rel") for n in caught["int_half"]) and any(n.startswith("tie") for n in caught["tie_high"])
    assert any(n.startswith("NaN") for n in caught["nan_low"])
    assert {n.split(":")[0] for n in caught["tail_twice"]} >= {f"E={SC.TRIP - 1}", f"E={SC.TRIP + 1}", f"E={SC.LANES - 1}"}
    assert not any(n.startswith((f"E={SC.TRIP}:", f"E={2 * SC.TRIP}:")) for n in caught["tail_twice"])
    assert {n.split(":")[0] for n in caught["store_neighbour"]} >= {f"N={SC.ROUND + 1}", f"N={SC.ROUND - 1}"}


def test_check_rejects_a_nan_out_of_place_and_a_missing_one(world):
    by = {c.name: (c, x, ref) for c, x, ref in world}
    c, x, ref = by["E=80"]
    good = (np.array([ref.pure, ref.final]), ref.clip.astype(np.float32), ref.neg.astype(np.float32))
    assert SC.check(good, ref) <= 1
    for which in (1, 2):
        bad = [a.copy() for a in good]
        bad[which][3] = np.nan
        with pytest.raises(AssertionError):
            SC.check(tuple(bad), ref)
    for at in (0, 1):
        bad = [a.copy() for a in good]
        bad[0][at] = (bad[0][at] + 1) % c.N
        with pytest.raises(AssertionError):
            SC.check(tuple(bad), ref)
    c, x, ref = by["N=4: waves"]           # no other nouns: every negative logit is NaN
    good = (np.array([ref.pure, ref.final]), ref.clip.astype(np.float32), ref.neg.astype(np.float32))
    assert np.isnan(good[2]).all() and SC.check(good, ref) <= 1
    bad = [a.copy() for a in good]
    bad[2][1] = 0.0
    with pytest.raises(AssertionError):
        SC.check(tuple(bad), ref)
    bad = [a.copy() for a in good]
    bad[1][0] += np.float32(2.5 * SC.logit_bound(ref.scale))
    with pytest.raises(AssertionError):
        SC.check(tuple(bad), ref)


# ---- the refs of the fused entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SC.REF_CASES)), ids=[SC.case_id(rc) for rc in SC.REF_CASES])
def test_refs_are_decided_under_every_configuration(k):
    """with the oracle's coherence scores in place of the device's (they differ in the last bits: the margins do not care)"""
    rc = SC.REF_CASES[k]
    q = SC.ref_inputs(rc)
    assert q["hybrid"].shape == (rc.N, rc.E) and rc.H * rc.W <= 64 * 96 and rc.S <= 3
    ks = set()
    for s, t in enumerate(q["sentences"]):
        gem = O.coherence_scores(t["imgattn"], q["masks"], t["dirflag"], t["black"])
        assert not np.isnan(gem).any()
        for r, a, k1, k2 in [(0.5, 0.6, rc.k1, rc.k2)] + SC.SWEEP:
            ref = SC.reference(SC.ref_sentence_inputs(q, s, gem, 100.0, r, k1, k2, a))
            d = SC.decided(ref)
            assert d["pure"] and d["final"], (rc.name, s, (r, a, k1, k2), {n: (g.tolist(), need) for n, (g, need) in SC.margins(ref).items()})
            ks.add((k1, k2))
    assert {(k1, k2) for k1 in (1, 2, 16) for k2 in (1, 16)} <= ks
    same_r = [t for t in SC.SWEEP if t[0] == 0.5]
    assert {(t[2], t[3]) for t in same_r} == {(k1, k2) for k1 in (1, 2, 16) for k2 in (1, 16)}      # one r-group: the prefix property
    assert {t[0] for t in SC.SWEEP} >= {0.0, 1.0} and {t[1] for t in SC.SWEEP} >= {0.0, 1.0}
