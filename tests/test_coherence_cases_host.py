"""CPU: tests/coherence_cases.py itself -- the constants it reads from csrc/scoring.hip, the launch routes its cases reach, its
reference against the numpy oracle and against a torch-float32 restatement of Hybridgl_main.py:203-223, and its checker against
planted errors (each must be rejected on at least one case, and the same implementation without the error accepted on all)."""
import numpy as np
import pytest
import torch

import coherence_cases as CC
from oracle import clip_oracle as O

IDS = [CC.case_id(c) for c in CC.CASES]


def test_constants_parse_from_scoring_hip():
    k = CC.constants()
    assert set(k) == {"PX_LANE", "PIX_PER_BLOCK", "MASK_GROUP", "REF_MASK_GROUP", "REF_MAXS", "REF_MM_BLOCKS"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    assert k["PIX_PER_BLOCK"] == 256 * k["PX_LANE"]          # 256 threads of PX_LANE pixels: what `routes` and the masks assume
    assert k["MASK_GROUP"] < k["REF_MASK_GROUP"]


def test_cases_are_the_planes_and_inputs_they_claim():
    assert [(c.H, c.W) for c in CC.CASES] == [(3, 7), (40, 50), (64, 64), (128, 128), (64, 65), (97, 131), (1, 4097), (4097, 1), (33, 2),
                                              (5, 15)]
    assert sorted(c.N for c in CC.CASES) == [8] + [9] * 7 + [33, 40]
    seen = set()
    for c in CC.CASES:
        kinds = CC.mask_kinds(c)
        assert len(kinds) == c.N and kinds[:4] == ["empty", "full", "hole_max", "hole_min"]
        seen |= set(kinds)
        m = CC.masks_for(c)
        HW = c.H * c.W
        cnt = (m.reshape(c.N, -1) != 0).sum(1)
        assert cnt[0] == 0 and cnt[1] == HW and cnt[2] == cnt[3] == HW - 1
        pmax, pmin = CC.extremes(c)
        for h in ("smooth", "signed", "peaked", "negzero"):
            a = CC.heat_for(c, h).reshape(-1)
            assert a[pmax] == a.max() and (a == a.max()).sum() == 1 and a[pmin] == a.min(), (c, h)
            assert m.reshape(c.N, -1)[2, pmax] == 0 and m.reshape(c.N, -1)[3, pmin] == 0
        a = CC.heat_for(c, "signed")
        assert a.min() < 0 < a.max()
        a = CC.heat_for(c, "ends").reshape(-1)
        assert a.argmax() == 0 and a.argmin() == HW - 1
        a = CC.heat_for(c, "negzero")
        assert np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all() and a.min() == 0
        a = CC.heat_for(c, "peaked").reshape(-1)
        assert a[pmax] == 1 and np.delete(a, pmax).max() < 1.2e-3
        assert np.ptp(CC.heat_for(c, "constant")) == 0
    assert seen >= set(CC.KINDS)
    big = {n: CC.masks_for(c) for c in CC.CASES if c.N >= 18 for n in [c.N]}
    for m in big.values():          # the byte values of the blobs
        assert {2, 0x7f, 0x80, 0xff} <= set(np.unique(m).tolist())
    s = CC.sentences_for(CC.CASES[0])
    assert len(s) == 24 and {t[1] for t in s} == set(CC.DIRFLAGS) and {t[2] for t in s} == {1.5, 1.8, 1.95}


def test_routes_reach_every_path():
    K = CC.CONST
    launches, ns = set(), {3: set(), 4: set()}
    groups = {K["MASK_GROUP"]: set(), K["REF_MASK_GROUP"]: set()}
    for c in CC.CASES:
        r = CC.routes(c.H, c.W, c.N, 1, "coherence_scores")
        launches.add(frozenset(r["launches"]))
        assert r["NS"] <= {1} and r["MG"] == K["MASK_GROUP"]
        for entry in ("score_ref", "score_group"):
            for S in (1, 2, 3, 4, 5, 6, 7, 17):      # S_LIST of tests/test_gpu_coherence_paths.py
                r = CC.routes(c.H, c.W, c.N, S, entry)
                assert r["CH"] == (3 if S <= 3 else 4) and sum(r["rows"]) == S and max(r["rows"]) <= K["REF_MAXS"]
                ns[r["CH"]] |= r["NS"]
                groups[r["MG"]].add((c.N <= r["MG"], r["groups"]))
        # one score_group call over the six refs of a plane: a 17-sentence ref beside it sends a short ref through CH = 4
        r = CC.routes(c.H, c.W, c.N, 3, "score_group", call_S=(1, 2, 3, 4, 5, 17))
        assert r["CH"] == 4 and (r["NS"] == {3} or not r["NS"])
    assert launches == {frozenset({"full"}), frozenset({"partial"}), frozenset({"full", "partial"})}
    assert ns[3] == {1, 2, 3} and ns[4] == {1, 2, 3, 4}    # S = 5, 6, 7 and 17 leave one, two, three and one map for a last pass
    r = CC.routes(97, 131, 33, 3, "score_group", call_S=(3, 17))
    assert r["NS"] == {3} and r["CH"] == 4                   # NS = 3 under CH = 4 ...
    r = CC.routes(97, 131, 33, 2, "score_group", call_S=(2, 17))
    assert r["NS"] == {2} and r["CH"] == 4                   # ... and NS = 2: the calls of test_gpu_coherence_paths.py with all planes
    for mg, seen in groups.items():
        assert {below for below, _ in seen} == {True, False}, f"MG {mg}: N on one side of the group boundary only"
    N = sorted({c.N for c in CC.CASES})
    assert K["MASK_GROUP"] in N and K["MASK_GROUP"] + 1 in N and K["REF_MASK_GROUP"] + 1 in N
    assert max(n for n in N if n <= K["REF_MASK_GROUP"]) >= K["MASK_GROUP"] + 1


def torch_f32(attn, masks, dirflag, black):
    """Hybridgl_main.py:203-223 with utils.py:135-161, line by line in torch float32 on the CPU.  `black` is the float32 the C
    ABI carries (2 - black is then exact in float32, as in the device code); a mask byte counts when it is not zero."""
    a = torch.from_numpy(np.ascontiguousarray(attn))
    H, W = a.shape
    a = (a - a.min()) / (a.max() - a.min())
    if dirflag == "left":
        pm = torch.linspace(1, 0, W).expand(H, W)
    elif dirflag == "right":
        pm = torch.linspace(0, 1, W).expand(H, W)
    elif dirflag == "middle":
        pm = torch.cat([torch.linspace(0, 1, W // 2), torch.linspace(1, 0, W - W // 2)]).expand(H, W)
    else:
        pm = torch.ones(H, W)
    a = a * pm
    a = a / a.mean()
    black = float(np.float32(black))
    out = []
    for m in masks:
        pred = torch.from_numpy((m != 0).astype(np.uint8))
        out.append(float((a * (2 - black) * pred / (pred.sum())).sum() - (a * black * (1 - pred) / ((1 - pred).sum())).sum()))
    return np.asarray(out)


@pytest.fixture(scope="module")
def world():
    """per case: masks, and per sentence (heat-map, reference)"""
    out = []
    for c in CC.CASES:
        masks = CC.masks_for(c)
        sent = []
        for h, d, b in CC.sentences_for(c):
            attn = CC.heat_for(c, h)
            sent.append((attn, d, b, CC.reference(attn, masks, d, b)))
        out.append((masks, sent))
    return out


def test_reference_has_nan_exactly_where_the_operation_divides_zero_by_zero(world):
    for c, (masks, sent) in zip(CC.CASES, world):
        for (h, d, b), (attn, _, _, ref) in zip(CC.sentences_for(c), sent):
            v = CC.normalised(attn, d)
            if h == "constant" or not (v > 0).any():        # flat map; W = 1 under `right`: the ramp is 0 on the whole plane
                assert np.isnan(ref[0]).all(), (c, h, d)
            else:      # the empty and the full mask (on a plane without full blocks, "full_blocks" is empty too, and so on)
                cnt = (masks.reshape(c.N, -1) != 0).sum(1)
                assert np.array_equal(np.isnan(ref[0]), (cnt == 0) | (cnt == c.H * c.W)), (c, h, d)
                assert np.isnan(ref[0][:2]).all() and not np.isnan(ref[0][2:4]).any()
                ok = ~np.isnan(ref[0])
                assert (ref[1][ok] >= 0).all() and (ref[2][ok] >= 0).all()


@pytest.mark.parametrize("k", range(len(CC.CASES)), ids=IDS)
def test_reference_agrees_with_the_numpy_oracle(world, k):
    masks, sent = world[k]
    for attn, d, b, ref in sent:
        with np.errstate(all="ignore"):
            CC.check(O.coherence_scores(attn, masks, d, b), ref, f"{IDS[k]} {d} {b}")


def test_reference_agrees_with_torch_float32(world):
    """the reference program's own arithmetic fits under C on every case (run with -s for the figures)"""
    worst = 0.0
    for c, (masks, sent) in zip(CC.CASES, world):
        w = max(CC.check(torch_f32(attn, masks, d, b), ref, f"{CC.case_id(c)} {d} {b}") for attn, d, b, ref in sent)
        print(f"torch float32 / bound, {CC.case_id(c):14s} {w:.3f}")
        worst = max(worst, w)
    print(f"torch float32 / bound, worst: {worst:.3f} (C = {CC.C_BOUND})")
    assert 0 < worst <= 1


def test_check_accepts_a_direct_float32_implementation_and_rejects_each_planted_error(world):
    caught = {d: 0 for d in CC.DEFECTS}
    for c, (masks, sent) in zip(CC.CASES, world):
        for attn, d, b, ref in sent[::5]:
            CC.check(CC.planted(attn, masks, d, b), ref, f"{CC.case_id(c)} {d} {b}")
            for defect in CC.DEFECTS:
                r = CC.ratios(CC.planted(attn, masks, d, b, defect), ref)
                caught[defect] += int((r > 1).any())
    assert all(v > 0 for v in caught.values()), caught
    # the subtraction in float32 is what the near-full masks are for: it passes the half-plane masks and misses the holes
    c = CC.CASES[5]
    masks, sent = world[5]
    attn, d, b, ref = sent[0]
    r = CC.ratios(CC.planted(attn, masks, d, b, "tot_minus_s_f32"), ref)
    kinds = CC.mask_kinds(c)
    # (not the hole at the minimum: its outside value is 0, and adding 0 leaves inside == total bit for bit)
    assert r[kinds.index("hole_first")] > 1 and r[kinds.index("hole_two")] > 1 and r[kinds.index("checker")] <= 1


def test_check_rejects_a_nan_out_of_place_and_a_missing_one():
    c = CC.CASES[2]
    masks, attn = CC.masks_for(c), CC.heat_for(c, "smooth")
    ref = CC.reference(attn, masks, "left", 1.8)
    good = ref[0].astype(np.float32)
    assert CC.check(good, ref) <= 1
    for at, v in ((0, 0.0), (1, np.inf), (5, np.nan)):
        bad = good.copy()
        bad[at] = v
        with pytest.raises(AssertionError):
            CC.check(bad, ref)
