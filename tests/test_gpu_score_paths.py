"""The per-sentence scoring on every path against the float64 reference of tests/score_cases.py: score_lists_body +
score_blend_body under score_sentence_kernel (ops.score_sentence: every case and probe of score_cases.ALL), under grp_score_kernel
(ops.score_ref, ops.score_group) and under grp_sweep_score_kernel (ops.score_group_sweep), and calc_score_kernel
(ops.calculate_score) at the same widths and counts.  Every logit is judged by score_cases.check against the reference -- never
against another entry -- and every index must be the reference's: tests/test_score_cases_host.py asserts that the reference alone
decides each of them.  For the fused entries the coherence scores the device pooled (want_scores; pinned by
tests/test_gpu_coherence_paths.py) are the reference's `gem` input; the sweep has no score rows and takes those of
ops.score_group on the same ref.

Everything is launched once (module fixtures).  Run with -s for the worst ratio of the device error to the bound, per entry."""
import numpy as np
import pytest
import torch

import score_cases as SC

pytestmark = pytest.mark.gpu

IDS = [SC.case_id(c) for c in SC.ALL]
LOGIT_SCALE = 100.0
BASE = (0.5, 0.6)       # r, alpha of the score_ref / score_group calls


def dev_of(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def world(cuda):
    """per case and probe: (case, reference, (idx, score_clip, score_neg) of ops.score_sentence)"""
    from hybridgl_amd import ops
    rows = []
    for c in SC.ALL:
        x = SC.inputs(c)
        got = ops.score_sentence(dev_of(x.hybrid, cuda), dev_of(x.sent, cuda), dev_of(x.nphr, cuda),
                                 dev_of(x.others, cuda) if x.others is not None else None, dev_of(x.boxes, cuda), dev_of(x.gem, cuda),
                                 float(x.scale), float(x.r), x.k1, x.k2, float(x.alpha), x.rela, x.has_other)
        rows.append((c, SC.reference(x), got))
    torch.cuda.synchronize()
    return [(c, ref, tuple(t.cpu().numpy() for t in got)) for c, ref, got in rows]


@pytest.mark.parametrize("k", range(len(SC.ALL)), ids=IDS)
def test_score_sentence(world, k):
    c, ref, got = world[k]
    d = SC.decided(ref, SC.has_ties(c))
    assert d["pure"] and d["final"]          # (tests/test_score_cases_host.py: no index is left to the implementation)
    w = SC.check(got, ref, SC.has_ties(c), c.name)
    print(f"score ratio to bound: score_sentence   {c.name:60s} {w:.4g}")


def test_score_sentence_worst_ratio(world):
    worst = max((float(max(SC.logit_ratios(g[1], ref.clip, ref.scale).max(), SC.logit_ratios(g[2], ref.neg, ref.scale).max())), c.name)
                for c, ref, g in world)
    print(f"score ratio to bound: score_sentence   worst {worst[0]:.4g} ({worst[1]}), C = {SC.C_BOUND}")
    assert worst[0] <= 1


def test_calculate_score(cuda):
    """the (N, E) of the cases with one and three text rows; logit_scale 100 and CLIP's own 1 / 0.07"""
    from hybridgl_amd import ops
    shapes = sorted({(c.N, c.E) for c in SC.CASES})
    calls = []
    for i, (N, E) in enumerate(shapes):
        rng = np.random.default_rng([N, E, 13])
        img = rng.standard_normal((N, E)).astype(np.float32)
        for T in (1, 3):
            txt = rng.standard_normal((T, E)).astype(np.float32)
            scale = 100.0 if (i + T) % 2 else 1 / 0.07
            calls.append((N, E, T, scale, img, txt, ops.calculate_score(dev_of(img, cuda), dev_of(txt, cuda), scale)))
    torch.cuda.synchronize()
    worst = (0.0, None)
    for N, E, T, scale, img, txt, out in calls:
        r = SC.logit_ratios(out.cpu().numpy(), SC.cosine_logits(img, txt, scale), scale)
        worst = max(worst, (float(r.max()), (N, E, T)))
        assert r.max() <= 1, f"calculate_score N={N} E={E} T={T}: ratio {float(r.max())}"
    print(f"score ratio to bound: calculate_score  worst {worst[0]:.4g} at (N, E, T) = {worst[1]} over {len(calls)} calls")
    assert {T for _, _, T, *_ in calls} == {1, 3} and worst[0] > 0


# ---- whole refs through the fused entries -----------------------------------------------------------------------------------
class RefWorld:
    """one ref of score_cases.REF_CASES on the device and its rows from ops.score_ref, ops.score_group and the sweep"""

    def __init__(self, rc, dev):
        from hybridgl_amd import ops
        self.rc = rc
        self.np = q = SC.ref_inputs(rc)
        target = dev_of(q["target"], dev)
        sents = [dict(t, imgattn=dev_of(t["imgattn"], dev), target=target) for t in q["sentences"]]
        self.q = dict(hybrid=dev_of(q["hybrid"], dev), text=dev_of(q["text"], dev), boxes=dev_of(q["boxes"], dev),
                      masks=dev_of(q["masks"], dev), sentences=sents, k1=rc.k1, k2=rc.k2)
        d = self.q
        self.score_ref = ops.score_ref(d["hybrid"], d["text"], d["boxes"], d["masks"], sents, LOGIT_SCALE, BASE[0], rc.k1, rc.k2, BASE[1],
                                       want_scores=True)
        self.score_group = ops.score_group([d], LOGIT_SCALE, BASE[0], BASE[1], want_scores=True)[0]
        self.sweep = ops.score_group_sweep([d], SC.SWEEP, LOGIT_SCALE)[0]
        torch.cuda.synchronize()

    def judge(self, entry, out):
        idx, _, clip, neg, gem = (t.cpu().numpy() for t in out)
        worst = 0.0
        for s in range(self.rc.S):
            assert not np.isnan(gem[s]).any()
            ref = SC.reference(SC.ref_sentence_inputs(self.np, s, gem[s], LOGIT_SCALE, BASE[0], self.rc.k1, self.rc.k2, BASE[1]))
            d = SC.decided(ref)
            assert d["pure"] and d["final"], f"{entry} {self.rc.name} sentence {s}: the reference does not decide"
            worst = max(worst, SC.check((idx[s], clip[s], neg[s]), ref, False, f"{entry} {self.rc.name} sentence {s}"))
        print(f"score ratio to bound: {entry:16s} {self.rc.name:24s} worst {worst:.4g}")
        return worst


@pytest.fixture(scope="module")
def ref_worlds(cuda):
    return [RefWorld(rc, cuda) for rc in SC.REF_CASES]


REF_IDS = [SC.case_id(rc) for rc in SC.REF_CASES]


@pytest.mark.parametrize("k", range(len(SC.REF_CASES)), ids=REF_IDS)
def test_score_ref(ref_worlds, k):
    assert 0 < ref_worlds[k].judge("score_ref", ref_worlds[k].score_ref) <= 1


@pytest.mark.parametrize("k", range(len(SC.REF_CASES)), ids=REF_IDS)
def test_score_group(ref_worlds, k):
    assert 0 < ref_worlds[k].judge("score_group", ref_worlds[k].score_group) <= 1


@pytest.mark.parametrize("k", range(len(SC.REF_CASES)), ids=REF_IDS)
def test_score_group_sweep(ref_worlds, k):
    """every configuration's row against the reference UNDER THAT configuration: k1 in {1, 2, 16} x k2 in {1, 16} share one r, so
    their lists are prefixes of one pair of lists built to (16, 16)"""
    w = ref_worlds[k]
    idx = w.sweep[0].cpu().numpy()
    gem = w.score_group[4].cpu().numpy()
    assert idx.shape == (len(SC.SWEEP), w.rc.S, 2)
    finals = set()
    for c, (r, a, k1, k2) in enumerate(SC.SWEEP):
        for s in range(w.rc.S):
            ref = SC.reference(SC.ref_sentence_inputs(w.np, s, gem[s], LOGIT_SCALE, r, k1, k2, a))
            d = SC.decided(ref)
            assert d["pure"] and d["final"], f"sweep {w.rc.name} configuration {c} sentence {s}: the reference does not decide"
            SC.check_indices(idx[c, s], ref, False, f"sweep {w.rc.name} configuration {(r, a, k1, k2)} sentence {s}")
            finals.add((s, ref.final))
    if w.rc.N > 3:
        assert len(finals) > w.rc.S          # the configurations do not all answer alike
    # the logits of the sweep's r = 0.5 group are those of score_group (same r): its bound is the sweep's
    print(f"score ratio to bound: sweep            {w.rc.name:24s} indices of {len(SC.SWEEP)} configurations x {w.rc.S} sentences equal")
