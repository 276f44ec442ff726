"""The coherence pooling on every path against the float64 reference of tests/coherence_cases.py: pool_block<NS, FULL> under
masked_pool_kernel (ops.coherence_scores) and under grp_masked_pool_kernel<MG, CH> / grp_masked_pool_last_kernel<MG>
(ops.score_ref: MG = 8, ops.score_group: MG = 32), both min / max paths, both final reductions and the direct outside sum of
the masks that cover more than half of the plane.  Every `gem` row is judged by coherence_cases.check against the reference,
never against another entry; that the entries agree with each other bit for bit ALSO on the near-full masks (which
tests/test_gpu_tail_entries.py has none of) is asserted beside it.

The planes, masks and heat-maps are those of coherence_cases.CASES; the mask planes of a case live twice on the device, at a
16-byte-aligned address and one byte behind one.  References and the per-sentence results are computed once (module fixture).
Run with -s for the worst ratio of the device error to the bound, per entry and case."""
import numpy as np
import pytest
import torch

import coherence_cases as CC

pytestmark = pytest.mark.gpu

E = 80
LOGIT_SCALE, R_MIX, K1, K2, ALPHA = 100.0, 0.5, 3, 6, 0.6
S_LIST = (1, 2, 3, 4, 5, 6, 7, 17)      # CH = 3: NS 1, 2, 3; CH = 4: NS 4, 4 + 1, 4 + 2, 4 + 3; 17: more than a row of REF_MAXS
IDS = [CC.case_id(c) for c in CC.CASES]
RELA = ("none", "left", "big", "within")


def same(u, v):
    return bool((torch.isnan(u) == torch.isnan(v)).all()) and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))


def at_offset(planes, start, dev):
    """uint8 device tensor of `planes` that begins `start` bytes behind a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.zeros(planes.size + 32, dtype=torch.uint8, device=dev)
    o = (-buf.data_ptr()) % 16 + start
    t = buf[o:o + planes.size].view(*planes.shape)
    t.copy_(torch.from_numpy(planes))
    assert t.data_ptr() % 16 == start
    return t


class World:
    """one case on the device: masks at both alignments, the 24 sentences with heat-map, reference and ops.coherence_scores"""

    def __init__(self, c, dev):
        from hybridgl_amd import ops
        self.c = c
        planes = CC.masks_for(c)
        self.masks = [at_offset(planes, 0, dev), at_offset(planes, 1, dev)]
        self.target = at_offset(planes[min(5, c.N - 1)], 0, dev)
        g = torch.Generator(device="cpu").manual_seed(c.H * 1000 + c.W)
        self.hybrid = torch.randn(c.N, E, generator=g).to(dev)
        self.boxes = torch.randint(0, 40, (c.N, 4), generator=g).to(dev)
        self.text = torch.randn(3 * max(S_LIST), E, generator=g).to(dev)
        self.sent = []
        for h, d, b in CC.sentences_for(c):
            attn = CC.heat_for(c, h)
            dev_attn = torch.from_numpy(attn).to(dev)
            got = [ops.coherence_scores(dev_attn, m, d, b) for m in self.masks]
            self.sent.append(dict(heat=h, dirflag=d, black=b, attn=dev_attn, ref=CC.reference(attn, planes, d, b), got=got))
        torch.cuda.synchronize()

    def ref_of(self, S, first, align):
        """a ref of S sentences, the case's sentences from `first` on in rotation; (operands of ops.score_group, sentence indices)"""
        which = [(first + j) % len(self.sent) for j in range(S)]
        recs = [dict(sentence_row=3 * j, noun_phrase_row=3 * j + 1, other_row0=3 * j + 2, n_other=1, dirflag=self.sent[w]["dirflag"],
                     relaword=RELA[j % 4], has_other_nouns=j % 2 == 0, black=self.sent[w]["black"], imgattn=self.sent[w]["attn"],
                     target=self.target) for j, w in enumerate(which)]
        q = dict(hybrid=self.hybrid, text=self.text[:3 * S], boxes=self.boxes, masks=self.masks[align], sentences=recs, k1=K1, k2=K2)
        return q, which


@pytest.fixture(scope="module")
def worlds(cuda):
    return [World(c, cuda) for c in CC.CASES]


def judge(entry, w, rows):
    """rows: (what, gem [N] device tensor, sentence index).  Prints the worst ratio to the bound, then asserts the bound on every
    row and that every row holds the bits of ops.coherence_scores for its sentence."""
    rows = [(what, gem.cpu().numpy(), gem, k) for what, gem, k in rows]
    worst = max(float(CC.ratios(g, w.sent[k]["ref"]).max()) for _, g, _, k in rows)
    print(f"coherence ratio to bound: {entry:24s} {CC.case_id(w.c):14s} worst {worst:.4g} over {len(rows)} rows")
    for what, g, gem, k in rows:
        s = w.sent[k]
        CC.check(g, s["ref"], f"{entry} {CC.case_id(w.c)} {what}: {s['heat']} {s['dirflag']} black {s['black']}")
        assert same(gem, s["got"][0]), f"{entry} {CC.case_id(w.c)} {what}: not the bits of ops.coherence_scores"


@pytest.mark.parametrize("k", range(len(CC.CASES)), ids=IDS)
def test_coherence_scores(worlds, k):
    """every heat-map under every dirflag, the mask planes aligned and one byte off"""
    w = worlds[k]
    r = CC.routes(w.c.H, w.c.W, w.c.N, 1, "coherence_scores")
    assert r["launches"] and r["groups"] == -(-w.c.N // CC.CONST["MASK_GROUP"])
    judge("coherence_scores", w, [(f"align {a}", s["got"][a], i) for i, s in enumerate(w.sent) for a in (0, 1)])


def fused_rows(outs, whichs, what):
    rows = []
    for out, which, tag in zip(outs, whichs, what):
        gem = out[4]
        assert gem.shape[0] == len(which)
        rows += [(f"{tag} sentence {j}", gem[j], sk) for j, sk in enumerate(which)]
    return rows


@pytest.mark.parametrize("k", range(len(CC.CASES)), ids=IDS)
def test_score_ref(worlds, k):
    from hybridgl_amd import ops
    w = worlds[k]
    outs, whichs = [], []
    for i, S in enumerate(S_LIST):
        q, which = w.ref_of(S, 5 * i, i % 2)
        outs.append(ops.score_ref(q["hybrid"], q["text"], q["boxes"], q["masks"], q["sentences"], LOGIT_SCALE, R_MIX, K1, K2, ALPHA,
                                  want_scores=True))
        whichs.append(which)
    judge("score_ref", w, fused_rows(outs, whichs, [f"S = {S}" for S in S_LIST]))


@pytest.mark.parametrize("k", range(len(CC.CASES)), ids=IDS)
def test_score_group_one_ref_per_call(worlds, k):
    """S <= 3 alone in a call: CH = 3"""
    from hybridgl_amd import ops
    w = worlds[k]
    outs, whichs = [], []
    for i, S in enumerate(S_LIST):
        q, which = w.ref_of(S, 7 * i + 1, (i + 1) % 2)
        outs.append(ops.score_group([q], LOGIT_SCALE, R_MIX, ALPHA, want_scores=True)[0])
        whichs.append(which)
    judge("score_group, one ref", w, fused_rows(outs, whichs, [f"S = {S}" for S in S_LIST]))


@pytest.mark.parametrize("k", range(len(CC.CASES)), ids=IDS)
def test_score_group_the_refs_of_a_plane_in_one_call(worlds, k):
    """the short refs beside the long ones: NS = 1, 2, 3 under CH = 4"""
    from hybridgl_amd import ops
    w = worlds[k]
    refs, whichs = zip(*[w.ref_of(S, 3 * i + 2, i % 2) for i, S in enumerate(S_LIST)])
    outs = ops.score_group(list(refs), LOGIT_SCALE, R_MIX, ALPHA, want_scores=True)
    judge("score_group, 8 refs", w, fused_rows(outs, whichs, [f"S = {S}" for S in S_LIST]))


def test_score_group_all_planes_in_one_call(worlds):
    """one ref per plane in one launch: the grid is sized by the 128 x 128 plane and the 40 masks, the surplus blocks of the
    other rows leave early; a 17-sentence ref among them"""
    from hybridgl_amd import ops
    S_of = [1, 2, 3, 4, 5, 17, 3, 2, 1, 4]
    refs, whichs = zip(*[w.ref_of(S, 11 + i, i % 2) for i, (w, S) in enumerate(zip(worlds, S_of))])
    outs = ops.score_group(list(refs), LOGIT_SCALE, R_MIX, ALPHA, want_scores=True)
    for w, out, which, S in zip(worlds, outs, whichs, S_of):
        judge("score_group, all planes", w, fused_rows([out], [which], [f"S = {S}"]))


def test_results_are_the_same_bits_from_run_to_run(worlds):
    """the direct outside sum is a fixed order of double adds: the case with every mask kind, five runs"""
    from hybridgl_amd import ops
    w = worlds[5]
    for s in w.sent[::3]:
        for _ in range(5):
            assert same(ops.coherence_scores(s["attn"], w.masks[1], s["dirflag"], s["black"]), s["got"][0])
