"""The two fused entries of the scoring tail, hgl_score_ref and hgl_score_group, called directly (hybridgl_amd.ops / ctypes)
against the per-sentence entries -- hgl_coherence_scores + hgl_score_sentence + 2 x hgl_iou_select per sentence, the independent
implementation include/hybridgl.h promises they equal bit for bit -- plus their error paths and the IoU counts against numpy.

The refs are chosen for where the kernels can go wrong, not for the workload: (N, H, W, S)
    (1, 64, 64, 2)     one proposal (the k1 / k2 clamp); the plane is exactly one full pooling block, no partial block
    (13, 97, 131, 5)   odd plane: full blocks and a partial last block, unaligned mask planes; two pooling passes (4 + 1 maps)
    (7, 120, 160, 9)   three pooling passes
    (5, 80, 72, 16)    a full row of sentences
    (3, 40, 50, 18)    plane smaller than one block (only the partial-block launch); more sentences than a row holds
    (40, 64, 96, 3)    more masks than one mask group of 32, and more than four groups of 8
Every per-sentence result is computed once (module fixture) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 64, 2), (13, 97, 131, 5), (7, 120, 160, 9), (5, 80, 72, 16), (3, 40, 50, 18), (40, 64, 96, 3)]
E = 80                     # not a multiple of the 64 lanes that stride over a feature row
LOGIT_SCALE, R_MIX, K1, K2, ALPHA = 100.0, 0.5, 3, 6, 0.6
HGL_EINVAL, HGL_EWORKSPACE = -1, -3


def same(u, v):
    """bit for bit, as test_fused_tail_equals_per_sentence_launches compares: NaN positions equal and nan_to_num equal"""
    if not u.is_floating_point():
        return torch.equal(u, v)
    return bool((torch.isnan(u) == torch.isnan(v)).all()) and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))


def make_ref(i, shape, dev):
    """operands of one ref as ops.score_group takes them (+ the ref's seed): synthetic masks / boxes / heat-maps / target, random
    hybrid and text features, the second sentence without other nouns"""
    from hybridgl_amd.pipeline import black_for, synthetic_ref
    N, H, W, S = shape
    ref = synthetic_ref(i, dev, N=N, H=H, W=W, n_sent=S, vocab=512, context=16)[0]
    ref.sentences[1].other_noun_rows = []
    ref.sentences[1].n_nouns = 0
    g = torch.Generator(device="cpu").manual_seed(100 + i)
    hybrid = torch.randn(N, E, generator=g).to(dev)
    text = torch.randn(3 * S, E, generator=g).to(dev)
    recs = [dict(sentence_row=s.sentence_row, noun_phrase_row=s.noun_phrase_row,
                 other_row0=s.other_noun_rows[0] if s.other_noun_rows else 0, n_other=len(s.other_noun_rows), dirflag=s.dirflag,
                 relaword=s.relaflag, has_other_nouns=s.n_nouns != 0, black=black_for(s.relaflag), imgattn=s.imgattn,
                 target=ref.target) for s in ref.sentences]
    return dict(hybrid=hybrid, text=text, boxes=ref.boxes, masks=ref.masks, sentences=recs, k1=K1, k2=K2)


def per_sentence(q):
    """(idx [S,2], iu [S,4], score_clip, score_neg, gem [S,N]) of a ref through the per-sentence entries"""
    from hybridgl_amd import ops
    idx, iu, sc, sn, gm = [], [], [], [], []
    for t in q["sentences"]:
        gem = ops.coherence_scores(t["imgattn"], q["masks"], t["dirflag"], t["black"])
        others = q["text"][t["other_row0"]:t["other_row0"] + t["n_other"]] if t["n_other"] else None
        i2, c, n = ops.score_sentence(q["hybrid"], q["text"][t["sentence_row"]], q["text"][t["noun_phrase_row"]], others, q["boxes"],
                                      gem, LOGIT_SCALE, R_MIX, q["k1"], q["k2"], ALPHA, t["relaword"], t["has_other_nouns"])
        iu.append(torch.cat([ops.iou_select(q["masks"], i2, 0, t["target"]), ops.iou_select(q["masks"], i2, 1, t["target"])]))
        idx.append(i2); sc.append(c); sn.append(n); gm.append(gem)
    return tuple(torch.stack(x) for x in (idx, iu, sc, sn, gm))


@pytest.fixture(scope="module")
def world(cuda):
    refs = [make_ref(i, s, cuda) for i, s in enumerate(SHAPES)]
    want = [per_sentence(q) for q in refs]
    torch.cuda.synchronize()
    return refs, want


def score_ref(q, **kw):
    from hybridgl_amd import ops
    return ops.score_ref(q["hybrid"], q["text"], q["boxes"], q["masks"], q["sentences"], LOGIT_SCALE, R_MIX, q["k1"], q["k2"], ALPHA, **kw)


def assert_rows(got, want, what):
    names = ("idx", "iu", "score_clip", "score_neg", "gem")
    for name, u, v in zip(names, got, want):
        assert u.shape == v.shape and same(u, v), f"{what}: {name} differs"


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_score_ref_equals_per_sentence_entries(cuda, world, k):
    refs, want = world
    q, w = refs[k], want[k]
    cum = torch.zeros(4, dtype=torch.int64, device=cuda)
    assert_rows(score_ref(q, cum=cum, want_scores=True), w, "want_scores")
    got = score_ref(q, cum=cum)           # the score rows go to the spare buffers of the workspace
    assert len(got) == 2
    assert_rows(got, w[:2], "spare buffers")
    assert torch.equal(cum, 2 * w[1].sum(0)) and int(cum[1]) > 0        # cum accumulates
    assert_rows(score_ref(q, cum=None, want_scores=True), w, "cum=None")


def group_case(refs, want, cuda):
    """ops.score_group of `refs` in one call against the per-sentence rows `want`"""
    from hybridgl_amd import ops
    cum = torch.zeros(4, dtype=torch.int64, device=cuda)
    outs = ops.score_group(refs, LOGIT_SCALE, R_MIX, ALPHA, cum=cum, want_scores=True)
    assert len(outs) == len(refs)
    for i, (got, w) in enumerate(zip(outs, want)):
        assert_rows(got, w, f"ref {i}")
    assert torch.equal(cum, sum(w[1].sum(0) for w in want))
    for i, (got, w) in enumerate(zip(ops.score_group(refs, LOGIT_SCALE, R_MIX, ALPHA), want)):
        assert len(got) == 2
        assert_rows(got, w[:2], f"ref {i}, spare buffers, cum=None")


def test_score_group_equals_per_sentence_entries(cuda, world):
    """all six refs in one call, the 18-sentence ref among them (two rows of the launch)"""
    refs, want = world
    group_case(refs, want, cuda)


def test_score_group_of_17_refs_equals_score_ref(cuda):
    """more refs than one launch holds (16): the first five shapes cycled"""
    from hybridgl_amd import ops
    refs = [make_ref(20 + i, SHAPES[i % 5], cuda) for i in range(17)]
    cum_r = torch.zeros(4, dtype=torch.int64, device=cuda)
    want = [score_ref(q, cum=cum_r, want_scores=True) for q in refs]
    cum_g = torch.zeros(4, dtype=torch.int64, device=cuda)
    outs = ops.score_group(refs, LOGIT_SCALE, R_MIX, ALPHA, cum=cum_g, want_scores=True)
    for i, (got, w) in enumerate(zip(outs, want)):
        assert_rows(got, w, f"ref {i}")
    assert torch.equal(cum_g, cum_r) and int(cum_g[1]) > 0


# ---- error paths, through ctypes: the return code, and nothing written -----------------------------------------------------
def pack(q, keep):
    """HglSentence array of a ref's sentence dicts (the tensors behind the pointers go to `keep`)"""
    from hybridgl_amd import _lib, ops
    arr = (_lib.HglSentence * len(q["sentences"]))()
    for j, t in enumerate(q["sentences"]):
        tgt = t["target"].view(torch.uint8) if t["target"].dtype == torch.bool else t["target"]
        keep += [t["imgattn"], tgt]
        arr[j] = _lib.HglSentence(t["sentence_row"], t["noun_phrase_row"], t["other_row0"], t["n_other"],
                                  t["dirflag"] if isinstance(t["dirflag"], int) else ops.DIRFLAG[t["dirflag"]],
                                  ops.RELAWORD.get(t["relaword"], 0), int(t["has_other_nouns"]), t["black"], t["imgattn"].data_ptr(),
                                  tgt.data_ptr())
    return arr


class Outputs:
    """outputs of one ref, pre-filled so that any write shows"""
    def __init__(self, q, dev):
        S, N = len(q["sentences"]), q["hybrid"].shape[0]
        self.idx = torch.full((S, 2), -7, dtype=torch.int32, device=dev)
        self.iu = torch.full((S, 4), -7, dtype=torch.int64, device=dev)
        self.scores = [torch.full((S, N), -7.0, device=dev) for _ in range(3)]

    def untouched(self):
        return bool((self.idx == -7).all()) and bool((self.iu == -7).all()) and all(bool((s == -7.0).all()) for s in self.scores)


def call_score_ref(q, out, cum, k1=K1, short=0):
    from hybridgl_amd import _lib
    lib = _lib.load()
    keep = []
    arr = pack(q, keep)
    N, S = q["hybrid"].shape[0], len(q["sentences"])
    masks = q["masks"].view(torch.uint8)
    _, H, W = masks.shape
    need = lib.hgl_score_ref_workspace_bytes(S, N, E, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=masks.device)
    rc = lib.hgl_score_ref(q["hybrid"].data_ptr(), q["text"].data_ptr(), q["text"].shape[0], q["boxes"].data_ptr(), masks.data_ptr(), N, E, H,
                           W, arr, S, LOGIT_SCALE, R_MIX, k1, q["k2"], ALPHA, out.idx.data_ptr(), out.iu.data_ptr(), cum.data_ptr(),
                           out.scores[0].data_ptr(), out.scores[1].data_ptr(), out.scores[2].data_ptr(), ws.data_ptr(), need - short,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def call_score_group(refs, outs, cum, k1=(K1, K1), short=0):
    from hybridgl_amd import _lib
    lib = _lib.load()
    keep = []
    recs = (_lib.HglGroupRef * len(refs))()
    for i, (q, o) in enumerate(zip(refs, outs)):
        arr = pack(q, keep)
        masks = q["masks"].view(torch.uint8)
        _, H, W = masks.shape
        keep += [arr, masks]
        recs[i] = _lib.HglGroupRef(q["hybrid"].data_ptr(), q["text"].data_ptr(), q["text"].shape[0], q["boxes"].data_ptr(), masks.data_ptr(),
                                   q["hybrid"].shape[0], H, W, arr, len(q["sentences"]), k1[i], q["k2"], o.idx.data_ptr(), o.iu.data_ptr(),
                                   o.scores[0].data_ptr(), o.scores[1].data_ptr(), o.scores[2].data_ptr())
    need = lib.hgl_score_group_workspace_bytes(recs, len(refs), E)
    ws = torch.empty(need, dtype=torch.uint8, device=refs[0]["hybrid"].device)
    rc = lib.hgl_score_group(recs, len(refs), E, LOGIT_SCALE, R_MIX, ALPHA, cum.data_ptr(), ws.data_ptr(), need - short,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def broken(q, j, **fields):
    """a copy of the ref whose sentence j has the given fields replaced"""
    sent = [dict(t) for t in q["sentences"]]
    sent[j].update(fields)
    return dict(q, sentences=sent)


BAD = {
    "text row out of range": lambda q: (broken(q, 2, sentence_row=q["text"].shape[0]), {}, HGL_EINVAL),
    "other rows past T": lambda q: (broken(q, 2, other_row0=q["text"].shape[0] - 1, n_other=2), {}, HGL_EINVAL),
    "bad dirflag": lambda q: (broken(q, 2, dirflag=4), {}, HGL_EINVAL),
    "k1 = 0": lambda q: (q, dict(k1=0), HGL_EINVAL),
    "workspace one byte short": lambda q: (q, dict(short=1), HGL_EWORKSPACE),
}


@pytest.mark.parametrize("case", list(BAD))
def test_error_paths_return_their_code_and_write_nothing(cuda, world, case):
    """HGL_EINVAL for a bad sentence record or k1, HGL_EWORKSPACE for a short workspace, from both entries; every check comes
    before the first launch: outputs and accumulators keep what they held"""
    from hybridgl_amd import _lib, ops
    refs, want = world
    good, q0 = refs[2], refs[1]
    q, kw, code = BAD[case](q0)
    cum = torch.full((4,), 5, dtype=torch.int64, device=cuda)
    out = Outputs(q, cuda)
    assert call_score_ref(q, out, cum, **kw) == code
    assert out.untouched() and bool((cum == 5).all())
    assert _lib.load().hgl_last_error().decode().startswith("score_ref: ")
    # the group entry: the bad ref behind a good one
    outs = [Outputs(good, cuda), Outputs(q, cuda)]
    gkw = dict(k1=(K1, kw["k1"])) if "k1" in kw else kw
    assert call_score_group([good, q], outs, cum, **gkw) == code
    assert all(o.untouched() for o in outs) and bool((cum == 5).all())
    msg = _lib.load().hgl_last_error().decode()
    assert msg.startswith("score_group: ") and (code == HGL_EWORKSPACE or "ref 1" in msg)
    # ... and through ops, as an exception that carries the code (ops sizes the workspace itself and maps an unknown
    # direction word to "none": those two cases exist at the C entry only)
    if case not in ("workspace one byte short", "bad dirflag"):
        bad = dict(q, **kw)
        with pytest.raises(_lib.HybridGLError, match=rf"code {code}"):
            ops.score_ref(bad["hybrid"], bad["text"], bad["boxes"], bad["masks"], bad["sentences"], LOGIT_SCALE, R_MIX, bad["k1"], bad["k2"],
                          ALPHA)
        with pytest.raises(_lib.HybridGLError, match=rf"code {code}"):
            ops.score_group([good, bad], LOGIT_SCALE, R_MIX, ALPHA)
    # the same operands, unbroken, pass through the same helpers
    out = Outputs(q0, cuda)
    assert call_score_ref(q0, out, cum) == 0
    assert_rows((out.idx, out.iu, *out.scores), want[1], "unbroken ref")


# ---- the IoU entries against a numpy count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,start", [(12707, 1), (4096, 0)], ids=["12707 bytes, unaligned", "4096 bytes, aligned"])
def test_iou_entries_equal_numpy_count(cuda, n, start):
    from hybridgl_amd import ops
    rng = np.random.default_rng(n)
    vals = np.array([0, 0, 1, 1, 2, 255], dtype=np.uint8)        # a byte counts when it is not zero
    planes = vals[rng.integers(0, len(vals), (3, n))]
    gt = vals[rng.integers(0, len(vals), n)]
    # planes that begin `start` bytes into an allocation (allocations are 256-byte aligned)
    mbuf = torch.zeros(start + 3 * n, dtype=torch.uint8, device=cuda)
    gbuf = torch.zeros(start + n, dtype=torch.uint8, device=cuda)
    masks, g = mbuf[start:].view(3, n), gbuf[start:]
    masks.copy_(torch.from_numpy(planes))
    g.copy_(torch.from_numpy(gt))
    assert masks.data_ptr() % 16 == start % 16 and g.data_ptr() % 16 == start % 16
    idx = torch.tensor([2, 1], dtype=torch.int32, device=cuda)
    for which, row in ((0, 2), (1, 1)):
        a, b = planes[row] != 0, gt != 0
        count = [int((a & b).sum()), int((a | b).sum())]
        assert ops.iou_select(masks, idx, which, g).tolist() == count
        assert ops.iou_counts(masks[row], g).tolist() == count
