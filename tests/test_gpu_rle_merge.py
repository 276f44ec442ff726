"""hgl_rle_merge_device (csrc/rle.hip) through ops.rle_merge: new masks voted out of encoded masks.  Integer and byte equality
throughout: the expected value is always ops.rle_encode of the dense numpy vote, uploaded, at the same slot_words -- table rows
equal, slot words equal as far as the form defines them, the guard words beyond untouched.  Shapes with padding bits, exactly one
word, form-1 words that span columns, a tall narrow image, one pixel, one row, one column; k from 0 to 300 under every rule name,
(0, 0) and (0, k); repeated members against the weighted count; source forms 0, 1 and mixed; output forms 0, 1 and 2; sources of
code 1 and 2; every refusal; groups against per-image calls; every HGL_EINVAL before a launch; the reference's rleMerge
(tests/golden/rle_merge_fuzz.npz)."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops

import rle_merge_cases as MC

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SHAPES = [(70, 37), (64, 64), (3, 50), (129, 5), (1, 1), (1, 40), (40, 1)]
KS = [0, 1, 2, 3, 7, 16, 255, 300]


def seeded(n, H, W, seed):
    """n masks: rectangles (few runs: form 0 at the default slot size) and noise (form 1), an empty and a full one among them"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        if i % 2 == 0:
            y0, y1 = sorted(int(v) for v in rng.integers(0, H + 1, 2))
            x0, x1 = sorted(int(v) for v in rng.integers(0, W + 1, 2))
            out[i, y0:y1 + 1, x0:x1 + 1] = 1
        else:
            out[i] = (rng.random((H, W)) < (0.25, 0.5, 0.85)[i % 3]).astype(np.uint8)
    if n > 4:
        out[3] = 0
        out[4] = 1
    return out


def encode(masks, dev, slot_words=None):
    return ops.rle_encode(torch.from_numpy(np.ascontiguousarray(masks)).to(dev), slot_words=slot_words)


def defined_words(row, H, W):
    """how many words of a slot its table row defines"""
    return int(row[0]) if row[1] == 0 else ((H * W + 31) // 32 if row[1] == 1 else 0)


def check_entries(got, want_masks, hw, slot_words, dev, codes=None, ks=None):
    """got = (slots, table, status) of a call over a sentinel-filled buffer; want_masks[s]: the dense mask, or None for a refusal"""
    slots, table, status = (t.cpu().numpy() for t in got)
    slots = slots.view(np.uint32)
    for s, want in enumerate(want_masks):
        H, W = hw[s]
        if want is None:
            assert table[s].tolist() == [0, 3, 0, 0] and status[s, 0] == 2 and status[s, 2:].tolist() == [0, 0], (s, table[s], status[s])
            assert (slots[s] == SENTINEL).all(), s
            continue
        es, et = encode(want[None], dev, slot_words)
        es, et = es.cpu().numpy().view(np.uint32), et.cpu().numpy()
        assert table[s].tolist() == et[0].tolist(), (s, table[s], et[0])
        n = defined_words(et[0], H, W)
        assert (slots[s, :n] == es[0, :n]).all(), s
        assert (slots[s, n:] == SENTINEL).all(), s
        assert status[s, 0] == (codes[s] if codes else 0) and status[s, 2:].tolist() == [0, 0], (s, status[s])
    if ks is not None:
        assert status[:, 1].tolist() == list(ks)


def merge(src, sizes, counts_src, members, bounds, counts_out, slot_words, dev, offsets=None):
    S = int(sum(counts_out))
    out = torch.full((S * (8 + slot_words),), SENTINEL, dtype=torch.int32, device=dev)
    return ops.rle_merge(src[0], src[1], sizes, counts_src, members, offsets, bounds, counts_out, slot_words=slot_words, out=out)


def rules_for(k):
    names = ["union", "intersect", "majority", "at_least:2", "exactly:1", "exactly:2", "at_least:0"]
    return [ops.rle_merge_rule(n, k) for n in names] + [(0, 0), (0, k)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_every_k_and_rule_against_the_dense_vote(cuda, H, W):
    masks = seeded(7, H, W, 100 + H * W)
    src = encode(masks, cuda)      # mixed forms where the noise has more runs than ceil(H*W/32)
    sw = ops.rle_slot_words(H, W)
    rng = np.random.default_rng(H + W)
    for k in KS:
        rules = rules_for(k)
        mem = [rng.integers(0, 7, k).tolist() for _ in rules]      # k <= 7 may repeat, k > 7 must: the weighted count
        got = merge(src, [(H, W)], [7], mem, rules, [len(rules)], sw, cuda)
        want = [MC.vote(masks, m, lo, hi) for m, (lo, hi) in zip(mem, rules)]
        check_entries(got, want, [(H, W)] * len(rules), sw, cuda, ks=[k] * len(rules))
        if k == 0:
            assert [int(w.sum()) for w in want] == [0, H * W, 0, 0, 0, 0, H * W, H * W, H * W]


def test_source_forms_and_output_forms(cuda):
    H, W = 70, 37
    yy, xx = np.mgrid[0:H, 0:W]
    checker = ((yy + xx) % 2).astype(np.uint8)
    masks = np.stack([checker, 1 - checker, seeded(2, H, W, 5)[1], seeded(1, H, W, 6)[0]])
    mem, rules = [[0], [0, 1], [0, 2], [3, 3, 2], [1, 3]], [(1, 1), (2, 2), (1, 2), (2, 3), (0, 0)]
    want = [MC.vote(masks, m, lo, hi) for m, (lo, hi) in zip(mem, rules)]
    plane = ops.rle_slot_words(H, W)
    forms = {}
    for name, src_sw in (("form 0", H * W + 1), ("mixed", plane), ("form 1", plane)):
        use = masks if name != "form 1" else masks[:3]      # the rectangle is form 0 at any slot size
        src = encode(use, cuda, src_sw)
        forms[name] = sorted(set(src[1][:, 1].tolist()))
        m2, r2, w2 = (mem, rules, want) if name != "form 1" else (mem[:3], rules[:3], want[:3])
        for out_sw, out_forms in ((H * W + 1, {0}), (plane, {0, 1}), (3, {0, 2}), (0, {2})):
            got = merge(src, [(H, W)], [len(use)], m2, r2, [len(m2)], out_sw, cuda)
            check_entries(got, w2, [(H, W)] * len(m2), out_sw, cuda)
            assert set(got[1][:, 1].tolist()) == out_forms, (name, out_sw)
    assert forms == {"form 0": [0], "mixed": [0, 1], "form 1": [1]}
    # 3 x 50: the 32-bit words of a form-1 slot span columns, on the way in and on the way out
    H, W = 3, 50
    masks = np.stack([((np.mgrid[0:H, 0:W][0] + np.mgrid[0:H, 0:W][1]) % 2).astype(np.uint8), seeded(2, H, W, 9)[1]])
    src = encode(masks, cuda)
    assert src[1][:, 1].tolist() == [1, 1]
    got = merge(src, [(H, W)], [2], [[0], [0, 1], [0, 1]], [(1, 1), (1, 2), (1, 1)], [3], ops.rle_slot_words(H, W), cuda)
    check_entries(got, [masks[0], masks[0] | masks[1], masks[0] ^ masks[1]], [(H, W)] * 3, ops.rle_slot_words(H, W), cuda)
    assert got[1][0, 1].item() == 1


def test_sources_of_code_1_and_2(cuda):
    H, W = 70, 37
    masks = seeded(3, H, W, 21)
    lists = [MC.counts_of(m).tolist() for m in masks]
    short = [100, 50, 7, 900]                       # sums to less than H*W: clipped, pixels past the last run are 0
    long_ = [5, 0xFFFFFFFF, 5, 9]                   # a run that passes H*W: clipped there
    slots, table = ops.rle_pack(lists + [short, long_], H, W, slot_words=2600, device=cuda)
    dec, st = ops.rle_decode(slots, table, H, W)
    assert st[:, 0].tolist() == [0, 0, 0, 1, 1]
    dense = dec.cpu().numpy()
    assert (dense[:3] == masks).all()
    table = table.clone()
    slots2 = torch.cat([slots, slots[:2]])
    table2 = torch.cat([table, torch.tensor([[3, 2, 0, 0], [2601, 0, 0, 0]], dtype=torch.int32, device=cuda)])      # two entries of code 2
    dense = np.concatenate([dense, np.zeros((2, H, W), np.uint8)])
    mem = [[0, 1], [0, 3], [3, 4, 2], [0, 5], [6], [1, 6, 2], [4, 4]]
    rules = [(1, 2), (1, 2), (2, 3), (1, 2), (1, 1), (1, 3), (2, 2)]
    want = [MC.vote(dense, m, lo, hi) if not (set(m) & {5, 6}) else None for m, (lo, hi) in zip(mem, rules)]
    got = merge((slots2, table2), [(H, W)], [7], mem, rules, [7], 90, cuda)
    check_entries(got, want, [(H, W)] * 7, 90, cuda, codes=[0, 1, 1, 2, 2, 2, 1], ks=[2, 2, 3, 2, 1, 3, 2])


def test_every_refusal_that_gives_code_2(cuda):
    sizes, cs, co = [(70, 37), (3, 50)], [3, 2], [9, 2]
    a, b = seeded(3, 70, 37, 31), seeded(2, 3, 50, 32)
    sa, sb = encode(a, cuda, 100), encode(b, cuda, 100)
    src = (torch.cat([sa[0], sb[0]]), torch.cat([sa[1], sb[1]]))
    # entries 0 .. 8 belong to image 0 (sources 0 .. 2), 9 and 10 to image 1 (sources 3, 4)
    # e0: 0,1   e1: 2,3 (3 is image 1's)   e2: -1   e3: 5 (beyond Ssrc)   e4: 0,1,2   e5 .. e8: none   e9: 3,4   e10: 2 (image 0's)
    members = [0, 1, 2, 3, -1, 5, 0, 1, 2, 3, 4, 2]
    offsets = [0, 2, 4, 5, 6, 9, 9, 9, 9, 9, 11, 12]
    bounds = [(1, 2), (1, 2), (1, 1), (1, 1), (2, 3), (-1, 0), (2, 1), (0, 0), (0, 5), (1, 2), (1, 1)]      # e5: lo < 0, e6: lo > hi
    got = merge(src, sizes, cs, members, bounds, co, 100, cuda, offsets=offsets)
    full = np.ones((70, 37), np.uint8)
    want = [a[0] | a[1], None, None, None, MC.vote(a, [0, 1, 2], 2, 3), None, None, full, full, b[0] | b[1], None]
    check_entries(got, want, [(70, 37)] * 9 + [(3, 50)] * 2, 100, cuda, ks=[2, 2, 1, 1, 3, 0, 0, 0, 0, 2, 1])
    # offsets that step back or leave [0, M]: the entry is refused, with k reported as 0; its neighbours are served
    for offs, bad in (([0, 3, 2, 5], [1]), ([0, 2, 6, 5], [1, 2]), ([-1, 2, 4, 5], [0]), ([0, 2, 4, 7], [2])):
        got = merge(sa, [(70, 37)], [3], [0, 1, 2, 0, 1], [(1, 9)] * 3, [3], 100, cuda, offsets=offs)
        want, ks = [], []
        for s in range(3):
            ok = s not in bad
            want.append(MC.vote(a, [0, 1, 2, 0, 1][offs[s]:offs[s + 1]], 1, 9) if ok else None)
            ks.append(offs[s + 1] - offs[s] if ok else 0)
        check_entries(got, want, [(70, 37)] * 3, 100, cuda, ks=ks)
    # k > 65535: 1 x 1 masks, one member repeated
    one = encode(np.ones((1, 1, 1), np.uint8), cuda, 2)
    mem = torch.zeros(65536 + 65535, dtype=torch.int32, device=cuda)
    got = merge(one, [(1, 1)], [1], mem, [(65535, 65535), (1, 70000)], [2], 2, cuda, offsets=[0, 65535, 65535 + 65536])
    check_entries(got, [np.ones((1, 1), np.uint8), None], [(1, 1)] * 2, 2, cuda, ks=[65535, 65536])


def group_case(seed=41):
    sizes = [(70, 37), (64, 64), (3, 50), (129, 5)]
    cs, co = [3, 0, 5, 2], [2, 1, 0, 3]      # image 1 owns no source, image 2 no output
    masks = [seeded(n, H, W, seed + g) for g, ((H, W), n) in enumerate(zip(sizes, cs))]
    first = np.concatenate([[0], np.cumsum(cs)])
    local = [[[0, 1, 2], [2, 2, 1]], [[]], [], [[0, 1], [1], [0, 0, 1]]]      # members within the image
    rules = [[(2, 3), (1, 2)], [(0, 0)], [], [(1, 2), (0, 0), (3, 3)]]
    return sizes, cs, co, masks, first, local, rules


def test_a_group_against_per_image_calls_and_twice(cuda):
    sizes, cs, co, masks, first, local, rules = group_case()
    sw = 120
    enc = [encode(m, cuda, sw) for m in masks if len(m)]
    src = (torch.cat([e[0] for e in enc]), torch.cat([e[1] for e in enc]))
    members = [[first[g] + m for m in entry] for g in range(4) for entry in local[g]]
    bounds = [r for g in range(4) for r in rules[g]]
    got = merge(src, sizes, cs, members, bounds, co, sw, cuda)
    again = merge(src, sizes, cs, members, bounds, co, sw, cuda)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    want, hw = [], []
    for g, (H, W) in enumerate(sizes):
        for entry, (lo, hi) in zip(local[g], rules[g]):
            want.append(MC.vote(masks[g], entry, lo, hi) if len(masks[g]) else np.full((H, W), int(lo == 0), np.uint8))
            hw.append((H, W))
    check_entries(got, want, hw, sw, cuda, ks=[3, 3, 0, 2, 1, 3])
    # every image alone: the same bytes, guard words included
    s0 = 0
    for g, (H, W) in enumerate(sizes):
        if co[g] == 0:
            continue
        lo_, hi_ = int(first[g]), int(first[g + 1])
        alone = merge((src[0][lo_:hi_], src[1][lo_:hi_]), [(H, W)], [cs[g]], local[g], rules[g], [co[g]], sw, cuda)
        for x, y in zip(got, alone):
            assert torch.equal(x[s0:s0 + co[g]], y), g
        s0 += co[g]


def test_64_images(cuda):
    sizes = [(1 + (5 * g) % 71, 1 + (3 * g) % 67) for g in range(64)]
    masks = [seeded(2, H, W, 500 + g) for g, (H, W) in enumerate(sizes)]
    sw = 160
    enc = [encode(m, cuda, sw) for m in masks]
    src = (torch.cat([e[0] for e in enc]), torch.cat([e[1] for e in enc]))
    members = [[2 * g, 2 * g + 1] for g in range(64)]
    bounds = [[(1, 2), (2, 2), (1, 1), (0, 0)][g % 4] for g in range(64)]
    got = merge(src, sizes, [2] * 64, members, bounds, [1] * 64, sw, cuda)
    want = [MC.vote(masks[g], [0, 1], *bounds[g]) for g in range(64)]
    check_entries(got, want, sizes, sw, cuda, ks=[2] * 64)


def test_every_einval_leaves_the_outputs_untouched(cuda):
    lib = _lib.load()
    H, W, sw = 70, 37, 200
    src = encode(seeded(3, H, W, 61), cuda, sw)
    S = 2
    out = torch.full((S * (8 + sw),), SENTINEL, dtype=torch.int32, device=cuda)
    before = out.clone()
    mem = torch.tensor([0, 2, 2], dtype=torch.int32, device=cuda)      # two rectangles: form 0
    off = torch.tensor([0, 2, 3], dtype=torch.int32, device=cuda)
    bnd = torch.tensor([[1, 2], [1, 1]], dtype=torch.int32, device=cuda)
    good = np.asarray([[H, W, 0, 0]], dtype=np.int64)
    need = lib.hgl_rle_merge_workspace_bytes(good.ctypes.data, 1, 3, sw, S, 3)
    assert need == MC.workspace_bytes(good.tolist(), 3, sw, S, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    base, stream = out.data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(images=good, G=1, Ssrc=3, S=S, M=3, sw_src=sw, sw_out=sw, memp=mem.data_ptr(), offp=off.data_ptr(), bndp=bnd.data_ptr(),
             slotp=base + 16 * S, tablep=base, statp=base + 4 * S * (4 + sw), wsp=ws.data_ptr(), ws_bytes=need, srcp=src[0].data_ptr(),
             imagesp=None):
        return lib.hgl_rle_merge_device(srcp, sw_src, src[1].data_ptr(), Ssrc, images.ctypes.data if imagesp is None else imagesp, G,
                                        memp, M, offp, bndp, slotp, sw_out, tablep, S, statp, wsp, ws_bytes, stream)

    def edit(col, v):
        im = good.copy()
        im[0, col] = v
        return im
    two = np.asarray([[H, W, 0, 0], [H, W, 2, 1]], dtype=np.int64)
    bad = {"G = 0": dict(G=0), "G = 65": dict(images=np.tile(good, (65, 1)), G=65), "H = 0": dict(images=edit(0, 0)),
           "W < 0": dict(images=edit(1, -1)), "H*W = 2^31": dict(images=edit(0, 1 << 31)), "first source not 0": dict(images=edit(2, 1)),
           "first output not 0": dict(images=edit(3, 1)), "source rows beyond Ssrc": dict(images=two, G=2, Ssrc=1),
           "output rows beyond S": dict(images=two, G=2, S=0), "Ssrc < 0": dict(Ssrc=-1), "S < 0": dict(S=-1), "M < 0": dict(M=-1),
           "slot_words_src < 0": dict(sw_src=-1), "slot_words < 0": dict(sw_out=-1), "no members": dict(memp=None),
           "no offsets": dict(offp=None), "no bounds": dict(bndp=None), "no slots": dict(slotp=None), "no table": dict(tablep=None),
           "no status": dict(statp=None), "no sources": dict(srcp=None), "no images": dict(imagesp=0)}
    for what, kw in bad.items():
        assert call(**kw) == -1, what      # HGL_EINVAL
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.hgl_last_error()      # HGL_EWORKSPACE
    assert call(wsp=None) == -3
    torch.cuda.synchronize()
    assert torch.equal(out, before)      # nothing was enqueued
    # S = 0 is a call without work: no workspace, no launch
    assert call(S=0, wsp=None, ws_bytes=0, offp=None, bndp=None, slotp=None, tablep=None, statp=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    assert call() == 0
    torch.cuda.synchronize()
    assert out[:4 * S].reshape(S, 4)[:, 1].tolist() == [0, 0] and not torch.equal(out, before)


def test_sam_merge_rles_is_mask_merge(cuda):
    """sam.merge_rles on uncompressed dicts and on COCO strings: the reference's counts, in the form of the inputs"""
    from hybridgl_amd import sam as hsam
    cases = MC.golden_cases()
    for H, W, masks, union, inter in cases[::7] + cases[-3:]:
        plain = [{"size": [H, W], "counts": MC.counts_of(m).tolist()} for m in masks]
        coco = [hsam.coco_encode_rle(r) for r in plain]
        for intersect, want in ((False, union), (True, inter)):
            assert hsam.merge_rles(plain, intersect) == {"size": [H, W], "counts": want.tolist()}
            assert hsam.merge_rles(coco, intersect) == hsam.coco_encode_rle({"size": [H, W], "counts": want.tolist()})
    with pytest.raises(ValueError):
        hsam.merge_rles([])
    with pytest.raises(ValueError, match="size"):
        hsam.merge_rles([{"size": [4, 4], "counts": [16]}, {"size": [4, 5], "counts": [20]}])


def test_the_references_rle_merge(cuda):
    """union and intersection equal rleMerge's counts on every case of the golden file: one call per shape"""
    cases = MC.golden_cases()
    for H, W in sorted({(c[0], c[1]) for c in cases}):
        mine = [c for c in cases if (c[0], c[1]) == (H, W)]
        masks = np.concatenate([c[2] for c in mine])
        src = encode(masks, cuda)
        members, bounds, want, at = [], [], [], 0
        for _, _, m, union, inter in mine:
            n = len(m)
            members += [list(range(at, at + n))] * 2
            bounds += [ops.rle_merge_rule("union", n), ops.rle_merge_rule("intersect", n)]
            want += [union, inter]
            at += n
        sw = H * W + 1
        slots, table, status = merge(src, [(H, W)], [len(masks)], members, bounds, [len(want)], sw, cuda)
        slots, table, status = slots.cpu().numpy().view(np.uint32), table.cpu().numpy(), status.cpu().numpy()
        assert (status[:, 0] == 0).all() and (table[:, 1] == 0).all()
        for s, counts in enumerate(want):
            assert table[s, 0] == len(counts) and slots[s, :len(counts)].tolist() == counts.tolist(), (H, W, s)
            assert table[s, 2] == int(counts[1::2].sum())
