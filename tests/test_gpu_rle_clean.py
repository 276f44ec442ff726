"""hgl_rle_clean_device (csrc/rle_clean.hip) on the GPU: remove_small_regions on encoded sets.  Everything is integers, so
every comparison is equality, bit for bit: ops.rle_remove_small_regions into a fenced buffer pre-filled with a pattern against
the numpy contract (tests/rle_clean_cases.py: host codec -> flood fill holes -> flood fill islands -> host encode -> box)
written into a buffer filled the same way -- so a word the call must not write is a word that kept its fill -- over every
pattern of the connected-component case list and its transpose, in modes holes, islands and both; then against the device's own
pixel path (sam.remove_small_regions / remove_small_regions_boxes on the decoded masks, ops.rle_encode); then the corners of
the contract: images of many sizes and one without an entry in one call, form-1 inputs, entries of code 1 and 2, output forms
0 / 1 / 2, the segment limit, thresholds 0 and 1, zero-length runs, two calls."""
import numpy as np
import pytest
import torch

from hybridgl_amd import ops, sam

import rle_clean_cases as RC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 64


def pack(entries, sw, form=0):
    """host (slots [S,sw] uint32, table [S,4] int32) of bool masks: form 0 = counts, form 1 = the bit plane"""
    S = len(entries)
    slots = np.full((S, sw), 0xA5A5A5A5, np.uint32)      # junk behind what the form defines: nobody may read it
    table = np.zeros((S, 4), np.int32)
    for i, m in enumerate(entries):
        c = RC.counts_of(m)
        w = c if form == 0 else RC.plane_of(m)
        assert len(w) <= sw
        slots[i, :len(w)] = w
        table[i] = (len(c), form, 0, 0)
    return slots, table


def call(slots, table, sizes, counts, thresh, mode, dev, osw, seg_cap=None):
    """ops.rle_remove_small_regions into the middle of a poisoned buffer -> (flat int32 host copy of the S*(12+osw) words, the
    guards kept their fill)"""
    S = slots.shape[0]
    n = S * (12 + osw)
    big = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device=dev)
    d_slots = torch.from_numpy(slots.view(np.int32)).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    ops.rle_remove_small_regions(d_slots, d_table, sizes, counts, thresh, mode, seg_cap=seg_cap, slot_words=osw, out=big[GUARD:GUARD + n])
    host = big.cpu().numpy()
    assert (d_slots.cpu().numpy() == slots.view(np.int32)).all() and (d_table.cpu().numpy() == table).all()      # the inputs stand
    return host[GUARD:GUARD + n].copy(), bool((host[:GUARD] == POISON).all() and (host[GUARD + n:] == POISON).all())


def statement(wants, osw):
    """the contract's buffer: table | slots | boxes | result over POISON"""
    S = len(wants)
    flat = np.full(S * (12 + osw), POISON, np.int32)
    slots, table = ops.rle_split(flat, S, osw)
    boxes, result = flat[S * (4 + osw):S * (8 + osw)].reshape(S, 4), flat[S * (8 + osw):].reshape(S, 4)
    for i, w in enumerate(wants):
        if w["mask"] is None:
            table[i], boxes[i], result[i] = (0, 3, 0, 0), (0, 0, 0, 0), w["result"]
            continue
        row, words = RC.encoded(w["mask"], osw)
        table[i], boxes[i], result[i] = row, w["box"], w["result"]
        slots[i, :len(words)] = words.view(np.int32)
    return flat


def groups():
    """{threshold: {shape: [index into RC.pairs()]}}: one call per threshold, one image per shape"""
    out = {}
    for i, (_, m, t) in enumerate(RC.pairs()):
        out.setdefault(t, {}).setdefault(m.shape, []).append(i)
    return out


@pytest.mark.parametrize("mode", ["holes", "islands", "both"])
def test_the_case_list_against_the_numpy_contract(cuda, mode):
    pairs, wants = RC.pairs(), RC.wants(mode)
    seen = set()
    for t, by_shape in sorted(groups().items()):
        shapes = sorted(by_shape)
        sizes = shapes[:1] + [(5, 5)] + shapes[1:]      # an image that owns no entry, second in the list
        counts = [len(by_shape[shapes[0]]), 0] + [len(by_shape[s]) for s in shapes[1:]]
        idx = [i for s in shapes for i in by_shape[s]]
        masks = [pairs[i][1] for i in idx]
        sw = max(len(RC.counts_of(m)) for m in masks)
        osw = max((m.size + 31) // 32 for m in masks)      # every entry's plane fits: forms 0 and 1 only
        slots, table = pack(masks, sw)
        got, fences = call(slots, table, sizes, counts, t, mode, cuda, osw)
        want = statement([wants[i] for i in idx], osw)
        assert fences, t
        if not np.array_equal(got, want):
            S = len(idx)
            gs, gt = ops.rle_split(got, S, osw)
            ws, wt = ops.rle_split(want, S, osw)
            for k, i in enumerate(idx):
                assert np.array_equal(gt[k], wt[k]), (pairs[i][0], "table", gt[k], wt[k])
                assert np.array_equal(got[S * (4 + osw):].reshape(2, S, 4)[:, k], want[S * (4 + osw):].reshape(2, S, 4)[:, k]), (pairs[i][0], "box / result")
                assert np.array_equal(gs[k], ws[k]), (pairs[i][0], "slot")
        seen |= {int(f) for f in ops.rle_split(want, len(idx), osw)[1][:, 1]}
    assert seen == {0, 1}


@pytest.mark.parametrize("mode", ["holes", "islands", "both"])
def test_the_case_list_against_the_device_pixel_path(cuda, mode):
    pairs = RC.pairs()
    for t, by_shape in sorted(groups().items()):
        for (H, W), idx in sorted(by_shape.items()):
            masks = np.stack([pairs[i][1] for i in idx])
            osw = ops.rle_slot_words(H, W)
            slots, table = pack(list(masks), max(len(RC.counts_of(m)) for m in masks))
            got, fences = call(slots, table, [(H, W)], [len(idx)], t, mode, cuda, osw)
            S = len(idx)
            gs, gt = ops.rle_split(got, S, osw)
            gbox, gres = got[S * (4 + osw):].reshape(2, S, 4)
            # decode -> clean (twice) -> encode, on bytes
            cur = torch.from_numpy(masks.astype(np.uint8)).to(cuda)
            changed = torch.zeros(S, dtype=torch.int32, device=cuda)
            if mode != "islands":
                cur, ch = sam.remove_small_regions(cur, t, "holes")
                changed |= ch.to(torch.int32)
            if mode != "holes":
                cur, ch, _ = sam.remove_small_regions_boxes(cur, t, "islands")
                changed |= ch.to(torch.int32) << 1
            boxes = sam.mask_boxes(cur)
            rs, rt = ops.rle_encode(cur, slot_words=osw)
            rs, rt = rs.cpu().numpy(), rt.cpu().numpy()
            assert fences and np.array_equal(gt, rt), (t, H, W)
            assert np.array_equal(gbox, boxes.cpu().numpy()), (t, H, W)
            assert np.array_equal(gres[:, 2], changed.cpu().numpy()) and np.array_equal(gres[:, 1], rt[:, 2]), (t, H, W)
            assert np.array_equal(gres[:, 3], masks.reshape(S, -1).sum(axis=1)) and (gres[:, 0] == 0).all(), (t, H, W)
            for k in range(S):
                n = int(rt[k, 0]) if rt[k, 1] == 0 else osw
                assert np.array_equal(gs[k, :n], rs[k, :n]) and (gs[k, n:] == POISON).all(), (t, H, W, pairs[idx[k]][0])


def some(step, shapes=((65, 33), (33, 65), (129, 65), (37, 130), (2, 37))):
    """a sample of the case list at a few shapes: [(mask, threshold)] per shape"""
    out = {}
    for _, m, t in RC.pairs()[::step]:
        if m.shape in shapes:
            out.setdefault(m.shape, []).append((m, t))
    return out


def test_form_1_inputs_and_output_forms_0_1_2(cuda):
    seen = set()
    for (H, W), items in some(3).items():
        plane = (H * W + 31) // 32
        for t in sorted({t for _, t in items}):
            masks = [m for m, tt in items if tt == t]
            wants = [RC.clean(m, t, "both") for m in masks]
            slots, table = pack(masks, plane + 3, form=1)
            for osw in (plane, plane - 1, 9, 1, 0):      # counts or plane; counts or nothing
                got, fences = call(slots, table, [(H, W)], [len(masks)], t, "both", cuda, osw)
                want = statement(wants, osw)
                assert fences and np.array_equal(got, want), (H, W, t, osw)
                seen |= {int(f) for f in ops.rle_split(want, len(masks), osw)[1][:, 1]}
    assert seen == {0, 1, 2}


def test_codes_1_2_and_3_beside_entries_that_are_cleaned(cuda):
    H, W = 65, 33
    yy, xx = np.mgrid[:H, :W]
    checker = (xx + yy) % 2 == 0                                  # 33 * 33 segments of either colour
    blob = (abs(yy - 30) < 12) & (abs(xx - 16) < 9)
    blob[30, 16] = False                                          # a hole of one pixel
    blob[2, 2] = True                                             # an island of one
    masks = [blob, checker, blob, checker, blob]
    slots, table = pack(masks, 2200)
    # entry 2: counts that stop short of H*W (code 1: clipped, the rest background); entry 3: a row that describes no mask (code 2)
    short = RC.counts_of(blob)[:-1]
    slots[2, :len(short)] = short
    table[2] = (len(short), 0, 0, 0)
    table[3] = (2201, 0, 0, 0)
    cap = RC.segments(blob, True) + 5
    assert RC.segments(checker, False) > cap > max(RC.segments(blob, False), RC.segments(RC.mask_of(short, H, W)[0], True))
    for mode in ("holes", "islands", "both"):
        wants = [RC.clean(blob, 20, mode, seg_cap=cap), RC.clean(checker, 20, mode, seg_cap=cap),
                 RC.clean(RC.mask_of(short, H, W)[0], 20, mode, seg_cap=cap), dict(RC.REFUSED, result=(2, 0, 0, 0)),
                 RC.clean(blob, 20, mode, seg_cap=cap)]
        wants[2]["result"] = (1,) + tuple(wants[2]["result"][1:])
        assert [w["result"][0] for w in wants] == [0, 3, 1, 2, 0] and wants[0]["result"][2] == ops.CLEAN_MODES[mode]
        got, fences = call(slots, table, [(H, W)], [5], 20, mode, cuda, 80, seg_cap=cap)
        assert fences and np.array_equal(got, statement(wants, 80)), mode
        # with room for every segment nothing is refused
        got, _ = call(slots, table, [(H, W)], [5], 20, mode, cuda, 80)
        assert got[5 * (8 + 80):].reshape(5, 4)[:, 0].tolist() == [0, 0, 1, 2, 0]


def test_identity_thresholds_canonical_runs_and_two_calls(cuda):
    by_shape = some(5)
    shapes = sorted(by_shape)
    masks = [m for s in shapes for m, _ in by_shape[s]]
    counts = [len(by_shape[s]) for s in shapes]
    sw = max(len(RC.counts_of(m)) for m in masks) + 4
    osw = max((m.size + 31) // 32 for m in masks)
    slots, table = pack(masks, sw)
    # zero-length runs: the first foreground run of every entry that has one is split in two by an empty background run
    for i, m in enumerate(masks):
        c = RC.counts_of(m).tolist()
        if len(c) >= 2 and c[1] >= 2:
            c = [c[0], 1, 0, c[1] - 1] + c[2:]
            slots[i, :len(c)] = c
            table[i, 0] = len(c)
    assert (table[:, 0] > [len(RC.counts_of(m)) for m in masks]).any()
    for t in (0, 1):
        for mode in ("holes", "islands", "both"):
            got, fences = call(slots, table, shapes, counts, t, mode, cuda, osw)
            want = statement([dict(mask=m, box=RC.box_of(m), result=(0, int(m.sum()), 0, int(m.sum()))) for m in masks], osw)
            assert fences and np.array_equal(got, want), (t, mode)
    a, _ = call(slots, table, shapes, counts, 20, "both", cuda, osw)
    b, _ = call(slots, table, shapes, counts, 20, "both", cuda, osw)
    assert np.array_equal(a, b)
    assert np.array_equal(a, statement([RC.clean(m, 20, "both") for m in masks], osw))


def test_the_wrappers(cuda):
    H, W = 37, 130
    items = some(4, ((H, W),))[(H, W)]
    rles = [{"size": [H, W], "counts": RC.counts_of(m).tolist()} for m, _ in items]
    rles[1] = sam.coco_encode_rle(rles[1])
    for mode in ("holes", "islands", "both"):
        out, changed = sam.remove_small_regions_rles(rles, 20, mode)
        for k, ((m, _), r, c) in enumerate(zip(items, out, changed)):
            w = RC.clean(m, 20, mode)
            assert c == bool(w["result"][2]) and r["size"] == [H, W] and isinstance(r["counts"], str if k == 1 else list)
            assert sam.rle_counts(r).tolist() == RC.counts_of(w["mask"]).tolist(), (mode, k)
    assert sam.remove_small_regions_rles([], 20, "both") == ([], [])
    with pytest.raises(ValueError):
        sam.remove_small_regions_rles(rles[:1] + [{"size": [H, W + 1], "counts": [H * (W + 1)]}], 20, "both")
    with pytest.raises(ValueError):
        sam.remove_small_regions_rles([{"size": [H, W], "counts": [5]}], 20, "both")      # does not sum to H*W
    s, t = ops.rle_pack([r["counts"] for r in rles[:1]], H, W, device=cuda)
    with pytest.raises(ValueError):
        ops.rle_remove_small_regions(s, t, [(H, W)], [1], 20, "neither")
    with pytest.raises(ValueError):
        ops.rle_remove_small_regions(s, t, [(H, W)], [2], 20)
    e = ops.rle_remove_small_regions(s[:0], t[:0], [(H, W)], [0], 20)
    assert [tuple(x.shape) for x in e] == [(0, s.shape[1]), (0, 4), (0, 4), (0, 4)]


def test_either_side_of_the_4096_segments_the_kernel_keeps_in_lds(cuda):
    """an entry of at most 4096 segments of the pass's colour runs its union-find in LDS, a larger one in the workspace"""
    yy, xx = np.mgrid[:128, :65]
    rows = yy % 2 == 0
    a = rows[:, :64].copy()                     # 64 x 64 = 4096 segments of either colour; every row an island of 64
    b = rows | (xx == 64)                       # 4097 foreground segments, joined by the last column; 4096 of the background
    c = ~b                                      # the same as holes: 4097 background segments, 4096 of the foreground
    d = rows.copy()
    d[::4, 64] = False                          # 4096 + 32 foreground segments, islands of 65 and of 64
    assert [RC.segments(m, False) for m in (a, b, c, d)] == [4096, 4097, 4096, 4096 + 32] and RC.segments(c, True) == 4097
    for t in (65, 70, 5000):
        for mode in ("holes", "islands", "both"):
            masks = [a, b, c, d, a]
            sw = max(len(RC.counts_of(m)) for m in masks)
            slots, table = pack(masks, sw)
            got, fences = call(slots, table, [(128, 64), (128, 65), (128, 64)], [1, 3, 1], t, mode, cuda, 300)
            want = statement([RC.clean(m, t, mode) for m in masks], 300)
            assert fences and np.array_equal(got, want), (t, mode)
