"""hgl_rle_from_polygons_device (csrc/rle_poly.hip) on the GPU: polygons in, exactly what ops.rle_encode writes for the host
codec's mask out -- bit for bit, table, slots and the untouched words, for both rules, at every slot form, at the shapes where
a column-major bit stream can go wrong, on both sides of the LDS / workspace threshold, in every layout of a grouped call, with
refused entries between good ones, and composed with the decoder, the IoU and the matcher.  Every call is made twice and the
two results compared bit for bit.  The expected masks are refer_io.gt_mask_from_polygons' (tests/poly_cases.py)."""
import os
import re

import numpy as np
import pytest
import torch

import poly_cases as PC
from hybridgl_amd import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A


def lds_words():
    text = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle_group.h")).read()
    return int(re.search(r"constexpr\s+int\s+RLE_POLY_LDS_WORDS\s*=\s*(\d+)\s*;", text).group(1))


def rasterise(entries, sizes, counts, rule, slot_words=None, dev=None):
    """ops.rle_from_polygons into a sentinel-filled buffer, twice: the flat int32 buffer (table, slots, status) of the first
    call, asserted equal to the second's"""
    S = len(entries)
    sw = max(ops.rle_slot_words(H, W) for H, W in sizes) if slot_words is None else slot_words
    outs = []
    for _ in range(2):
        out = torch.full((S * (8 + sw),), SENTINEL, dtype=torch.int32, device=dev)
        ops.rle_from_polygons(entries, sizes, counts, rule=rule, slot_words=sw, device=dev, out=out)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    return outs[0], sw


def encoded(masks_per_image, sw, dev):
    """what ops.rle_encode writes for the expected masks at the same slot size into sentinel-filled buffers: (table [S,4],
    slots [S,sw]) of the whole call; masks_per_image: uint8 arrays [n,H,W] (n may be 0)"""
    tables, slots = [], []
    for m in masks_per_image:
        n = len(m)
        if n == 0:
            continue
        out = torch.full((n * (4 + sw),), SENTINEL, dtype=torch.int32, device=dev)
        s, t = ops.rle_encode(torch.from_numpy(np.ascontiguousarray(m)).to(dev), None, sw, out=out)
        tables.append(t)
        slots.append(s)
    return torch.cat(tables), torch.cat(slots)


def check_call(entries, sizes, counts, counts_images, areas, dev, slot_words=None):
    """both rules of one call against the encoder; counts_images: per image the count images [n,H,W] of its entries; areas:
    the host codec's area per entry.  Returns the tables of both rules on the host."""
    S = len(entries)
    tabs = []
    for rule in PC.RULES:
        flat, sw = rasterise(entries, sizes, counts, rule, slot_words, dev)
        want_t, want_s = encoded([PC.by_rule(c, rule) for c in counts_images], sw, dev)
        slots, table = ops.rle_split(flat, S, sw)
        status = flat[S * (4 + sw):].reshape(S, 4).cpu().numpy()
        assert torch.equal(table, want_t), (rule, np.argwhere((table != want_t).cpu().numpy())[:4])
        assert torch.equal(slots, want_s), (rule, np.argwhere((slots != want_s).cpu().numpy())[:4])
        assert np.array_equal(status, np.stack([np.zeros(S), np.asarray(areas), np.zeros(S), np.zeros(S)], 1).astype(np.int32)), rule
        tabs.append(table.cpu().numpy())
    return tabs


@pytest.fixture(scope="module")
def first_only():
    """[(count image, area)] of every case's first polygon alone"""
    return [PC.expected(H, W, polys[:1]) for H, W, polys in PC.cases()]


def test_all_cases_equal_the_encoder_of_the_host_codec(cuda, first_only):
    cases, full = PC.cases(), PC.expected_all()
    assert len(cases) == 448
    forms = set()
    for lo in range(0, len(cases), 64):
        chunk = range(lo, min(lo + 64, len(cases)))
        entries = [e for i in chunk for e in (cases[i][2], cases[i][2][:1])]
        sizes = [cases[i][:2] for i in chunk]
        images = [np.stack([full[i][0], first_only[i][0]]) for i in chunk]
        areas = [a for i in chunk for a in (full[i][1], first_only[i][1])]
        for t in check_call(entries, sizes, [2] * len(sizes), images, areas, cuda):
            forms |= set(t[:, 1].tolist())
    assert 0 in forms      # the other forms have a test of their own


def rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def test_forms(cuda):
    H, W = 64, 96
    comb = [rect(0, 6 * i + 1, W, 6 * i + 2) for i in range(10)] + [rect(10, 0, 12, H)]      # bars, and a post across them
    square = [rect(8, 8, 40, 40)]
    entries, sizes, counts = [square, comb, square], [(H, W)], [3]
    imgs = [np.stack([PC.expected(H, W, e)[0] for e in entries])]
    areas = [PC.expected(H, W, e)[1] for e in entries]
    plane = ops.rle_slot_words(H, W)
    t_once, t_any = check_call(entries, sizes, counts, imgs, areas, cuda, slot_words=plane)
    n_comb = int(t_once[1, 0])
    assert n_comb > plane and int(t_any[1, 0]) > plane      # many runs: the counts do not fit, the plane does
    assert t_once[:, 1].tolist() == [0, 1, 0] and t_any[:, 1].tolist() == [0, 1, 0]
    assert t_once[1, 2] != t_any[1, 2]      # the post crosses the bars: the rules differ
    small = 100
    assert small < plane and small < n_comb
    u_once, u_any = check_call(entries, sizes, counts, imgs, areas, cuda, slot_words=small)
    assert u_once[:, 1].tolist() == [0, 2, 0] and u_any[:, 1].tolist() == [0, 2, 0]
    # form 2: nothing written (check_call compared the sentinel words), counts and area still exact
    assert np.array_equal(u_once[:, [0, 2]], t_once[:, [0, 2]]) and np.array_equal(u_any[:, [0, 2]], t_any[:, [0, 2]])


def border_polygons(H, W):
    """axis-aligned and slanted polygons that touch every border of an H x W image"""
    return [rect(0, 0, W, H), [W / 2, 0, W, H / 2, W / 2, H, 0, H / 2], [-3.5, -2.25, 2 * W + 1.5, H / 3, W / 4, 2 * H + 0.75],
            [0, 0, W, H, W, 0, 0, H]]


def test_shapes_and_both_sides_of_the_lds_threshold(cuda):
    L = lds_words()
    lds_side, ws_side = (508, 645), (512, 640)
    plane = lambda hw: hw[0] * hw[1] // 32 + 1
    assert plane(lds_side) == L and plane(ws_side) == L + 1      # the last plane LDS holds, the first it does not
    gH, gW, gpolys = PC.golden_40gon()
    assert plane((gH, gW)) <= L
    sizes = [(1, 37), (45, 1), (1, 1), (63, 5), (64, 4), (65, 3), (31, 33), lds_side, ws_side, (gH, gW)]
    entries, images, areas, counts = [], [], [], []
    for H, W in sizes:
        polys = gpolys if (H, W) == (gH, gW) else border_polygons(H, W)
        mine = [polys[:1], polys[1:2], polys[2:3], polys]
        entries += mine
        exp = [PC.expected(H, W, e) for e in mine]
        images.append(np.stack([c for c, _ in exp]))
        areas += [a for _, a in exp]
        counts.append(len(mine))
    t_once, t_any = check_call(entries, sizes, counts, images, areas, cuda)
    assert (t_once[:, 2] > 0).sum() > len(sizes) and (t_any[:, 2] >= t_once[:, 2]).all() and (t_any[:, 2] > t_once[:, 2]).any()


def test_layout(cuda, first_only):
    cases, full = PC.cases(), PC.expected_all()
    rng = np.random.default_rng(3)
    pick = [int(v) for v in rng.permutation(len(cases))[:64]]
    # images without an entry at the front, in the middle and at the end; entries without a polygon
    counts = [0, 0] + [int(v) for v in rng.integers(0, 4, 60)] + [0, 0]
    counts[30] = 0
    counts[5] = 3
    entries, images, areas, sizes = [], [], [], []
    for g, (i, n) in enumerate(zip(pick, counts)):
        H, W, polys = cases[i]
        options = [(polys, full[i]), ([], (np.zeros((H, W), np.uint8), 0)), (polys[:1], first_only[i])]
        mine = [options[(g + k) % 3] for k in range(n)]
        entries += [e for e, _ in mine]
        images.append(np.stack([c for _, (c, _) in mine]) if n else np.zeros((0, H, W), np.uint8))
        areas += [a for _, (_, a) in mine]
        sizes.append((H, W))
    assert len(sizes) == 64 and any(len(e) == 0 for e in entries)
    t_once, _ = check_call(entries, sizes, counts, images, areas, cuda)
    empty = [k for k, e in enumerate(entries) if not e]
    assert (t_once[empty, 0] == 1).all() and (t_once[empty, 2] == 0).all()      # one count, H*W
    # S = 0: nothing to do, nothing returned
    slots, table, status = ops.rle_from_polygons([], [(5, 7), (3, 3)], [0, 0], device=cuda)
    assert tuple(slots.shape) == (0, 2) and tuple(table.shape) == (0, 4) and tuple(status.shape) == (0, 4)
    # one call of a single entry
    i = pick[7]
    check_call([cases[i][2]], [cases[i][:2]], [1], [full[i][0][None]], [full[i][1]], cuda)


def raw_call(lib, xy, point_offsets, entry_polys, images, rule, sw, dev):
    """the ABI itself (ops would raise on these inputs): flat sentinel-filled buffer (table, slots, status) after the call"""
    S, P, G = len(entry_polys) - 1, len(point_offsets) - 1, len(images)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    xy_d, po_d, ep_d = d(xy, np.float64), d(point_offsets, np.int32), d(entry_polys, np.int32)
    im = np.ascontiguousarray(images, dtype=np.int64)
    out = torch.full((S * (8 + sw),), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.hgl_rle_from_polygons_workspace_bytes(im.ctypes.data, G, S, P)), 256), dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    rc = lib.hgl_rle_from_polygons_device(xy_d.data_ptr(), po_d.data_ptr(), P, ep_d.data_ptr(), S, im.ctypes.data, G, rule, base + 16 * S,
                                          sw, base, base + 4 * S * (4 + sw), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_refused_entries_between_good_ones(cuda):
    lib = _lib.load()
    H, W = 40, 50
    good = [rect(5, 5, 30, 20), [2.5, 3.5, 45.0, 10.25, 20.0, 38.0]]
    nan, far = [4.0, 4.0, float("nan"), 9.0, 20.0, 30.0], [4.0, 4.0, 1.0e5, 9.0, 20.0, 30.0]
    # entries: good | NaN (+ a good polygon) | good | 1e5 | good | a polygon without a vertex (after a good one) | good
    polys = [good[0], good[1], nan, good[1], far, good[0], good[0], [], good[0], good[1]]
    entry_polys = [0, 1, 3, 4, 5, 6, 8, 10]
    xy = np.concatenate([np.asarray(p, np.float64) for p in polys])
    po = np.concatenate([[0], np.cumsum([len(p) // 2 for p in polys])])
    S, sw = 7, ops.rle_slot_words(H, W)
    refused = [1, 3, 5]
    kept = {0: [good[0]], 2: [good[1]], 4: [good[0]], 6: [good[0], good[1]]}
    for rule in (0, 1):
        outs = [raw_call(lib, xy, po, entry_polys, [[H, W, 0]], rule, sw, cuda) for _ in range(2)]
        assert outs[0][0] == 0 and outs[1][0] == 0 and torch.equal(outs[0][1], outs[1][1])
        flat = outs[0][1]
        slots, table = ops.rle_split(flat, S, sw)
        status = flat[S * (4 + sw):].reshape(S, 4).cpu().numpy()
        for s in refused:
            assert table[s].tolist() == [0, 3, 0, 0] and status[s].tolist() == [2, 0, 0, 0], s
            assert bool((slots[s] == SENTINEL).all()), s
        for s, e in kept.items():
            count, area = PC.expected(H, W, e)
            want_t, want_s = encoded([PC.by_rule(count, rule)[None]], sw, cuda)
            assert torch.equal(table[s], want_t[0]) and torch.equal(slots[s], want_s[0]) and status[s].tolist() == [0, area, 0, 0], s


def test_composition_with_decoder_iou_and_matcher(cuda):
    H, W = 70, 90
    polys = [rect(3 + 9 * i, 2 + 5 * i, 30 + 9 * i, 25 + 5 * i) for i in range(6)] + [[10.5, 60.0, 80.0, 5.5, 85.0, 66.0]]
    entries = [[p] for p in polys] + [polys[:3], polys]
    sizes, counts = [(H, W), (33, 31)], [len(entries), 2]
    other = [[rect(0, 0, 31, 33)], [[1.0, 1.0, 30.0, 5.0, 12.0, 31.0]]]
    all_entries = entries + other
    want = [PC.by_rule(PC.expected(H, W, e)[0], "once") for e in entries] + [PC.by_rule(PC.expected(33, 31, e)[0], "once") for e in other]
    slots, table, status = ops.rle_from_polygons(all_entries, sizes, counts, device=cuda)
    assert (status[:, 0] == 0).all()
    masks, _, dstatus = ops.rle_decode_group(slots, table, sizes, counts)
    assert (dstatus[:, 0] == 0).all()
    n = len(entries)
    assert np.array_equal(masks[0].cpu().numpy(), np.stack(want[:n])) and np.array_equal(masks[1].cpu().numpy(), np.stack(want[n:]))
    areas = np.asarray([int(m.sum()) for m in want])
    assert np.array_equal(table[:, 2].cpu().numpy(), areas) and np.array_equal(dstatus[:, 1].cpu().numpy(), areas)
    # against the encoder's set of the same masks: I = U = area
    es, et = ops.rle_encode(torch.from_numpy(np.stack(want[:n])).to(cuda))
    iu = ops.rle_iou(slots[:n].contiguous(), table[:n].contiguous(), es, et, H, W).cpu().numpy()
    assert np.array_equal(iu[:, 0], areas[:n]) and np.array_equal(iu[:, 1], areas[:n])
    # a set against itself: every entry its own best partner (the masks are pairwise different and none is empty)
    assert (areas > 0).all() and len({m.tobytes() for m in want[:n]}) == n
    _, ma, mb = ops.rle_match(slots, table, slots, table, sizes, counts, counts, matrix=False)
    for m in (ma.cpu().numpy(), mb.cpu().numpy()):
        assert np.array_equal(m[:, 0], np.zeros(len(want))) and np.array_equal(m[:, 1], areas) and np.array_equal(m[:, 3], areas)
        assert m[:, 2].tolist() == list(range(n)) + [0, 1]
