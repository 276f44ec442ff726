"""tests/paint_cases.py on the CPU: the case list's own coverage; the numpy statement of the paint contract against a naive loop
over pixels and list positions; render.DEMO_STYLE against a literal numpy restatement of the reference demo's overlay
(demo.py:212-219: the BGR swap, the uint8 wrap-around that zeroes two channels, addWeighted(img, 1, seg, 0.7, 0), the BGR file);
the palette's distinctness."""
import numpy as np

from hybridgl_amd import ops, render

import paint_cases as PC

f32 = np.float32


def test_the_case_list_covers_what_it_claims():
    todo = PC.cases()
    stats = PC.check_coverage(todo)
    assert len(stats) == len(todo) >= 40
    sizes = {hw for c in todo for hw in c["sizes"]}
    assert sizes >= set(PC.EDGE_SIZES)
    assert {int(c["table"][s, 1]) for c in todo for s in range(len(c["table"]))} >= {0, 1, 2}


def naive_mask(slot, row, H, W, sw):
    """pixel by pixel in run order"""
    n, form = int(row[0]), int(row[1])
    M = [[False] * W for _ in range(H)]
    if n < 0 or form not in (0, 1) or (form == 0 and n > sw) or (form == 1 and (H * W + 31) // 32 > sw):
        return 2, M
    if form == 1:
        for p in range(H * W):
            M[p % H][p // H] = bool((int(slot[p // 32]) >> (p % 32)) & 1)
        return 0, M
    p = 0
    for k in range(n):
        for _ in range(min(int(slot[k]), H * W - p)):      # clipped at the end of the image
            M[p % H][p // H] = bool(k & 1)
            p += 1
    return (0 if sum(int(v) for v in slot[:n]) == H * W else 1), M


def naive_paint(case, images, base, out, labels, status):
    slots, table, order, style, sw = case["slots"], case["table"], case["order"], case["style"], case["sw"]
    S, K, G = len(table), len(order), len(images)
    for g, (H, W, e, k, p) in enumerate(images):
        e1, k1 = (images[g + 1][2], images[g + 1][3]) if g + 1 < G else (S, K)
        pix = [[[0, 0, 0] if base is None else [int(v) for v in base[p + y * W + x]] for x in range(W)] for y in range(H)]
        lab = [[-1] * W for _ in range(H)]
        for t in range(k, k1):
            o = int(order[t])
            if o < 0 or o >= e1 - e:
                status[t] = (3, 0, 0, 0)
                continue
            code, M = naive_mask(slots[e + o], table[e + o], H, W, sw)
            if code == 2:
                status[t] = (2, 0, 0, 0)
                continue
            inside = lambda y, x: 0 <= y < H and 0 <= x < W and M[y][x]
            edge = [[M[y][x] and not (inside(y - 1, x) and inside(y + 1, x) and inside(y, x - 1) and inside(y, x + 1))
                     for x in range(W)] for y in range(H)]
            area, n_edge = sum(map(sum, M)), sum(map(sum, edge))
            a, b = (f32(v) for v in style[t, 1:3].view(f32))
            if not (np.isfinite(a) and np.isfinite(b)):
                status[t] = (4, area, 0, 0)
                continue
            status[t] = (code, area, n_edge, 0)
            w0, w3 = int(style[t, 0]), int(style[t, 3])
            col = [(w0 >> 16) & 255, (w0 >> 8) & 255, w0 & 255]
            ink = [(w3 >> 16) & 255, (w3 >> 8) & 255, w3 & 255]
            for y in range(H):
                for x in range(W):
                    if (w0 & PC.FILL) and M[y][x]:
                        for ch in range(3):
                            with np.errstate(all="ignore"):
                                v = np.rint(f32(f32(pix[y][x][ch]) * a) + f32(f32(col[ch]) * b))
                            pix[y][x][ch] = 0 if v != v else int(min(max(v, f32(0)), f32(255)))
                        lab[y][x] = t - k
                    if (w0 & PC.OUTLINE) and edge[y][x]:
                        pix[y][x] = list(ink)
                        lab[y][x] = t - k
        for y in range(H):
            for x in range(W):
                out[p + y * W + x] = pix[y][x]
                if labels is not None:
                    labels[p + y * W + x] = lab[y][x]


def test_the_numpy_statement_against_a_naive_loop():
    todo = PC.cases()
    pick = [c for c in todo if max(h * w for h, w in c["sizes"]) <= 33 * 31] + todo[-2:]
    assert len(pick) >= 20
    for k, c in enumerate(pick):
        for with_base, with_labels, gaps in ((True, True, None), (False, False, [3] * len(c["sizes"]))):
            if k % 2 and not with_base:
                continue
            images, total, base, out, labels, status, _ = PC.expect(c, with_base, with_labels, gaps)
            n_out = np.full_like(out, 0xA5)
            n_lab = None if labels is None else np.full_like(labels, -(0xA5 << 8))
            n_st = np.full_like(status, 0xA5)
            naive_paint(c, images, base, n_out, n_lab, n_st)
            assert np.array_equal(out, n_out) and np.array_equal(status, n_st), (c["seed"], with_base)
            assert labels is None or np.array_equal(labels, n_lab), c["seed"]
            if gaps:      # nothing outside the extents is written
                inside = np.zeros(total, bool)
                for H, W, _, _, p in images:
                    inside[p:p + H * W] = True
                assert (out[~inside] == 0xA5).all() and inside.sum() == total - 3 * len(images)


def test_the_blend_is_two_products_and_a_sum_in_fp32():
    c = np.arange(256, dtype=np.uint8).reshape(-1, 1).repeat(3, 1)
    # the demo's weights: 255 * 0.7f rounds to 178.5 exactly, so every base value is a tie; half to even, then saturation
    got, v = PC.blend(c, (0, 0, 255), 1.0, 0.7)
    assert (v[:, 2] == c[:, 2].astype(f32) + f32(178.5)).all() and np.array_equal(got[:, :2], c[:, :2])
    assert got[0, 2] == 178 and got[1, 2] == 180 and got[2, 2] == 180 and got[3, 2] == 182 and got[76, 2] == 254 and (got[77:, 2] == 255).all()
    # with a = 1 the unfused form and a fused multiply-add agree bit for bit: the only style that claims to match addWeighted
    fused = (c[:, 2].astype(np.float64) + np.float64(f32(255)) * np.float64(f32(0.7))).astype(f32)
    assert np.array_equal(fused, v[:, 2])
    # with another a they do not, and the contract is the unfused one
    got2, v2 = PC.blend(c, (9, 9, 9), 0.3, 0.7)
    fused2 = (np.float64(f32(0.3)) * c[:, 0] + np.float64(f32(f32(9) * f32(0.7)))).astype(f32)
    assert (fused2 != v2[:, 0]).any()
    # an overflowed product against one of the other sign is a NaN and paints 0; a plain overflow saturates
    assert PC.blend(c[5:6], (255, 255, 255), 3e38, -3e38)[0].tolist() == [[0, 0, 0]]
    assert PC.blend(c[1:2], (0, 0, 0), 3e38, 0.0)[0].tolist() == [[255, 255, 255]]
    assert PC.blend(c[5:6], (0, 0, 0), -1.0, 0.0)[0].tolist() == [[0, 0, 0]]


def test_demo_style_against_the_reference_overlay():
    rng = np.random.default_rng(5)
    H, W = 37, 41
    sam_img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)      # RGB, as np.array(Image.open(..).convert("RGB"))
    sam_img[0, :8, 2] = np.arange(70, 78)                          # around the saturation point and both parities
    mask = rng.random((H, W)) < 0.5
    mask[0, :8] = True
    # demo.py:212-219, statement by statement
    save_img = sam_img.copy()
    save_img = save_img[:, :, ::-1].copy()                         # cv2.cvtColor(save_img, cv2.COLOR_BGR2RGB): a channel swap
    seg = mask.astype("uint8") * 255
    seg = np.stack([seg, seg, seg], axis=2)                        # cv2.COLOR_GRAY2BGR
    with np.errstate(over="ignore"):
        seg[:, :, 2] = (255 - seg[:, :, 2]) * seg[:, :, 2]         # uint8 wrap-around: 0 * 255 and 255 * 0
        seg[:, :, 1] = (255 - seg[:, :, 1]) * seg[:, :, 1]
    assert seg.dtype == np.uint8 and not seg[:, :, 1:].any() and (seg[:, :, 0] == mask * 255).all()
    # cv2.addWeighted(save_img, 1, seg, 0.7, 0.) on 8-bit images: fp32 weights, round half to even, saturate
    acc = save_img.astype(f32) * f32(1) + seg.astype(f32) * f32(0.7) + f32(0)
    result_bgr = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    written = result_bgr[:, :, ::-1]                               # cv2.imwrite takes BGR: the file holds RGB
    # DEMO_STYLE through the contract
    assert render.DEMO_STYLE == dict(fill=(0, 0, 255), a=1.0, b=0.7, outline=None)
    row = ops.rle_paint_style(**render.DEMO_STYLE)
    c = PC.counts_of(mask)
    slots = np.zeros((1, len(c)), np.uint32)
    slots[0] = c
    table = np.array([[len(c), 0, int(mask.sum()), 0]], np.int32)
    out = np.zeros((H * W, 3), np.uint8)
    status = np.zeros((1, 4), np.int32)
    PC.paint(slots, table, [[H, W, 0, 0, 0]], np.zeros(1, np.int32), row[None], sam_img.reshape(-1, 3), out, None, status)
    assert np.array_equal(out.reshape(H, W, 3), written) and status[0, 0] == 0 and status[0, 1] == mask.sum()
    assert (out.reshape(H, W, 3)[0, :8, 2] == [248, 250, 250, 252, 252, 254, 254, 255]).all()


def test_the_palette_is_fixed_and_distinct():
    p = render.palette(255)
    assert len(set(p)) == 255 and (0, 0, 0) not in p and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in p)
    assert render.palette(3) == p[:3] == [(128, 0, 0), (0, 128, 0), (128, 128, 0)] and render.palette(0) == []
    assert render.palette(300)[255:] == p[:45]
    rows = render.proposal_styles(4)
    assert rows.shape == (4, 4) and rows.dtype == np.uint32 and (rows[:, 0] >> 24 == 3).all() and len(set(rows[:, 3].tolist())) == 4
