"""The contract of hgl_rle_paint_device (include/hybridgl.h) in numpy, and the cases the tests paint.

mask_of_entry   what the decoder would write for an entry (forms 0 and 1, the code 0 / 1 / 2 rules)
edge_of         M & ~(up & down & left & right), a neighbour outside the image counting as clear
blend           sat_u8(rint(f32(c)*a + f32(colour)*b)): two products and a sum, each rounded to fp32, no fused multiply-add
paint           the whole call, into buffers the caller filled with a sentinel; returns what the case list counts of itself
cases()         the list; check_coverage(cases) asserts that it is not thin (tests/test_paint_cases_host.py runs it on the CPU)

Everything is integers and bytes: every comparison against these functions is bit-equal."""
import numpy as np

FILL, OUTLINE = 1 << 24, 1 << 25
f32 = np.float32


def style_row(fill=None, a=1.0, b=0.0, outline=None):
    """one [4] uint32 style row: fill / outline are (R, G, B) or None"""
    rgb = lambda c: (int(c[0]) << 16) | (int(c[1]) << 8) | int(c[2])
    w0 = (rgb(fill) | FILL if fill is not None else 0) | (OUTLINE if outline is not None else 0)
    return np.array([w0, np.array([a], f32).view(np.uint32)[0], np.array([b], f32).view(np.uint32)[0],
                     rgb(outline) if outline is not None else 0], dtype=np.uint32)


def counts_of(mask):
    """column-major run lengths of a bool [H,W] mask, the first count the leading zeros"""
    flat = np.asarray(mask, bool).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    ends = np.concatenate([change, [flat.size]])
    counts = np.diff(np.concatenate([[0], ends]))
    return ([0] if flat[0] else []) + counts.tolist()


def plane_of(mask):
    """the form-1 slot: bit p % 32 of word p // 32 over p = x*H + y"""
    flat = np.asarray(mask, bool).T.reshape(-1)
    bits = np.zeros((flat.size + 31) // 32 * 32, np.uint64)
    bits[:flat.size] = flat
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def mask_of_entry(slot, row, H, W, sw):
    """(code, M [H,W] bool) of one entry: code 2 (no mask) gives an empty M"""
    n, form = int(row[0]), int(row[1])
    HW, pw = H * W, (H * W + 31) // 32
    if n < 0 or not ((form == 0 and n <= sw) or (form == 1 and pw <= sw)):
        return 2, np.zeros((H, W), bool)
    flat = np.zeros(HW, bool)
    if form == 1:
        words = np.asarray(slot[:pw], np.uint32)
        flat[:] = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:HW].astype(bool)
        code = 0
    else:
        ends = np.minimum(np.cumsum(np.asarray(slot[:n], np.uint64)), HW).astype(np.int64)      # saturated at H*W
        starts = np.concatenate([[0], ends[:-1]]) if n else ends
        for k in range(1, n, 2):
            flat[starts[k]:ends[k]] = True
        code = 0 if n and int(np.asarray(slot[:n], np.uint64).sum()) == HW else 1
    return code, flat.reshape(W, H).T.copy()


def edge_of(M):
    P = np.zeros((M.shape[0] + 2, M.shape[1] + 2), bool)
    P[1:-1, 1:-1] = M
    return M & ~(P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:])


def blend(c, colour, a, b):
    """c: uint8 [..., 3]; colour: (R, G, B); a, b: fp32 -> (uint8 [..., 3], the sums before rint)"""
    with np.errstate(all="ignore"):
        ca = c.astype(f32) * f32(a)
        kb = np.asarray(colour, f32) * f32(b)
        v = (ca + kb).astype(f32)
        r = np.rint(v)
        s = np.where(r >= 255, f32(255), np.where(r > 0, r, f32(0)))      # a NaN gives 0
    return s.astype(np.uint8), v


def rgb_of(word):
    return ((int(word) >> 16) & 255, (int(word) >> 8) & 255, int(word) & 255)


def paint(slots, table, images, order, style, base, out, labels, status):
    """The call: images [G,5] rows (H, W, e, k, p); slots uint32 [S,sw]; order int32 [K]; style uint32 [K,4]; base uint8
    [canvas_pixels,3] or None; out uint8 [canvas_pixels,3], labels int32 [canvas_pixels] or None and status int32 [K,4] are
    written in place, and only where the contract writes.  Returns the statistics check_coverage reads."""
    S, sw = slots.shape
    K, G = len(order), len(images)
    stats = dict(cover=0, twice=False, code2=False, code3=False, tie_even=False, tie_odd=False, saturate=False, border=False,
                 rows6364=False, cols6364=False, codes=set())
    for g, (H, W, e, k, p) in enumerate(images):
        e1, k1 = (images[g + 1][2], images[g + 1][3]) if g + 1 < G else (S, K)
        canvas = np.zeros((H, W, 3), np.uint8) if base is None else base[p:p + H * W].reshape(H, W, 3).copy()
        lab = np.full((H, W), -1, np.int32)
        cover = np.zeros((H, W), np.int32)
        listed, good = [], []
        for t in range(k, k1):
            o = int(order[t])
            if not 0 <= o < e1 - e:
                status[t] = (3, 0, 0, 0)
                good.append(False)
                continue
            listed.append(o)
            code, M = mask_of_entry(slots[e + o], table[e + o], H, W, sw)
            if code == 2:
                status[t] = (2, 0, 0, 0)
                good.append(False)
                continue
            E = edge_of(M)
            a, b = style[t, 1:3].view(f32)
            if not (np.isfinite(a) and np.isfinite(b)):
                status[t] = (4, int(M.sum()), 0, 0)
                good.append(False)
                continue
            status[t] = (code, int(M.sum()), int(E.sum()), 0)
            good.append(True)
            w0 = int(style[t, 0])
            touched = np.zeros((H, W), bool)
            if w0 & FILL:
                new, v = blend(canvas[M], rgb_of(w0), a, b)
                frac = v - np.floor(v)
                tie = (frac == 0.5) & (v > 0) & (v < 255)
                stats["tie_even"] |= bool((tie & (canvas[M] % 2 == 0)).any())
                stats["tie_odd"] |= bool((tie & (canvas[M] % 2 == 1)).any())
                stats["saturate"] |= bool(((np.rint(v) > 255) | (np.rint(v) < 0)).any())
                canvas[M] = new
                touched |= M
            if w0 & OUTLINE:
                canvas[E] = rgb_of(style[t, 3])
                touched |= E
                stats["border"] |= bool(E[0].any() or E[-1].any() or E[:, 0].any() or E[:, -1].any())
                stats["rows6364"] |= bool(H > 64 and E[63].any() and E[64].any())
                stats["cols6364"] |= bool(W > 64 and E[:, 63].any() and E[:, 64].any())
            lab[touched] = t - k
            cover += touched
        stats["codes"] |= {int(status[t, 0]) for t in range(k, k1)}
        stats["cover"] = max(stats["cover"], int(cover.max()))
        stats["twice"] |= len(set(listed)) < len(listed)
        codes = [int(status[t, 0]) for t in range(k, k1)]
        for c, key in ((2, "code2"), (3, "code3")):      # between good ones
            stats[key] |= any(codes[i] == c and any(good[:i]) and any(good[i + 1:]) for i in range(len(codes)))
        out[p:p + H * W] = canvas.reshape(-1, 3)
        if labels is not None:
            labels[p:p + H * W] = lab.reshape(-1)
    return stats


def layout(sizes, counts, order_counts, gaps=None):
    """(images [G,5] rows, canvas_pixels): the canvases back to back, gaps[g] pixels in front of image g"""
    rows, e, k, p = [], 0, 0, 0
    for g, ((H, W), n, m) in enumerate(zip(sizes, counts, order_counts)):
        p += gaps[g] if gaps else 0
        rows.append([H, W, e, k, p])
        e, k, p = e + n, k + m, p + H * W
    return rows, p


def blob(rng, H, W, kind):
    """a mask with structure: a box, a disc, noise, the full image, a frame that crosses rows / columns 63 | 64"""
    y, x = np.mgrid[:H, :W]
    if kind == "full":
        return np.ones((H, W), bool)
    if kind == "noise":
        return rng.random((H, W)) < 0.5
    if kind == "disc":
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(H, W) // 2 + 2)
        return (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    if kind == "cross":      # a thick band over the middle rows and one over the middle columns
        return (abs(y - H // 2) <= max(H // 4, 1)) | (abs(x - W // 2) <= max(W // 4, 1))
    y0, x0 = rng.integers(0, H), rng.integers(0, W)
    return (y >= y0) & (y <= y0 + rng.integers(0, H)) & (x >= x0) & (x <= x0 + rng.integers(0, W))


PALETTE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (250, 200, 3), (17, 33, 65), (128, 128, 128), (255, 255, 255), (0, 0, 0)]
DEMO = dict(fill=(0, 0, 255), a=1.0, b=0.7)


def encode_set(masks_sizes, sw, forms, broken=(), short=()):
    """slots [S,sw] uint32 and table [S,4] int32 of masks in the given forms; `broken`: entries whose row describes no mask;
    `short`: form-0 entries that lose their last count"""
    S = len(masks_sizes)
    slots = np.full((S, sw), 0xDEADBEEF, np.uint32)
    table = np.zeros((S, 4), np.int32)
    for s, (M, form) in enumerate(zip(masks_sizes, forms)):
        if s in broken:
            table[s] = (sw + 5, 0, 0, 0) if s % 2 else (3, 2, 0, 0)
            continue
        if form == 0:
            c = counts_of(M)
            if s in short and len(c) >= 2:      # the counts no longer sum to H*W: code 1
                c = c[:-1]
            assert len(c) <= sw
            slots[s, :len(c)] = c
            table[s] = (len(c), 0, int(M.sum()), 0)
        else:
            w = plane_of(M)
            assert len(w) <= sw
            slots[s, :len(w)] = w
            table[s] = (len(counts_of(M)), 1, int(M.sum()), 0)
    return slots, table


def make_case(seed, sizes, form=0, sw=None):
    """One group: every image gets a handful of entries and a paint list that stacks them, lists one twice, and carries a
    code-2 entry and a code-3 position between good ones; styles: the demo's (exact .5 ties, saturation), the palette with
    outlines, a halving blend, an outline alone."""
    rng = np.random.default_rng(seed)
    masks, forms, counts, order, order_counts, styles, broken, short = [], [], [], [], [], [], set(), set()
    for g, (H, W) in enumerate(sizes):
        n = 0 if (len(sizes) > 2 and g % 7 == 3) else 5
        m = 0 if (len(sizes) > 2 and g % 7 == 5) else (8 if n else 2)
        kinds = ["cross", "full", "box", "disc", "noise"]
        for i in range(n):
            masks.append(blob(rng, H, W, kinds[i]))
            forms.append(form if form in (0, 1) else int(rng.integers(0, 2)))
        if n:
            broken.add(len(masks) - 2)      # the image's entry 3
            if seed % 2:
                short.add(len(masks) - 3)   # its entry 2
        counts.append(n)
        order_counts.append(m)
        if m and n:
            # cross, full, cross again: >= 3 positions on the cross's pixels; entry 3 is code 2; 9 and -1 are code 3
            order += [0, 1, 3, 0, 9, 2, 4, -1]
            styles += [style_row(**DEMO), style_row(PALETTE[(seed + g) % 8], 0.5, 0.5, PALETTE[(seed + g + 1) % 8]),
                       style_row(PALETTE[2], 1.0, 1.0), style_row(outline=PALETTE[(seed + 3) % 8]),
                       style_row(**DEMO), style_row(PALETTE[(seed + 5) % 8], 1.0, 0.7, PALETTE[0]),
                       style_row(PALETTE[3], -0.5 if seed % 3 else float("inf"), 2.0, PALETTE[(seed + 2) % 8]), style_row(**DEMO)]
        elif m:
            order += [0, -1]      # an image without entries: every position is code 3
            styles += [style_row(**DEMO), style_row(outline=PALETTE[1])]
    need = max([len(counts_of(M)) if f == 0 else (M.size + 31) // 32 for M, f in zip(masks, forms)], default=1)
    sw = max(need, 1) if sw is None else sw
    slots, table = encode_set(masks, sw, forms, broken, short)
    return dict(seed=seed, sizes=list(sizes), counts=counts, order=np.array(order, np.int32).reshape(-1),
                order_counts=order_counts, style=np.array(styles, np.uint32).reshape(-1, 4), slots=slots, table=table, sw=sw,
                masks=masks, base_seed=seed + 1000)


# the sizes the kernel can go wrong at: one pixel, one row, one column, either side of the 64-row word and of the 64-column
# tile, a size off every multiple, both at once
EDGE_SIZES = [(1, 1), (1, 7), (7, 1), (63, 5), (64, 4), (65, 3), (5, 63), (4, 64), (3, 65), (31, 33)]


def cases():
    out = []
    for i, hw in enumerate(EDGE_SIZES):
        out.append(make_case(i, [hw], form=0))
        out.append(make_case(100 + i, [hw], form=1))
    for i in range(24):      # both boundaries at once, in groups of one to three images
        sizes = [(65 + (i + g) % 9, 66 + (2 * i + g) % 7) for g in range(1 + i % 3)]
        out.append(make_case(200 + i, sizes, form=2))
    return out


def base_of(case, canvas_pixels):
    return np.random.default_rng(case["base_seed"]).integers(0, 256, (canvas_pixels, 3), dtype=np.uint8)


def expect(case, with_base=True, with_labels=True, gaps=None, fence=0xA5):
    """(images, canvas_pixels, base, out, labels, status, stats) of a case, out / labels / status from sentinel-filled buffers"""
    images, total = layout(case["sizes"], case["counts"], case["order_counts"], gaps)
    base = base_of(case, total) if with_base else None
    out = np.full((total, 3), fence, np.uint8)
    labels = np.full(total, -(fence << 8), np.int32) if with_labels else None
    status = np.full((len(case["order"]), 4), fence, np.int32)
    stats = paint(case["slots"], case["table"], images, case["order"], case["style"], base, out, labels, status)
    return images, total, base, out, labels, status, stats


def check_coverage(todo):
    """a thin list cannot pass quietly"""
    stats = [expect(c)[-1] for c in todo]
    count = lambda f: sum(1 for s in stats if f(s))
    assert count(lambda s: s["cover"] >= 3) >= 40
    assert count(lambda s: s["twice"]) >= 20
    assert count(lambda s: s["code2"]) >= 20 and count(lambda s: s["code3"]) >= 20
    assert count(lambda s: s["tie_even"] and s["tie_odd"]) >= 20
    assert count(lambda s: s["saturate"]) >= 20
    assert count(lambda s: s["border"]) >= 20 and count(lambda s: s["rows6364"]) >= 20 and count(lambda s: s["cols6364"]) >= 20
    assert count(lambda s: 1 in s["codes"]) >= 10 and count(lambda s: 4 in s["codes"]) >= 10
    return stats


# ---- rle_paint_plan (csrc/rle_group.h) as Python arithmetic, for tests/native/rle_paint_sanitize.cpp: a case is
# (images rows, S, K, slot_words, canvas_pixels, base address, out address)
A = dict(base=0x7F0000000000, out=0x7F4000000000)


def plan_case(images, S, K, sw=8, canvas=None, base=None, out=None):
    images = [list(r) for r in images]
    if canvas is None:
        canvas = max([r[4] + r[0] * r[1] for r in images], default=0)
    return dict(images=images, S=S, K=K, sw=sw, canvas=canvas, base=A["base"] if base is None else base,
                out=A["out"] if out is None else out)


def plan_line_of(c):
    return " ".join(str(v) for v in [len(c["images"]), c["S"], c["K"], c["sw"], c["canvas"], c["base"], c["out"]]
                    + [v for r in c["images"] for v in r])


def plan_want_of(c):
    """None when the plan refuses the case, else ((tiles, words, blocks), per image (H, W, first, word0, tile0, pix0, entry0,
    entries))"""
    G, S, K = len(c["images"]), c["S"], c["K"]
    I32 = 1 << 31
    if not 1 <= G <= 64 or not (0 <= S < I32 and 0 <= K < I32) or not 0 <= c["sw"] < I32 or not 0 <= c["canvas"] < (1 << 60):
        return None
    tiles = words = blocks = 0
    rows, ext = [], []
    for g, (H, W, e, k, p) in enumerate(c["images"]):
        e1, k1 = (c["images"][g + 1][2], c["images"][g + 1][3]) if g + 1 < G else (S, K)
        if not (0 < H < I32 and 0 < W < I32 and H * W < I32):
            return None
        if not (0 <= e <= e1 <= S and (g or e == 0)) or not (0 <= k <= k1 <= K and (g or k == 0)):
            return None
        if not (0 <= p <= c["canvas"] and H * W <= c["canvas"] - p):
            return None
        if any(not (hi <= p or p + H * W <= lo) for lo, hi in ext):
            return None
        ext.append((p, p + H * W))
        Q = W * ((H + 63) // 64)
        rows.append((H, W, k, words, tiles, p, e, e1 - e))
        words += (k1 - k) * Q
        blocks += (k1 - k) * ((Q + 255) // 256)
        if words >= 1 << 32 or blocks >= I32:
            return None
        tiles += ((W + 63) // 64) * ((H + 63) // 64)
        if tiles >= I32:
            return None
    n = 3 * c["canvas"]
    if c["base"] and n and not (c["base"] + n <= c["out"] or c["out"] + n <= c["base"]):
        return None
    return (tiles, words, blocks), rows


PLAN_SIZES = [(70, 37), (64, 64), (1, 1), (480, 640), (3, 65), (65, 3), (31, 33), (5, 5)]
PLAN_N = [3, 0, 5, 64, 1, 2, 0, 7]
PLAN_M = [2, 1, 0, 64, 3, 0, 0, 9]


def plan_packed(sizes, counts, order_counts, gaps=None):
    images, total = layout(sizes, counts, order_counts, gaps)
    return images, sum(counts), sum(order_counts), total


def plan_refusals():
    """(a word of the message, the case): one per rule of the contract"""
    im, S, K, total = plan_packed(PLAN_SIZES, PLAN_N, PLAN_M)
    big = (1 << 31) - 1
    edit = lambda g, col, v: [[v if (i == g and j == col) else x for j, x in enumerate(r)] for i, r in enumerate(im)]
    return [
        ("0 images", plan_case([], 0, 0, canvas=0)),
        ("65 images", plan_case([[2, 2, 0, 0, 4 * g] for g in range(65)], 0, 0)),
        ("bad sizes", plan_case(im, -1, K)),
        ("bad sizes", plan_case(im, S, -1)),
        ("slot_words -1", plan_case(im, S, K, sw=-1)),
        ("slot_words 2147483648", plan_case(im, S, K, sw=1 << 31)),
        ("canvas_pixels -1", plan_case(im, S, K, canvas=-1)),
        ("bad size 0 x 64", plan_case(edit(1, 0, 0), S, K)),
        ("bad size 46341 x 46341", plan_case([[46341, 46341, 0, 0, 0]], 0, 0)),
        ("image 2: entries", plan_case(edit(3, 2, 2), S, K)),                 # a step back
        ("image 6: entries", plan_case(edit(7, 2, S + 1), S, K)),             # beyond S
        ("image 0: entries", plan_case(edit(0, 2, 1), S, K)),                 # the first entry is not 0
        ("image 3: list entries", plan_case(edit(4, 3, 1), S, K)),
        ("image 6: list entries", plan_case(edit(7, 3, K + 1), S, K)),
        ("image 0: list entries", plan_case(edit(0, 3, 1), S, K)),
        ("lie outside", plan_case(im, S, K, canvas=total - 1)),
        ("lie outside", plan_case(edit(2, 4, -1), S, K, canvas=total)),
        ("canvases of images 2 and 3 overlap", plan_case(edit(3, 4, im[2][4]), S, K, canvas=total)),
        ("too many plane words", plan_case([[1, big, 0, 0, 0]], 0, 3, canvas=big)),
        ("too many tiles", plan_case([[1, big, 0, 0, g * big] for g in range(64)], 0, 0)),
        ("out overlaps base", plan_case(im, S, K, out=A["base"] + 3 * total - 1)),
        ("out overlaps base", plan_case(im, S, K, out=A["base"] - 3 * total + 1)),
    ]
