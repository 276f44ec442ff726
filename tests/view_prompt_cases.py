"""The contract of a visual prompt (include/hybridgl.h HglViewPrompt; hybridgl_amd/csrc/view_prompt.h) in numpy, and the case
table the host, sanitizer and GPU tests share.  Window, taps, marker bands and gray are integers; the blend follows
oracle.clip_oracle.synthesize_views / bilinear_resize operation for operation, so at the default prompt views() IS that oracle.

A prompt here is a plain dict of the struct's fields (prompt(...) fills the defaults); boxes are inclusive XYXY."""
import numpy as np

from oracle.clip_oracle import CLIP_MEAN, IMAGENET_MEAN, IMAGENET_STD

F32 = np.float32
FIELDS = ("window", "pad_permille", "square", "local_bg", "global_bg", "marker", "thickness", "grow")
DEFAULT = dict(window=0, pad_permille=0, square=0, local_bg=0, local_fill=tuple(float(v) for v in CLIP_MEAN), global_bg=0,
               global_fill=(0, 0, 0), marker_rgb=(255, 0, 0), marker=0, thickness=1, grow=0)
PRESETS = {
    "hybridgl": {},
    "black": dict(global_bg=3, global_fill=(0, 0, 0)),
    "gray": dict(global_bg=2),
    "keep": dict(global_bg=1),
    "red_circle": dict(global_bg=1, marker=1, marker_rgb=(255, 0, 0), thickness=2),
    "masked_crop": dict(window=1, square=1),
    "crop": dict(window=1, square=1, local_bg=1),
}
# the single-field variations of the GPU test: pad 0 / 250, square on / off, each background, each marker at t 1 and 3 and g 0
# and 2; the marker that crosses the border comes from the boxes (a box on a corner, grown)
VARIATIONS = (
    [dict(window=1, pad_permille=p, square=s) for p in (0, 250) for s in (0, 1)]
    + [dict(window=1, pad_permille=4000, square=1, local_bg=1)]
    + [dict(global_bg=b, global_fill=(10, 200, 30)) for b in (0, 1, 2, 3)]
    + [dict(local_bg=1), dict(local_fill=(0.25, -1.5, 2.0))]
    + [dict(marker=k, thickness=t, grow=g, global_bg=1, marker_rgb=(0, 255, 64)) for k in (1, 2) for t in (1, 3) for g in (0, 2)]
    + [dict(marker=1, thickness=5, grow=40), dict(marker=2, thickness=64, grow=7, window=1, pad_permille=500)]
)
# one refusal per rule of view_prompt.h vp_refusal: (message, prompt fields, H, W, have_blurred, have_boxes)
REFUSALS = [
    ("image side outside 1..8192", {}, 8193, 10, 1, 1), ("image side outside 1..8192", {}, 10, 0, 1, 1),
    ("window is not 0 (frame) or 1 (box)", dict(window=2), 10, 10, 1, 1),
    ("pad_permille outside 0..4000", dict(pad_permille=4001), 10, 10, 1, 1),
    ("pad_permille outside 0..4000", dict(pad_permille=-1), 10, 10, 1, 1),
    ("square is not 0 or 1", dict(square=2), 10, 10, 1, 1),
    ("local_bg is not 0 (fill) or 1 (keep)", dict(local_bg=-1), 10, 10, 1, 1),
    ("local_fill is not finite", dict(local_fill=(0.0, float("nan"), 0.0)), 10, 10, 1, 1),
    ("global_bg is not 0 (blur), 1 (keep), 2 (gray) or 3 (fill)", dict(global_bg=4), 10, 10, 1, 1),
    ("marker is not 0 (none), 1 (ellipse) or 2 (box)", dict(marker=3), 10, 10, 1, 1),
    ("thickness outside 1..64", dict(thickness=0), 10, 10, 1, 1), ("thickness outside 1..64", dict(thickness=65), 10, 10, 1, 1),
    ("grow outside 0..4096", dict(grow=4097), 10, 10, 1, 1),
    ("a blur background needs the blurred image", {}, 10, 10, 0, 1),
    ("a box window or a marker needs the boxes", dict(window=1), 10, 10, 1, 0),
    ("a box window or a marker needs the boxes", dict(marker=2), 10, 10, 1, 0),
]


def prompt(preset="hybridgl", **fields):
    p = dict(DEFAULT)
    p.update(PRESETS[preset])
    assert all(k in DEFAULT for k in fields), fields
    p.update(fields)
    return p


def refusal(p, H, W, have_blurred=True, have_boxes=True):
    """vp_refusal: the message of the first broken rule, or None"""
    if not (1 <= H <= 8192 and 1 <= W <= 8192):
        return "image side outside 1..8192"
    if p["window"] not in (0, 1):
        return "window is not 0 (frame) or 1 (box)"
    if not 0 <= p["pad_permille"] <= 4000:
        return "pad_permille outside 0..4000"
    if p["square"] not in (0, 1):
        return "square is not 0 or 1"
    if p["local_bg"] not in (0, 1):
        return "local_bg is not 0 (fill) or 1 (keep)"
    if not all(np.isfinite(F32(v)) for v in p["local_fill"]):
        return "local_fill is not finite"
    if not 0 <= p["global_bg"] <= 3:
        return "global_bg is not 0 (blur), 1 (keep), 2 (gray) or 3 (fill)"
    if not 0 <= p["marker"] <= 2:
        return "marker is not 0 (none), 1 (ellipse) or 2 (box)"
    if not 1 <= p["thickness"] <= 64:
        return "thickness outside 1..64"
    if not 0 <= p["grow"] <= 4096:
        return "grow outside 0..4096"
    if p["global_bg"] == 0 and not have_blurred:
        return "a blur background needs the blurred image"
    if needs_boxes(p) and not have_boxes:
        return "a box window or a marker needs the boxes"
    return None


def needs_boxes(p):
    return p["window"] == 1 or p["marker"] != 0


def clamp_box(box, H, W):
    """-> (x0, y0, x1, y1, empty): empty as GIVEN (x1 < x0 or y1 < y0), then every coordinate clamped into the image"""
    x0, y0, x1, y1 = (int(v) for v in box)
    c = lambda v, hi: min(max(v, 0), hi)
    return c(x0, W - 1), c(y0, H - 1), c(x1, W - 1), c(y1, H - 1), (x1 < x0 or y1 < y0)


def window(p, box, H, W):
    """-> (ox, oy, ew, eh); box None = no box"""
    if p["window"] != 1 or box is None:
        return 0, 0, W, H
    x0, y0, x1, y1, empty = clamp_box(box, H, W)
    if empty:
        return 0, 0, W, H
    w, h = x1 - x0 + 1, y1 - y0 + 1
    m = max(w, h) * p["pad_permille"] // 1000
    if not p["square"]:
        return x0 - m, y0 - m, w + 2 * m, h + 2 * m
    s = max(w, h) + 2 * m
    return (x0 + x1 + 1 - s) // 2, (y0 + y1 + 1 - s) // 2, s, s


def taps(res, extent, origin):
    """one axis: (i0, i1, l0, l1) -- ATen's source index (one fma, emulated through float64 as oracle.clip_oracle._src_index
    does) inside the window, the taps stop at extent - 1, the origin is added last"""
    scale = F32(extent) / F32(res)
    d = (np.arange(res, dtype=F32) + F32(0.5)).astype(np.float64)
    src = np.maximum((np.float64(scale) * d - 0.5).astype(F32), F32(0))
    a = np.minimum(src.astype(np.int64), extent - 1)
    l1 = (src - a.astype(F32)).astype(F32)
    return a + origin, a + (a < extent - 1) + origin, (F32(1) - l1).astype(F32), l1


def _inside(DX, DY, A, B):
    if A <= 0 or B <= 0:
        return np.zeros(np.broadcast(DX, DY).shape, bool)
    return DX * DX * (B * B) + DY * DY * (A * A) <= (A * A) * (B * B)      # python / int64: below 2^58 by the size limits


def marker_band(p, box, H, W):
    """bool [H, W]: the pixels of the image that carry the marker of `box`"""
    out = np.zeros((H, W), bool)
    if p["marker"] == 0 or box is None:
        return out
    x0, y0, x1, y1, empty = clamp_box(box, H, W)
    if empty:
        return out
    g, t = p["grow"], p["thickness"]
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    if p["marker"] == 2:
        grown = lambda e: (x >= x0 - e) & (x <= x1 + e) & (y >= y0 - e) & (y <= y1 + e)
        return grown(g + t) & ~grown(g)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    DX, DY = 2 * x + 1 - (x0 + x1 + 1), 2 * y + 1 - (y0 + y1 + 1)
    return _inside(DX, DY, w + 2 * g + 2 * t, h + 2 * g + 2 * t) & ~_inside(DX, DY, w + 2 * g, h + 2 * g)


def gray(img):
    """[..., 3] uint8 -> [...] uint8: (77 R + 150 G + 29 B + 128) >> 8"""
    v = img.astype(np.int64)
    return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).astype(np.uint8)


def _resample(src, fill, ty, tx, H, W):
    """src [C, H, W] f32, fill [C]: oracle.clip_oracle.bilinear_resize with the taps given; a tap outside the image is `fill`"""
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = ty, tx

    def rows(ys):
        ok = (ys >= 0) & (ys < H)
        return np.where(ok[None, :, None], src[:, np.clip(ys, 0, H - 1), :], fill[:, None, None])

    def cols(r, xs):
        ok = (xs >= 0) & (xs < W)
        return np.where(ok[None, None, :], r[:, :, np.clip(xs, 0, W - 1)], fill[:, None, None])
    top, bot = rows(y0), rows(y1)
    # a row outside the image is fill in every column, also where the column lies inside: rows() made it so already
    t = cols(top, x0) * lx0 + cols(top, x1) * lx1
    b = cols(bot, x0) * lx0 + cols(bot, x1) * lx1
    return (t * ly0[:, None] + b * ly1[:, None]).astype(F32)


def views(sam_img, blurred, image_norm, masks, p, boxes=None, res=224):
    """-> (local, global) [N, 3, res, res] f32.  sam_img / blurred [H, W, 3] uint8 (blurred may be None unless global_bg is the
    blur), image_norm [3, H, W] f32, masks [N, H, W], boxes [N, 4] inclusive XYXY (None: none needed)."""
    assert refusal(p, *masks.shape[1:], blurred is not None, boxes is not None) is None
    H, W = masks.shape[1:]
    lfill = np.asarray(p["local_fill"], F32)
    gfill = np.asarray(p["global_fill"], np.uint8)
    bg = {0: blurred, 1: sam_img, 2: np.repeat(gray(sam_img)[:, :, None], 3, axis=2),
          3: np.broadcast_to(gfill, sam_img.shape)}[p["global_bg"]]
    loc, glo = [], []
    for n, m in enumerate(masks):
        m = m != 0
        box = boxes[n] if boxes is not None and needs_boxes(p) else None
        ox, oy, ew, eh = window(p, box, H, W)
        ty, tx = taps(res, eh, oy), taps(res, ew, ox)
        comp = np.where(m[:, :, None], sam_img, bg)
        comp = np.where(marker_band(p, box, H, W)[:, :, None], np.asarray(p["marker_rgb"], np.uint8), comp)
        g = (comp.astype(F32) / F32(255)).transpose(2, 0, 1)      # T.ToTensor
        g = _resample(g, gfill.astype(F32) / F32(255), ty, tx, H, W)
        glo.append(((g - IMAGENET_MEAN[:, None, None]) / IMAGENET_STD[:, None, None]).astype(F32))
        l = image_norm.astype(F32) if p["local_bg"] == 1 else np.where(m[None], image_norm.astype(F32), lfill[:, None, None])
        loc.append(_resample(l, lfill, ty, tx, H, W))
    return np.stack(loc), np.stack(glo)


# ---- the shared case table: images, masks and caller-supplied boxes -------------------------------------------------------------
SHAPES = [(37, 53, 32), (97, 130, 64)]      # H, W, res
N_MASKS = 6


def case_masks(H, W, seed=5):
    """N = 6: a seeded blob, a blob on a corner, then oracle.cases.edge_masks' specials: empty, thin line, full, single pixel"""
    from oracle.cases import edge_masks
    m = edge_masks(N_MASKS, H, W, seed)
    c = np.zeros((H, W), bool)
    c[: H // 4, W - W // 5:] = True      # a blob on the top right corner: its grown marker crosses the border
    m[1] = c
    return m


def mask_boxes(masks):
    """batched_mask_to_box: inclusive XYXY, (0, 0, 0, 0) for an empty mask"""
    out = np.zeros((len(masks), 4), np.int32)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[i] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return out


def caller_boxes(H, W):
    """N = 6 caller-supplied boxes: empty in x, empty in y, wholly outside the image (clamps to a corner pixel), hanging over
    every edge, a 1 x 1 box, a box larger than res in one direction"""
    return np.array([[9, 4, 8, 20], [3, 12, 30, 11], [-40, -30, -5, -2], [-7, -9, W + 11, H + 3], [W // 2, H // 2, W // 2, H // 2],
                     [2, 3, W - 2, 9]], np.int32)


def case_inputs(H, W, seed=3):
    from hybridgl_amd.synth import box_blur_u8, imagenet_normalize, synth_image
    img = synth_image(H, W, seed)
    return img, box_blur_u8(img), imagenet_normalize(img), case_masks(H, W)


# ---- the line protocol of tests/native/view_prompt_sanitize.cpp -----------------------------------------------------------------
def harness_line(p, H, W, res, box, pixels, have_blurred=1, have_boxes=1):
    """`H W res window pad square local_bg global_bg marker thickness grow fill_nan have_blurred have_boxes x0 y0 x1 y1 K (x y r g b)*K`"""
    nan = int(not all(np.isfinite(F32(v)) for v in p["local_fill"]))
    head = [H, W, res] + [p[k] for k in FIELDS] + [nan, have_blurred, have_boxes] + [int(v) for v in box] + [len(pixels)]
    return " ".join(str(v) for v in head + [v for px in pixels for v in px])


def harness_want(p, H, W, res, box, pixels, have_blurred=1, have_boxes=1):
    """the line the harness must print: `-1 message`, or `0 empty x0 y0 x1 y1 | ox oy ew eh | taps of output 0, res // 2, res - 1 on
    x then y as i0 i1 bits(l0) bits(l1) | marker gray per pixel`"""
    why = refusal(p, H, W, have_blurred, have_boxes)
    if why is not None:
        return "-1 " + why
    x0, y0, x1, y1, empty = clamp_box(box, H, W)
    b = box if needs_boxes(p) else None
    ox, oy, ew, eh = window(p, b, H, W)
    out = [f"0 {int(empty)} {x0} {y0} {x1} {y1}", f"{ox} {oy} {ew} {eh}"]
    tp = []
    for extent, origin in ((ew, ox), (eh, oy)):
        i0, i1, l0, l1 = taps(res, extent, origin)
        for o in (0, res // 2, res - 1):
            tp += [int(i0[o]), int(i1[o]), int(l0[o:o + 1].view(np.uint32)[0]), int(l1[o:o + 1].view(np.uint32)[0])]
    out.append(" ".join(str(v) for v in tp))
    band = marker_band(p, b, H, W) if H * W <= 1 << 16 else None
    px = []
    for (x, y, r, g, bl) in pixels:
        if band is not None:
            on = bool(band[y, x])
        else:      # a large image: the one pixel alone
            on = bool(marker_band_at(p, b, x, y, H, W))
        px += [int(on), int(gray(np.array([r, g, bl], np.uint8)))]
    out.append(" ".join(str(v) for v in px))
    return " | ".join(out)


def marker_band_at(p, box, x, y, H, W):
    """marker_band at one pixel, in python integers"""
    if p["marker"] == 0 or box is None:
        return False
    x0, y0, x1, y1, empty = clamp_box(box, H, W)
    if empty:
        return False
    g, t = p["grow"], p["thickness"]
    if p["marker"] == 2:
        grown = lambda e: x0 - e <= x <= x1 + e and y0 - e <= y <= y1 + e
        return grown(g + t) and not grown(g)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    DX, DY = 2 * x + 1 - (x0 + x1 + 1), 2 * y + 1 - (y0 + y1 + 1)
    ins = lambda A, B: A > 0 and B > 0 and DX * DX * B * B + DY * DY * A * A <= A * A * B * B
    return ins(w + 2 * g + 2 * t, h + 2 * g + 2 * t) and not ins(w + 2 * g, h + 2 * g)
