"""Geometries, inputs, reference and checker for the fused SAM mask post-processing (csrc/sam_glue.hip: hgl_sam_postprocess with
sam_postprocess_sep_kernel, sam_postprocess_kernel and sam_finalize_kernel), plain numpy, no GPU code.

The operation is Sam.postprocess_masks (modeling/sam.py:133-162) -- low-res logits -> bilinear to S x S -> crop [in_h, in_w] ->
bilinear to H x W, both align_corners=False -- followed by the threshold, calculate_stability_score (utils/amg.py:156-176),
batched_mask_to_box (utils/amg.py:303-346) and the two filters of automatic_mask_generator.py:287-298.

`reference` is the yardstick: source indices and weights exactly as oracle/clip_oracle.py:_src_index gives them (float32 ATen
semantics with one fma: they are part of the operation's definition, pure-float64 indices differ by up to 1e-3 in logit at
S = 1024), the four blends in float64.

`classify` restates csrc/post_geom.h (src_idx, the bounds of a tile, the fit test behind the host's choice) in Python and says,
per geometry, which kernel a call takes and, per 64 x 64 tile, whether the per-pixel kernel stages the tile's low-res patch in
LDS or reads global memory.  The table constants are read from post_geom.h, so a retune moves the expectations of
tests/test_post_cases_host.py instead of silently moving the cases to other routes; the restatement itself is held against
the header by tests/native/post_geom_routes.cpp (tests/test_post_cases_host.py).

`check_outputs` judges the four production outputs (masks, boxes, stability, keep) WITHOUT the kernel's logits, so it judges
the production configuration (full_logits == nullptr).  Tolerance: tol = 2^-20 max|low_res|.  A pixel is four nested convex
blends; each is two products, one sum and the rounded weight 1 - l1, and no convex blend leaves the input range, so each of
the sixteen roundings is at most 2^-24 max|low_res|: 2^-20 is a bound, not a fit (the float32 CPU implementations, torch's
F.interpolate and the numpy oracle, stay below 2.4e-6 on these inputs; tests/test_post_cases_host.py).  A pixel whose reference
value lies within tol of a threshold is undecided: it may fall either way, and `undecided_share` caps how many there may be.

tests/test_post_cases_host.py checks this module on the CPU, tests/test_gpu_postprocess_paths.py runs the device code.
"""
import os
import re
from collections import namedtuple

import numpy as np

from oracle.clip_oracle import _src_index

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POST_GEOM = os.path.join(ROOT, "hybridgl_amd", "csrc", "post_geom.h")

MASK_THRESHOLD = 0.0            # the model's value (Sam.mask_threshold)
UNDECIDED_CAP = 1e-3            # share of a candidate's pixels that may lie within tol of one of the three thresholds


# ------------------------------------------------------------------------------------------------------------- the geometries
# orig = (H, W) of the output, inp = (in_h, in_w) of the crop of the S x S plane, low = side of the low-res plane.
# kernel: "sep" (shared tables) or "pix" (per-pixel); tiles: "staged" / "unstaged" / "mixed" for the per-pixel kernel's tiles
Geom = namedtuple("Geom", "orig inp S low kernel tiles note")

GEOMS = [
    Geom((192, 256), (192, 256), 256, 64, "sep", "staged", "aligned rows"),
    Geom((333, 500), (171, 256), 256, 64, "sep", "staged", "downscale, W%16 = 4"),
    Geom((160, 200), (205, 256), 256, 64, "sep", "staged", "W%16 = 8"),
    Geom((147, 110), (256, 192), 256, 64, "sep", "staged", "exactly 112 stage-1 columns"),
    Geom((700, 900), (199, 256), 256, 64, "sep", "staged", "165 tiles, patch 7"),
    Geom((1, 1), (256, 256), 256, 64, "sep", "staged", "single pixel"),
    Geom((427, 640), (683, 1024), 1024, 256, "sep", "staged", "production size"),
    Geom((20, 193), (100, 193), 256, 64, "sep", "staged", "5 : 1 rows, 1 : 1 columns: a corner pixel lights ONE output pixel"),
    Geom((146, 109), (256, 192), 256, 64, "pix", "staged", "113 stage-1 columns"),
    Geom((96, 128), (192, 256), 256, 64, "pix", "staged", "2 : 1"),
    Geom((130, 70), (256, 138), 256, 64, "pix", "staged", "portrait"),
    Geom((87, 65), (256, 192), 256, 64, "pix", "staged", "patch exactly 48"),
    Geom((300, 400), (768, 1024), 1024, 256, "pix", "staged", "production size"),
    Geom((53, 40), (256, 192), 256, 64, "pix", "unstaged", "49 patch columns"),
    Geom((64, 64), (256, 256), 256, 64, "pix", "unstaged", "one tile, the patch is the whole low-res plane"),
    Geom((13, 9), (256, 177), 256, 64, "pix", "unstaged", "W < 16"),
    Geom((97, 130), (764, 1024), 1024, 256, "pix", "unstaged", "production size"),
    Geom((65, 65), (256, 256), 256, 64, "pix", "mixed", "1 staged + 3 unstaged tiles, ph <= 48 < pw and pw <= 48 < ph, odd W"),
]


def geom_id(g):
    return f"{g.orig[0]}x{g.orig[1]}-in{g.inp[0]}x{g.inp[1]}-S{g.S}"


# ----------------------------------------------------------------------------------------------------------- path classifier
def table_constants(path=POST_GEOM):
    """PTW, PTH, PR, PX1 as csrc/post_geom.h declares them"""
    src = open(path).read()
    out = {}
    for name in ("PTW", "PTH", "PR", "PX1"):
        m = re.findall(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + name + r"\s*=\s*(\d+)\s*[,;]", src)
        if len(m) != 1:
            raise ValueError(f"{name}: {len(m)} declarations in {os.path.basename(path)}")
        out[name] = int(m[0])
    return out


def src_idx(scale, dst, in_size):
    """src_idx of post_geom.h for one destination index or an array of them: fmaf(scale, dst + 0.5f, -0.5f) (the float64
    product of two float32 values is exact, so one rounding of it is the fma), clamped -> (i0, i1)"""
    f = (np.float64(F32(scale)) * (np.asarray(dst).astype(F32) + F32(0.5)).astype(np.float64) - 0.5).astype(F32)
    f = np.where(f < 0, F32(0), f)
    i0 = np.minimum(f.astype(np.int64), in_size - 1)
    return i0, i0 + (i0 < in_size - 1)


def _scale(a, b):
    return F32(a) / F32(b)


def _axis(out, in1, low, S, tile):
    """per 64-wide strip of one axis: (stage-1 count, low-res patch side), as both kernels compute them"""
    s1, s2 = _scale(in1, out), _scale(low, S)
    o0 = np.arange(0, out, tile)
    ol = np.minimum(o0 + tile - 1, out - 1)
    a0, _ = src_idx(s1, o0, in1)
    _, b1 = src_idx(s1, ol, in1)
    u0, _ = src_idx(s2, a0, low)
    _, e1 = src_idx(s2, b1, low)
    return [(int(n), int(m)) for n, m in zip(b1 - a0 + 1, e1 - u0 + 1)]


def sep_fits(out, in1, low, S, c=None):
    """post_sep_fits: every 64-wide strip of one axis fits the shared tables"""
    c = c or table_constants()
    return all(cols <= c["PX1"] and patch <= c["PR"] for cols, patch in _axis(out, in1, low, S, c["PTW"]))


Tile = namedtuple("Tile", "by bx ph pw cols staged")
Route = namedtuple("Route", "sep tiles n_staged n_unstaged max_cols max_patch")


def classify(g, c=None):
    """-> Route: sep = the host chooses the shared-table kernel (with HGL_SAM_POST_SEP unset); tiles = the tiles of the launch
    with the low-res patch (ph x pw), the stage-1 column count and whether the per-pixel kernel would stage the patch"""
    c = c or table_constants()
    (H, W), (ih, iw) = g.orig, g.inp
    ys = _axis(H, ih, g.low, g.S, c["PTH"])
    xs = _axis(W, iw, g.low, g.S, c["PTW"])
    tiles = [Tile(by, bx, ph, pw, cols, ph <= c["PR"] and pw <= c["PR"])
             for by, (_, ph) in enumerate(ys) for bx, (cols, pw) in enumerate(xs)]
    sep = sep_fits(W, iw, g.low, g.S, c) and sep_fits(H, ih, g.low, g.S, c)
    ns = sum(t.staged for t in tiles)
    return Route(sep, tiles, ns, len(tiles) - ns, max(max(a for a, _ in xs), max(a for a, _ in ys)),
                 max(max(t.ph, t.pw) for t in tiles))


def store_routes(g, K):
    """which store forms the launch takes: "vector" (a thread's 16 pixels as one aligned 16-byte word) and "bytewise" (a
    partial or unaligned segment), restating `npx == PPX && (pix0 & 15) == 0`"""
    H, W = g.orig
    x = np.arange(0, W, 16)
    npx = np.minimum(16, W - x)
    pix0 = (np.arange(K)[:, None, None] * H * W + np.arange(H)[None, :, None] * W + x[None, None, :])
    vec = (npx[None, None, :] == 16) & (pix0 % 16 == 0)
    return {"vector": bool(vec.any()), "bytewise": bool((~vec).any())}


# ------------------------------------------------------------------------------------------------------------------ reference
def reference(low, inp, orig, S):
    """low [K, hl, wl] float32 -> float64 [K, H, W]: _src_index's float32 indices and weights, the four blends in float64
    (stage 1 is evaluated only on the rows and columns that survive the crop)"""
    low = np.asarray(low)
    assert low.dtype == F32 and low.ndim == 3
    (H, W), (ih, iw) = orig, inp
    hl, wl = low.shape[1:]
    v0, v1, m0, m1 = (a[:ih] for a in _src_index(S, hl))
    u0, u1, n0, n1 = (a[:iw] for a in _src_index(S, wl))
    y0, y1, ly0, ly1 = _src_index(H, ih)
    x0, x1, lx0, lx1 = _src_index(W, iw)
    m0, m1, n0, n1, ly0, ly1, lx0, lx1 = (a.astype(np.float64) for a in (m0, m1, n0, n1, ly0, ly1, lx0, lx1))
    out = np.empty((len(low), H, W), dtype=np.float64)
    for k, L in enumerate(low.astype(np.float64)):
        a = L[:, u0] * n0 + L[:, u1] * n1                          # [hl, iw]
        b = a[v0] * m0[:, None] + a[v1] * m1[:, None]              # [ih, iw]
        c = b[:, x0] * lx0 + b[:, x1] * lx1                        # [ih, W]
        out[k] = c[y0] * ly0[:, None] + c[y1] * ly1[:, None]
    return out


def tolerance(low):
    return float(np.abs(low).max()) * 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------------- patterns
RANDOM = 8
STRUCTURED = ("const_off", "const_on", "corner_tl", "corner_tr", "corner_bl", "corner_br", "ramp_x", "ramp_y")
NAMES = tuple(f"random{i}" for i in range(RANDOM)) + STRUCTURED
# the candidates of the K = 8 batch of the one-tile geometries: half random, half structured
PICK8 = (0, 1, 2, 3, NAMES.index("const_off"), NAMES.index("const_on"), NAMES.index("corner_br"), NAMES.index("ramp_y"))


def last_low(n_in, low, S):
    """the low-res index under the last row / column that survives the crop: floor((in - 1) low / S), not low - 1"""
    return (n_in - 1) * low // S


def planes(g):
    """-> (names, low [16, low, low] float32): eight N(0, 3) planes, distinct per candidate (a permutation of candidates shows),
    and eight structured ones"""
    (ih, iw), n = g.inp, g.low
    rng = np.random.default_rng([20240607, g.orig[0], g.orig[1], ih, iw, g.S])
    low = np.empty((len(NAMES), n, n), dtype=F32)
    low[:RANDOM] = (rng.standard_normal((RANDOM, n, n)) * 3).astype(F32)
    cy, cx = last_low(ih, n, g.S), last_low(iw, n, g.S)
    s = {k: i for i, k in enumerate(NAMES)}
    low[s["const_off"]] = -5                   # empty mask, 0/0 stability, box 0,0,0,0
    low[s["const_on"]] = 5                     # inter == union == H*W, full box
    for name, (v, u) in (("corner_tl", (0, 0)), ("corner_tr", (0, cx)), ("corner_bl", (cy, 0)), ("corner_br", (cy, cx))):
        low[s[name]] = -10                     # one low-res pixel on, at a corner of the region that survives the crop
        low[s[name], v, u] = 10
    # ramps from -6.3 to 5.9 over the surviving region (and on beyond it): 0, +-0.1 and +-1 are crossed inside the output
    low[s["ramp_x"]] = (-6.3 + 12.2 * np.arange(n) / max(cx, 1)).astype(F32)[None, :]
    low[s["ramp_y"]] = (-6.3 + 12.2 * np.arange(n) / max(cy, 1)).astype(F32)[:, None]
    return NAMES, low


def batch(g, K):
    """the K = 16 batch, K = 15 (the same minus its last plane) or K = 8 (PICK8) -> (names, low, index of each plane in the
    K = 16 batch)"""
    names, low = planes(g)
    idx = {16: tuple(range(16)), 15: tuple(range(15)), 8: PICK8}[K]
    return tuple(names[i] for i in idx), np.ascontiguousarray(low[list(idx)]), idx


def batch_sizes(g):
    """K = 16 (gridDim.z % 8 == 0: the XCD remap is on), 15 (off), and 8 where the launch has one tile per candidate"""
    nt = -(-g.orig[0] // 64) * -(-g.orig[1] // 64)
    return (16, 15, 8) if nt == 1 else (16, 15)


# predicted IoUs of the K = 16 batch for the runs with the filter on: above 0.7, below it, exactly 0.7 (dropped: the test is
# a strict >) and NaN (dropped); const_off, const_on, one corner and one ramp survive
IOU16 = np.array([0.9, 0.5, 0.7, np.nan, 0.95, 0.71, 0.3, 0.8,
                  0.9, 0.99, 0.9, 0.7, 0.75, np.nan, 0.85, 0.2], dtype=F32)

# off: stability offset; iou_thr: -1e30 = the filter is off; stab_thr 0: no stability filter (NaN survives), 1.0: only
# inter == union survives (the all-on plane, stability exactly 1.0)
Params = namedtuple("Params", "name off iou_thr stab_thr")
PARAMS = [
    Params("off1.0-nofilter", 1.0, -1e30, 0.0),
    Params("off1.0-iou0.7-stab1.0", 1.0, 0.7, 1.0),
    Params("off0.1-nofilter-stab1.0", 0.1, -1e30, 1.0),
    Params("off0.1-iou0.7", 0.1, 0.7, 0.0),
]


def passes_iou(iou, iou_thr):
    """the kernels' test: the filter exists only for thresholds > 0 and is a strict float32 `>` (NaN fails)"""
    iou = np.asarray(iou, dtype=F32)
    if not F32(iou_thr) > 0:
        return np.ones(iou.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return iou > F32(iou_thr)


# -------------------------------------------------------------------------------------------------------------------- checker
def box_of(mask):
    """batched_mask_to_box of one mask: XYXY inclusive, None when empty"""
    ys, xs = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    return None if not len(ys) else (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


class Bounds:
    """What the reference of one batch admits, per candidate, at tolerance tol and stability offset off: computed once and
    shared by every run that is judged against it"""

    def __init__(self, ref, tol, off, thr=MASK_THRESHOLD):
        self.ref, self.tol, self.off, self.thr = ref, tol, off, thr
        K, H, W = ref.shape
        self.sure = ref > thr + tol                     # on in every admissible result
        self.poss = ref > thr - tol                     # on in some admissible result
        self.decided = self.sure | ~self.poss
        self.inter = np.stack([(ref > thr + off + tol).sum((1, 2)), (ref > thr + off - tol).sum((1, 2))], 1)
        self.union = np.stack([(ref > thr - off + tol).sum((1, 2)), (ref > thr - off - tol).sum((1, 2))], 1)
        self.box_sure = [box_of(m) for m in self.sure]
        self.box_poss = [box_of(m) for m in self.poss]
        und = (~self.decided).sum((1, 2)) + (self.inter[:, 1] - self.inter[:, 0]) + (self.union[:, 1] - self.union[:, 0])
        self.undecided_share = und / float(H * W)

    def take(self, idx):
        """the bounds of a sub-batch (candidates idx of this one)"""
        idx = list(idx)
        b = object.__new__(Bounds)
        b.ref, b.tol, b.off, b.thr = self.ref[idx], self.tol, self.off, self.thr
        b.sure, b.poss, b.decided = self.sure[idx], self.poss[idx], self.decided[idx]
        b.inter, b.union = self.inter[idx], self.union[idx]
        b.box_sure, b.box_poss = [self.box_sure[i] for i in idx], [self.box_poss[i] for i in idx]
        b.undecided_share = self.undecided_share[idx]
        return b


def stability_admissible(s, inter, union):
    """is float32 s the quotient float32(i) / float32(u) of SOME pair with inter[0] <= i <= inter[1], union[0] <= u <= union[1]
    (0/0 = NaN)?  Exact when both intervals are points; otherwise every u of its interval is tried with the i nearest s u."""
    s = F32(s)
    if np.isnan(s):
        return inter[0] == 0 and union[0] == 0
    u = np.arange(max(int(union[0]), 1), int(union[1]) + 1, dtype=np.int64)
    if not len(u):
        return False
    near = np.rint(np.float64(s) * u).astype(np.int64)
    for d in (-1, 0, 1):
        i = near + d
        ok = (i >= inter[0]) & (i <= inter[1]) & (i >= 0)
        if (ok & ((i.astype(F32) / u.astype(F32)) == s)).any():
            return True
    return False


def check_outputs(b, names, masks, boxes, stab, keep, iou, p):
    """The four production outputs of one call against the bounds b of its batch -> list of (pattern, quantity, detail ...),
    empty when every output is admissible.  masks uint8 [K,H,W], boxes [K,4], stab float32 [K], keep uint8 [K], iou the
    predictions handed to the call, p its Params."""
    K, H, W = b.ref.shape
    masks, boxes, stab, keep = np.asarray(masks), np.asarray(boxes).astype(np.int64), np.asarray(stab, dtype=F32), np.asarray(keep)
    assert masks.shape == (K, H, W) and boxes.shape == (K, 4) and stab.shape == (K,) and keep.shape == (K,)
    alive = passes_iou(iou, p.iou_thr)
    bad = []
    for k, n in enumerate(names):
        if b.undecided_share[k] > UNDECIDED_CAP:
            bad.append((n, "undecided share", float(b.undecided_share[k])))
        m = masks[k]
        if m.max() > 1:
            bad.append((n, "mask value", int(m.max())))
        if not alive[k]:                        # filtered before any pixel work: zero mask, stability 0, empty box, keep 0
            if m.any():
                bad.append((n, "filtered mask", int((m != 0).sum())))
            if not stab[k] == 0:
                bad.append((n, "filtered stability", float(stab[k])))
            if boxes[k].any():
                bad.append((n, "filtered box", boxes[k].tolist()))
            if keep[k] != 0:
                bad.append((n, "filtered keep", int(keep[k])))
            continue
        wrong = ((m != 0) != b.sure[k]) & b.decided[k]
        if wrong.any():
            ys, xs = np.nonzero(wrong)
            bad.append((n, "mask", int(wrong.sum()), (int(ys[0]), int(xs[0]))))
        if not stability_admissible(stab[k], b.inter[k], b.union[k]):
            bad.append((n, "stability", float(stab[k]), b.inter[k].tolist(), b.union[k].tolist()))
        # the box: that of the mask which came with it, and edge by edge between the surely-on and the possibly-on pixels
        own = box_of(m != 0)
        got = tuple(boxes[k].tolist())
        if got != (own or (0, 0, 0, 0)):
            bad.append((n, "box of its own mask", got, own))
        lo, hi = b.box_sure[k], b.box_poss[k]
        if hi is None:
            ok = got == (0, 0, 0, 0)
        elif lo is None:                        # only undecided pixels: empty, or any box inside theirs
            ok = got == (0, 0, 0, 0) or (hi[0] <= got[0] <= got[2] <= hi[2] and hi[1] <= got[1] <= got[3] <= hi[3])
        else:
            ok = (hi[0] <= got[0] <= lo[0] and hi[1] <= got[1] <= lo[1] and lo[2] <= got[2] <= hi[2] and lo[3] <= got[3] <= hi[3])
        if not ok:
            bad.append((n, "box", got, lo, hi))
        with np.errstate(invalid="ignore"):
            want = 1 if (not p.stab_thr > 0 or stab[k] >= F32(p.stab_thr)) else 0
        if keep[k] != want:
            bad.append((n, "keep", int(keep[k]), want, float(stab[k])))
    return bad


def outputs_from_logits(full, iou, p, thr=MASK_THRESHOLD):
    """What the operation derives from full-resolution logits `full` [K,H,W] (any float type; the comparisons are made in its
    own precision against float32 thresholds, as the kernels make them) -> (masks u8, boxes i64 [K,4], stab f32, keep u8)."""
    full = np.asarray(full)
    K = len(full)
    alive = passes_iou(iou, p.iou_thr)
    t, off = F32(thr), F32(p.off)
    masks = ((full > t) & alive[:, None, None]).astype(np.uint8)
    inter = (full > F32(t + off)).sum((1, 2))
    union = (full > F32(t - off)).sum((1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        stab = np.where(alive, inter.astype(F32) / union.astype(F32), F32(0)).astype(F32)
    boxes = np.array([box_of(m) or (0, 0, 0, 0) for m in masks], dtype=np.int64).reshape(K, 4)
    with np.errstate(invalid="ignore"):
        keep = (alive & ((not p.stab_thr > 0) | (stab >= F32(p.stab_thr)))).astype(np.uint8)
    return masks, boxes, stab, keep
