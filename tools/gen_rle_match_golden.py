"""Writes tests/golden/rle_match_fuzz.npz: what the reference's mask API (refer/external/maskApi.c compiled by oracle/Makefile
into oracle/_ref/libmaskapi_ref.so) says of seeded mask sets, every mask of one set against every mask of the other --
the checker of hgl_rle_match_device.

    python tools/gen_rle_match_golden.py [OUT.npz]

Per shape k (SHAPES below) two pairs of sets:
  s{k}_a [na,H,W], s{k}_b [nb,H,W]   masks whose first and last rows are empty.  rleIou pre-filters with rleToBbox, whose box is
                                     not tight when a foreground run wraps from one column into the next; with those two rows
                                     empty no run wraps and the box is tight, so rleIou is the exact ratio on every pair.
      s{k}_crowd [nb]                iscrowd flags of set B
      s{k}_iou, s{k}_iou_crowd       rleIou(dt = A, gt = B, iscrowd = 0 / the flags) as [na,nb] float64 (0 where the box filter sees an empty mask)
      s{k}_inter [na,nb] int64       rleArea(rleMerge({a, b}, intersect = 1))
  e{k}_a, e{k}_b, e{k}_inter         masks that touch the first and last rows (full masks, wrapping runs): the merge / area
                                     counts only.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gtmask_oracle as G  # noqa: E402

# (H, W, na, nb): two words per column with padding bits; exactly one word; a few rows; a tall narrow image
SHAPES = [(70, 37, 19, 23), (64, 64, 17, 33), (3, 50, 3, 5), (129, 5, 40, 9)]


def mask_set(n, H, W, rng, inner):
    """n seeded masks: ellipses, rectangles, sparse noise, an empty one, a duplicate; inner: rows 0 and H-1 stay empty"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                cy, cx = rng.random() * H, rng.random() * W
                ry, rx = (0.08 + 0.4 * rng.random()) * H + 0.5, (0.08 + 0.4 * rng.random()) * W + 0.5
                out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
        elif kind == 1:
            y0, y1 = sorted(int(v) for v in rng.integers(0, H + 1, 2))
            x0, x1 = sorted(int(v) for v in rng.integers(0, W + 1, 2))
            out[i, y0:y1 + 1, x0:x1 + 1] = 1
        elif kind == 2:
            out[i] = (rng.random((H, W)) < 0.3).astype(np.uint8)
        else:
            out[i] = (rng.random((H, W)) < 0.9).astype(np.uint8)
    if n > 2:
        out[1] = 0                      # an empty mask
        out[n - 1] = out[0]             # a duplicate: a tie for whoever matches it
    if inner:
        out[:, 0, :] = 0
        out[:, H - 1, :] = 0
    else:
        out[0] = 1                      # a full mask
        if n > 3:
            out[2] = 0
            out[2, H - 1, 0:W - 1] = 1  # runs that wrap from one column into the next
            out[2, 0, 1:W] = 1
    return out


class Ref:
    def __init__(self):
        self.api = G.RefMaskApi()
        self.lib = self.api.lib

    def encode(self, masks):
        n, H, W = masks.shape
        R = (G._RLE * n)()
        col = np.ascontiguousarray(masks.transpose(0, 2, 1), dtype=np.uint8)      # column-major, mask after mask
        self.lib.rleEncode(R, col.ctypes.data_as(C.POINTER(C.c_ubyte)), C.c_ulong(H), C.c_ulong(W), C.c_ulong(n))
        return R

    def free(self, R):
        for r in R:
            self.lib.rleFree(C.byref(r))

    def iou(self, Ra, Rb, crowd):
        m, n = len(Ra), len(Rb)
        o = np.zeros((n, m), np.float64)
        flags = np.ascontiguousarray(crowd, dtype=np.uint8)
        self.lib.rleIou(Ra, Rb, C.c_ulong(m), C.c_ulong(n), flags.ctypes.data_as(C.POINTER(C.c_ubyte)),
                        o.ctypes.data_as(C.POINTER(C.c_double)))
        return o.T.copy()

    def inter(self, Ra, Rb):
        out = np.zeros((len(Ra), len(Rb)), np.int64)
        for i, a in enumerate(Ra):
            for j, b in enumerate(Rb):
                pair = (G._RLE * 2)(a, b)
                M = G._RLE()
                self.lib.rleMerge(pair, C.byref(M), C.c_ulong(2), C.c_int(1))
                area = C.c_uint(0)
                self.lib.rleArea(C.byref(M), C.c_ulong(1), C.byref(area))
                out[i, j] = int(area.value)
                self.lib.rleFree(C.byref(M))
        return out


def build(ref):
    out = {"shapes": np.asarray(SHAPES, dtype=np.int64)}
    for k, (H, W, na, nb) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 + k)
        for tag, inner in (("s", True), ("e", False)):
            a, b = mask_set(na, H, W, rng, inner), mask_set(nb, H, W, rng, inner)
            if nb > 2:
                b[nb - 2] = a[0]        # an identical mask across the sets
            Ra, Rb = ref.encode(a), ref.encode(b)
            out[f"{tag}{k}_a"], out[f"{tag}{k}_b"] = a, b
            out[f"{tag}{k}_inter"] = ref.inter(Ra, Rb)
            if inner:
                crowd = (rng.random(nb) < 0.4).astype(np.uint8)
                out[f"s{k}_crowd"] = crowd
                out[f"s{k}_iou"] = ref.iou(Ra, Rb, np.zeros(nb, np.uint8))
                out[f"s{k}_iou_crowd"] = ref.iou(Ra, Rb, crowd)
            ref.free(Ra)
            ref.free(Rb)
    return out


def main(argv):
    if not G.have_ref():
        raise SystemExit("oracle/_ref/libmaskapi_ref.so is not built (make -C oracle)")
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "rle_match_fuzz.npz")
    np.savez_compressed(path, **build(Ref()))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
