"""Writes tests/golden/rle_merge_fuzz.npz: what the reference's mask API (refer/external/maskApi.c compiled by oracle/Makefile
into oracle/_ref/libmaskapi_ref.so) says of seeded mask lists merged into one -- the checker of hgl_rle_merge_device.

    python tools/gen_rle_merge_golden.py [OUT.npz]

Cases in the order shape of SHAPES x n of MEMBERS x variant of VARIANTS; few arrays, so that the file stays small:
  m{k}_{n}                     np.packbits of the members [VARIANTS,n,H,W] of shape k (encoded by the reference's own rleEncode)
  union, inter                 the counts of rleMerge(R, M, n, 0) / rleMerge(R, M, n, 1) of all cases back to back, uint32
  union_len, inter_len         how many of them every case owns
Variants: 0 seeded shapes and noise; 1 the same with an empty member; 2 with a full member; 3 every member has pixel (0,0) set.
Every stored count list is canonical (no zero count after index 0): rleMerge emits zero-length runs only for inputs that hold
them, and rleEncode writes none.  The tool asserts it and skips nothing.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gtmask_oracle as G  # noqa: E402

# two words per column with padding bits; exactly one word; a few rows; a tall narrow image; one row; one column
SHAPES = [(70, 37), (64, 64), (3, 50), (129, 5), (1, 40), (40, 1)]
MEMBERS = [1, 2, 3, 5]
VARIANTS = 4


def members(n, H, W, rng, variant):
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
        else:
            out[i] = (rng.random((H, W)) < (0.3 if kind == 2 else 0.9)).astype(np.uint8)
    if variant == 1:
        out[int(rng.integers(0, n))] = 0
    elif variant == 2:
        out[int(rng.integers(0, n))] = 1
    elif variant == 3:
        out[:, 0, 0] = 1
    return out


def merge(lib, R, n, intersect):
    M = G._RLE()
    lib.rleMerge(R, C.byref(M), C.c_ulong(n), C.c_int(intersect))
    counts = np.asarray([M.cnts[j] for j in range(M.m)], dtype=np.uint32)
    lib.rleFree(C.byref(M))
    return counts


def build(lib):
    out = {"shapes": np.asarray(SHAPES, dtype=np.int64), "members": np.asarray(MEMBERS, dtype=np.int64),
           "variants": np.asarray(VARIANTS, dtype=np.int64)}
    counts = {"union": [], "inter": []}
    for k, (H, W) in enumerate(SHAPES):
        for n in MEMBERS:
            sets = []
            for variant in range(VARIANTS):
                rng = np.random.default_rng(7000 + 100 * k + 10 * n + variant)
                masks = members(n, H, W, rng, variant)
                sets.append(masks)
                R = (G._RLE * n)()
                col = np.ascontiguousarray(masks.transpose(0, 2, 1), dtype=np.uint8)      # column-major, mask after mask
                lib.rleEncode(R, col.ctypes.data_as(C.POINTER(C.c_ubyte)), C.c_ulong(H), C.c_ulong(W), C.c_ulong(n))
                for name, intersect in (("union", 0), ("inter", 1)):
                    c = merge(lib, R, n, intersect)
                    assert int(c.sum()) == H * W and not (c[1:] == 0).any(), (k, n, variant, name, c)
                    counts[name].append(c)
                for r in R:
                    lib.rleFree(C.byref(r))
            out[f"m{k}_{n}"] = np.packbits(np.stack(sets).reshape(-1))
    for name, lists in counts.items():
        out[name] = np.concatenate(lists).astype(np.uint32)
        out[name + "_len"] = np.asarray([len(c) for c in lists], dtype=np.int64)
    return out


def main(argv):
    if not G.have_ref():
        raise SystemExit("oracle/_ref/libmaskapi_ref.so is not built (make -C oracle)")
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "rle_merge_fuzz.npz")
    np.savez_compressed(path, **build(G.RefMaskApi().lib))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
