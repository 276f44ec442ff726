"""Writes tests/golden/rle_nms_fuzz.npz: what the reference's rleNms (refer/external/maskApi.c:98-107 compiled by oracle/Makefile
into oracle/_ref/libmaskapi_ref.so) keeps of seeded mask lists -- the checker of hgl_rle_nms_device.

    python tools/gen_rle_nms_golden.py [OUT.npz]

Per shape k (SHAPES below, (H, W, n)) three lists of n masks, the generator of tools/gen_rle_match_golden.py for the first two:
  s{k}   "inner": the first and last rows are empty, so rleIou's rleToBbox pre-filter is tight (see the docstring of
         gen_rle_match_golden.py) and rleNms is the exact rule
  c{k}   "chain": bar i is the CHAIN_L pixels i .. i + CHAIN_L - 1 of the inner rows read row by row, so neighbours overlap by
         all but one pixel: IoU (L-1)/(L+1) = 5/7, then 4/8, 3/9, 2/10 -- on both sides of the thresholds, 0.5 met exactly.
         Entry i+1 falls to entry i and entry i+2 survives because i+1 fell.
  e{k}   "edge": a full mask and runs that wrap from one column into the next; masks and scores only
with  {tag}{k}_masks [n,H,W] uint8, {tag}{k}_scores [n] float32 (four values, so ties; one NaN, one +inf, one -inf) and, for s and c,
  {tag}{k}_thr  [T] float64   0, 0.3, 0.5, 0.7, 1.0, then for three seeded intersecting pairs the exact double I / U of the pair
                              (equality does not suppress) and the double just below it (it does)
  {tag}{k}_pairs [3,2]        those pairs
  {tag}{k}_keep [T,2,n] uint8 rleNms's keep flags per threshold; [:,0]: the stored order, [:,1]: the list sorted by descending
                              score, the index breaking ties, NaN first (the box NMS's order), flags mapped back to stored indices
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_rle_match_golden import Ref, mask_set  # noqa: E402
from oracle import gtmask_oracle as G  # noqa: E402

# two plane words per column with padding bits, n crosses one 64-row walk block; exactly one word, n crosses the 32-row tile; a few
# rows; a tall narrow image, two walk blocks and a part
SHAPES = [(70, 37, 70), (64, 64, 33), (3, 50, 5), (129, 5, 130)]
BASE_THR = [0.0, 0.3, 0.5, 0.7, 1.0]
CHAIN_L = 6


def chain_set(n, H, W):
    out = np.zeros((n, H, W), np.uint8)
    inner = out[:, 1:H - 1, :].reshape(n, -1)      # a copy when H - 2 rows are not contiguous: written back below
    assert inner.shape[1] >= n + CHAIN_L
    for i in range(n):
        inner[i, i:i + CHAIN_L] = 1
    out[:, 1:H - 1, :] = inner.reshape(n, H - 2, W)
    return out


def scores_for(n, rng):
    s = (rng.integers(0, 4, n) * 0.25).astype(np.float32)
    s[n // 2], s[n // 3], s[n - 1] = np.nan, np.inf, -np.inf
    return s


def walk_order(scores):
    """descending score, the index breaks ties, a NaN ranks above every number"""
    return sorted(range(len(scores)), key=lambda i: (0 if np.isnan(scores[i]) else 1, -float(scores[i]) if not np.isnan(scores[i]) else 0.0, i))


def pair_thresholds(masks, rng):
    flat = masks.reshape(len(masks), -1).astype(np.int64)
    inter = flat @ flat.T
    area = flat.sum(axis=1)
    cand = [(i, j) for i in range(len(masks)) for j in range(i + 1, len(masks)) if 0 < inter[i, j] < area[i] + area[j] - inter[i, j]]
    picks = [cand[int(k)] for k in rng.choice(len(cand), 3, replace=False)]
    thr = []
    for i, j in picks:
        r = float(inter[i, j]) / float(area[i] + area[j] - inter[i, j])
        thr += [r, float(np.nextafter(r, -np.inf))]
    return np.asarray(picks, np.int64), thr


def nms(ref, masks, order, thr):
    R = ref.encode(masks[order])
    keep = np.zeros(len(order), np.uint32)
    ref.lib.rleNms(R, C.c_ulong(len(order)), keep.ctypes.data_as(C.POINTER(C.c_uint)), C.c_double(thr))
    ref.free(R)
    out = np.zeros(len(order), np.uint8)
    out[np.asarray(order)] = keep.astype(np.uint8)
    return out


def build(ref):
    out = {"shapes": np.asarray(SHAPES, dtype=np.int64)}
    for k, (H, W, n) in enumerate(SHAPES):
        rng = np.random.default_rng(2000 + k)
        sets = {"s": mask_set(n, H, W, rng, True), "c": chain_set(n, H, W), "e": mask_set(n, H, W, rng, False)}
        for tag, masks in sets.items():
            scores = scores_for(n, rng)
            out[f"{tag}{k}_masks"], out[f"{tag}{k}_scores"] = masks, scores
            if tag == "e":
                continue
            pairs, extra = pair_thresholds(masks, rng)
            thr = np.asarray(BASE_THR + extra, np.float64)
            orders = [list(range(n)), walk_order(scores)]
            out[f"{tag}{k}_thr"], out[f"{tag}{k}_pairs"] = thr, pairs
            out[f"{tag}{k}_keep"] = np.stack([np.stack([nms(ref, masks, o, float(t)) for o in orders]) for t in thr])
    return out


def main(argv):
    if not G.have_ref():
        raise SystemExit("oracle/_ref/libmaskapi_ref.so is not built (make -C oracle)")
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "rle_nms_fuzz.npz")
    np.savez_compressed(path, **build(Ref()))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
