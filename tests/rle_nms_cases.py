"""What the mask NMS on encoded sets (hgl_rle_nms_device) is judged on, plain numpy, no GPU code: the golden file
tests/golden/rle_nms_fuzz.npz (tools/gen_rle_nms_golden.py: the reference's rleNms on seeded lists), the greedy walk over dense
float64 ratios that every result is compared with, the walk order, and rle_nms_plan (csrc/rle_group.h) with the workspace
arithmetic of csrc/rle.hip restated in Python."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rle_nms_fuzz.npz")
SHAPES = [(70, 37, 70), (64, 64, 33), (3, 50, 5), (129, 5, 130)]
BASE_THR = [0.0, 0.3, 0.5, 0.7, 1.0]
NMS_MAX, TA, TB = 4096, 32, 64

_golden = None


def golden():
    """{name: array} of the golden file, loaded once"""
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def sets(tags="sce"):
    """[(name, H, W, masks [n,H,W], scores [n])] of the golden file's lists with one of the tags (s inner, c chain, e edge)"""
    z = golden()
    return [(f"{tag}{k}", H, W, z[f"{tag}{k}_masks"], z[f"{tag}{k}_scores"]) for k, (H, W, n) in enumerate(SHAPES) for tag in tags]


def walk_order(scores, n=None):
    """the order of the walk as a list of indices: the given order without scores; else descending score, the index breaks
    ties, a NaN ranks above every number"""
    if scores is None:
        return list(range(n))
    return sorted(range(len(scores)), key=lambda i: (0, 0.0, i) if math.isnan(scores[i]) else (1, -float(scores[i]), i))


def counts(masks):
    """(inter [n,n] int64, area [n] int64) of a list of dense masks"""
    flat = masks.reshape(len(masks), -1).astype(np.int64)
    return flat @ flat.T, flat.sum(axis=1)


def greedy(inter, area, order, thr, metric=0, dead=()):
    """the contract's walk over dense counts in float64: (kept indices in walk order, rank [n], by [n]); an entry of `dead`
    (code 2) has rank -1, is not kept and suppresses nobody"""
    n = len(area)
    order = [i for i in order if i not in dead]
    kept, rank, by = [], np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for pos, i in enumerate(order):
        rank[i] = pos
        for k in kept:
            if area[i] == 0 or area[k] == 0:
                continue
            I = int(inter[i, k])
            D = int(area[i] + area[k] - I) if metric == 0 else int(min(area[i], area[k]))
            if (0.0 if I == 0 else float(I) / float(D)) > thr:
                by[i] = k
                break
        if by[i] < 0:
            kept.append(i)
    return kept, rank, by


def plan(images, S):
    """rle_nms_plan in Python: None when the geometry is refused, else (tiles, blocks, words, pairs, splits, sup_words) and the
    rows (H, W, first, word0, tile0, blk0, pair0, sup0)"""
    G = len(images)
    if not 1 <= G <= 64 or S < 0:
        return None
    for g, (H, W, e) in enumerate(images):
        e_next = images[g + 1][2] if g + 1 < G else S
        if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31 and H * W < 2 ** 31):
            return None
        if not (0 <= e <= e_next <= S and (g > 0 or e == 0)):
            return None
        if e_next - e > NMS_MAX:
            return None
    tiles = blocks = words = pairs = sup = 0
    rows = []
    for g, (H, W, e) in enumerate(images):
        n = (images[g + 1][2] if g + 1 < G else S) - e
        Q = W * ((H + 63) // 64)
        rows.append((H, W, e, words, tiles, blocks, pairs, sup))
        pairs += n * n
        words += n * Q
        blocks += n * ((Q + 255) // 256)
        tiles += ((n + TA - 1) // TA) * ((n + TB - 1) // TB)
        sup += n * ((n + 63) // 64)
        if words >= 2 ** 32 or blocks >= 2 ** 31 or tiles >= 2 ** 31:
            return None
    splits = min(max((1024 + tiles - 1) // tiles, 1), 32) if tiles else 1
    return (tiles, blocks, words, pairs, splits, sup), rows


def workspace_bytes(images, S, slot_words):
    """hgl_rle_nms_workspace_bytes: run starts, status, boxes, planes, partial counts, order, suppression words"""
    p = plan(images, S)
    if p is None or S <= 0 or slot_words < 0:
        return 0
    (tiles, blocks, words, pairs, splits, sup), _ = p
    up = lambda v: (v + 255) // 256 * 256
    return up(S * (slot_words + 1) * 4) + 2 * up(S * 16) + up(8 * words) + up(4 * splits * pairs) + up(4 * S) + up(8 * sup)
