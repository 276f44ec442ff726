"""The polygon sets the device rasteriser (csrc/rle_poly.hip) and its walk (csrc/poly_walk.h) are judged on, and what they are
judged by: the 48 vectors of tests/golden/gtmask.npz and the 400 seeded sets of oracle.gen_gtmask_golden.fuzz_cases(), with the
host codec's count image (refer_io.gt_mask_from_polygons, pinned to the reference on the CPU by tests/test_gtmask.py) as the
expected result: count == 1 for rule 0 ("once"), count >= 1 for rule 1 ("any").  Shared by the CPU and the GPU tests; computed
once per process."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ("once", "any")


@functools.lru_cache(maxsize=None)
def cases():
    """[(H, W, polygons)]: the golden vectors, then the fuzz sets -- 448 in all"""
    from oracle import gen_gtmask_golden as GG
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gtmask.npz"))
    out = []
    for i in range(int(gold["n_cases"][0])):
        H, W = (int(v) for v in gold[f"c{i}_size"])
        xy, polys, p = gold[f"c{i}_xy"], [], 0
        for k in gold[f"c{i}_npts"]:
            polys.append(xy[p:p + 2 * int(k)].tolist())
            p += 2 * int(k)
        out.append((H, W, polys))
    out += [(H, W, [list(p) for p in polys]) for H, W, polys in GG.fuzz_cases()[0]]
    return out


def expected(H, W, polygons):
    """(count image [H,W] uint8, the host codec's area) of one polygon set; an empty set is the empty image"""
    from hybridgl_amd import refer_io
    if not polygons:
        return np.zeros((H, W), np.uint8), 0
    return refer_io.gt_mask_from_polygons(polygons, H, W)


def by_rule(count, rule):
    """the mask of a count image under a rule, uint8 0 / 1"""
    return ((count == 1) if rule in (0, "once") else (count >= 1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected_all():
    """[(count image, area)] of cases(), in order"""
    return [expected(H, W, polys) for H, W, polys in cases()]


def golden_40gon():
    """the 480 x 640 case of the golden vectors: a smooth 40-gon and a small triangle"""
    H, W, polys = next(c for c in cases() if (c[0], c[1]) == (480, 640))
    assert len(polys) == 2 and len(polys[0]) == 80
    return H, W, polys
