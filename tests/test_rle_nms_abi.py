"""The entries of the mask NMS on encoded sets (csrc/rle.hip: hgl_rle_nms_device): declared, bound, exported, the ABI version still
7; the workspace query against the plan arithmetic restated in Python (tests/rle_nms_cases.py), its 0 for every geometry the call
refuses and for S = 0; the refusal without a device; ops.rle_nms_layout; and the golden file tests/golden/rle_nms_fuzz.npz pinned
without a GPU: every keep vector the reference's rleNms stored is re-derived by a greedy numpy walk over dense float64 ratios of
the stored masks, with no exception -- the proof that the reference is exact on these inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import rle_nms_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_nms_workspace_bytes", "hgl_rle_nms_device"]
GOOD = [[70, 37, 0], [64, 64, 3], [512, 640, 3], [3, 50, 8]]      # S = 9: 3 + 0 + 5 + 1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arr(images):
    return np.asarray(images, dtype=np.int64).reshape(-1, 3)


def bad_geometries():
    """(images, S) the call refuses"""
    def edit(g, col, v):
        im = [list(r) for r in GOOD]
        im[g][col] = v
        return im
    return {"G = 0": ([], 9), "G = 65": ([[4, 4, 0]] * 65, 1), "entries step back": (edit(2, 2, 2), 9),
            "first entry not 0": (edit(0, 2, 1), 9), "entries beyond S": (GOOD, 7), "H*W = 2^31": (edit(1, 0, 1 << 25), 9),
            "H = 0": (edit(0, 0, 0), 9), "W < 0": (edit(0, 1, -3), 9), "S < 0": (GOOD[:1], -1),
            "4097 entries": ([[4, 4, 0]], 4097), "4097 entries in the middle": ([[4, 4, 0], [4, 4, 2], [4, 4, 4099]], 4100),
            "plane words": ([[64, 1 << 20, 0]], 4096)}


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert getattr(raw, name) is not None, name
    decl = lambda name: [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "double": C.c_double, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    for name in NEW:
        res, args = _lib.PROTOTYPES[name]
        assert [kind(a) for a in decl(name)] == list(args), name
    assert _lib.PROTOTYPES[NEW[0]][0] is C.c_size_t and _lib.PROTOTYPES[NEW[1]][0] is C.c_int
    assert len(decl(NEW[0])) == 4 and len(decl(NEW[1])) == 15
    assert decl(NEW[1])[7] == "double thr" and decl(NEW[1])[8] == "int metric"
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_workspace_query(lib):
    def q(images, S, sw):
        a = arr(images)      # alive until the call has returned
        return lib.hgl_rle_nms_workspace_bytes(a.ctypes.data, len(images), S, sw)

    for sw in (0, 1, 40, 12800):
        want = NC.workspace_bytes(GOOD, 9, sw)
        assert want > 0 and q(GOOD, 9, sw) == want
    # by hand: 3 entries of 70 x 37 (2 words per column), 5 of 512 x 640 (8), 1 of 3 x 50 (1); three tiles -> 32 splits of
    # 9 + 25 + 1 pair counts; one suppression word per entry
    up = lambda n: (n + 255) // 256 * 256
    words = 3 * 37 * 2 + 5 * 640 * 8 + 50
    assert q(GOOD, 9, 40) == up(9 * 41 * 4) + 2 * up(9 * 16) + up(8 * words) + up(4 * 32 * 35) + up(4 * 9) + up(8 * 9)
    one = [[1, 1, 0]]
    assert q(one, 1, 1) == NC.workspace_bytes(one, 1, 1) == 7 * 256
    full = [[8, 8, 0]]      # the per-image limit itself: 128 x 64 tiles, one split, 4096 * 64 suppression words
    assert q(full, 4096, 2) == NC.workspace_bytes(full, 4096, 2) == up(4096 * 12) + 2 * up(4096 * 16) + up(8 * 4096 * 8) \
        + 4 * 4096 * 4096 + up(4 * 4096) + 8 * 4096 * 64
    many = [[4, 4, 130 * g] for g in range(64)]
    assert q(many, 64 * 130, 3) == NC.workspace_bytes(many, 64 * 130, 3) > 0
    # a geometry the call refuses has no size; neither has a call without an entry
    for what, (images, S) in bad_geometries().items():
        assert NC.plan(images, S) is None, what
        a = arr(images) if len(images) else np.zeros((1, 3), np.int64)
        assert lib.hgl_rle_nms_workspace_bytes(a.ctypes.data, len(images), S, 4) == 0, what
    assert lib.hgl_rle_nms_workspace_bytes(None, 4, 9, 4) == 0
    assert q(GOOD, 9, -1) == 0
    none = [r[:2] + [0] for r in GOOD]
    assert NC.plan(none, 0) is not None and q(none, 0, 4) == 0


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = arr(GOOD[:1])
    assert lib.hgl_rle_nms_device(None, 4, None, 0, a.ctypes.data, 1, None, 0.5, 0, None, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_nms_layout_and_names():
    images = ops.rle_nms_layout([(70, 37), (64, 64), (512, 640), (3, 50)], [3, 0, 5, 1])
    assert images.dtype == np.int64 and images.tolist() == GOOD
    for sizes, counts in [([(4, 4)], [1, 2]), ([(4, 4)], [-1])]:
        with pytest.raises(ValueError):
            ops.rle_nms_layout(sizes, counts)
    assert ops.NMS_METRIC == {"iou": 0, "containment": 1}


def test_golden_is_what_a_greedy_walk_over_dense_ratios_gives():
    z = NC.golden()
    assert z["shapes"].tolist() == [list(s) for s in NC.SHAPES]
    checked = fell = 0
    for name, H, W, masks, scores in NC.sets("sc"):
        n = len(masks)
        assert masks.shape == (n, H, W) and set(np.unique(masks).tolist()) <= {0, 1} and scores.shape == (n,)
        assert not masks[:, 0].any() and not masks[:, H - 1].any()      # inner: the reference's box pre-filter is tight
        assert np.isnan(scores).sum() == 1 and np.isposinf(scores).sum() == 1 and np.isneginf(scores).sum() == 1
        assert len(np.unique(scores[np.isfinite(scores)])) <= 4      # ties
        inter, area = NC.counts(masks)
        thr, keep, pairs = z[name + "_thr"], z[name + "_keep"], z[name + "_pairs"]
        assert thr[:5].tolist() == NC.BASE_THR and len(thr) == 11 and keep.shape == (11, 2, n)
        for p, (i, j) in enumerate(pairs):      # the exact ratio of a seeded pair, and the double just below it
            r = float(inter[i, j]) / float(area[i] + area[j] - inter[i, j])
            assert 0 < inter[i, j] and thr[5 + 2 * p] == r and thr[6 + 2 * p] == np.nextafter(r, -np.inf) < r
        for t, th in enumerate(thr):
            for o, sc in enumerate((None, scores)):
                kept, _, _ = NC.greedy(inter, area, NC.walk_order(sc, n), float(th), 0)
                want = np.zeros(n, np.uint8)
                want[kept] = 1
                assert np.array_equal(keep[t, o], want), (name, float(th), o)
                checked += 1
                fell += int(n - want.sum())
    assert checked == 8 * 11 * 2 and fell > 1000
    # the chain: entry 1 falls to entry 0 and entry 2 survives because entry 1 fell (5/7 > 0.7 >= 4/8)
    for k, (H, W, n) in enumerate(NC.SHAPES):
        inter, area = NC.counts(z[f"c{k}_masks"])
        assert (area == 6).all() and inter[0, 1] == 5 and inter[0, 2] == 4 and inter[1, 2] == 5
        assert z[f"c{k}_keep"][3, 0, :5].tolist() == [1, 0, 1, 0, 1]                  # thr 0.7
        assert z[f"c{k}_keep"][2, 0, :5].tolist() == [1, 0, 1, 0, 1]                  # thr 0.5: 4/8 is met, not exceeded
        assert z[f"c{k}_keep"][1, 0, :5].tolist() == [1, 0, 0, 0, 1]                  # thr 0.3: 3/9 exceeds it, 2/10 does not
    # an empty mask, a duplicate, a full mask and wrapping runs are in the lists
    for k, (H, W, n) in enumerate(NC.SHAPES):
        s, e = z[f"s{k}_masks"], z[f"e{k}_masks"]
        assert not s[1].any() and np.array_equal(s[0], s[n - 1]) and e[0].all()
        assert n <= 3 or (e[2, H - 1, 0] and e[2, 0, 1])
    assert os.path.getsize(NC.GOLDEN) <= 1 << 19
