"""The entries of the device mask merge (csrc/rle.hip: hgl_rle_merge_device): declared, bound, exported, the ABI version still 7;
the workspace query against the plan arithmetic restated in Python (tests/rle_merge_cases.py), its 0 for every geometry the call
refuses and for S = 0; the refusal without a device; ops.rle_merge_rule for every name and its refusals; and the golden file
tests/golden/rle_merge_fuzz.npz pinned without a GPU: every stored count list of the reference's rleMerge is re-derived from a
dense numpy OR / AND of the stored masks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import rle_merge_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_merge_workspace_bytes", "hgl_rle_merge_device"]
GOOD = [[70, 37, 0, 0], [64, 64, 3, 2], [512, 640, 3, 2], [3, 50, 8, 5]]      # Ssrc = 9: 3 + 0 + 5 + 1; S = 5: 2 + 0 + 3 + 0


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arr(images):
    return np.asarray(images, dtype=np.int64).reshape(-1, 4)


def bad_geometries():
    """(images, Ssrc, S, M) the call refuses"""
    def edit(g, col, v):
        im = [list(r) for r in GOOD]
        im[g][col] = v
        return im
    return {"G = 0": ([], 9, 5, 3), "G = 65": ([[4, 4, 0, 0]] * 65, 0, 1, 0), "source entries step back": (edit(2, 2, 2), 9, 5, 3),
            "output entries step back": (edit(3, 3, 1), 9, 5, 3), "first source entry not 0": (edit(0, 2, 1), 9, 5, 3),
            "first output entry not 0": (edit(0, 3, 1), 9, 5, 3), "source entries beyond Ssrc": (GOOD, 7, 5, 3),
            "output entries beyond S": (GOOD, 9, 4, 3), "H*W = 2^31": (edit(1, 0, 1 << 25), 9, 5, 3), "H = 0": (edit(0, 0, 0), 9, 5, 3),
            "W < 0": (edit(0, 1, -3), 9, 5, 3), "Ssrc < 0": (GOOD[:1], -1, 1, 0), "M < 0": (GOOD, 9, 5, -1),
            "source plane words": ([[64, 1 << 20, 0, 0]], 1 << 12, 1, 1), "merged plane words": ([[64, 1 << 20, 0, 0]], 1, 1 << 12, 1)}


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert getattr(raw, name) is not None, name
    decl = lambda name: [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    kind = lambda a: "p" if "*" in a else ("ll" if a.startswith("long long") else ("sz" if a.startswith("size_t") else "i"))
    ctype = {"p": C.c_void_p, "ll": C.c_longlong, "sz": C.c_size_t, "i": C.c_int}
    for name in NEW:
        res, args = _lib.PROTOTYPES[name]
        assert [ctype[kind(a)] for a in decl(name)] == list(args), name
    assert _lib.PROTOTYPES[NEW[0]][0] is C.c_size_t and _lib.PROTOTYPES[NEW[1]][0] is C.c_int
    assert len(decl(NEW[0])) == 6 and len(decl(NEW[1])) == 18
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_workspace_query(lib):
    def q(images, Ssrc, sw, S, M):
        a = arr(images)      # alive until the call has returned
        return lib.hgl_rle_merge_workspace_bytes(a.ctypes.data, len(images), Ssrc, sw, S, M)

    for sw in (0, 1, 40, 12800):
        want = MC.workspace_bytes(GOOD, 9, sw, 5, 7)
        assert want > 0 and q(GOOD, 9, sw, 5, 7) == want
    # by hand: 3 entries of 70 x 37 (2 words per column), 5 of 512 x 640 (8), 1 of 3 x 50 (1) -> source planes; 2 + 3 merged
    up = lambda n: (n + 255) // 256 * 256
    words_src, words_out = 3 * 37 * 2 + 5 * 640 * 8 + 50, 2 * 37 * 2 + 3 * 640 * 8
    assert q(GOOD, 9, 40, 5, 7) == up(9 * 41 * 4) + up(9 * 16) + up(8 * words_src) + up(8 * words_out)
    one = [[1, 1, 0, 0]]
    assert q(one, 1, 1, 1, 70000) == MC.workspace_bytes(one, 1, 1, 1, 70000) == 4 * 256
    assert q(one, 0, 0, 3, 0) == MC.workspace_bytes(one, 0, 0, 3, 0) == 256      # no source entry: three merged words
    many = [[4, 4, g, 2 * g] for g in range(64)]
    assert q(many, 64, 3, 128, 5) == MC.workspace_bytes(many, 64, 3, 128, 5) > 0
    # a geometry the call refuses has no size; neither has a call without an output entry
    for what, (images, Ssrc, S, M) in bad_geometries().items():
        assert MC.plan(images, Ssrc, S, M) is None, what
        a = arr(images) if len(images) else np.zeros((1, 4), np.int64)
        assert lib.hgl_rle_merge_workspace_bytes(a.ctypes.data, len(images), Ssrc, 4, S, M) == 0, what
    assert lib.hgl_rle_merge_workspace_bytes(None, 4, 9, 4, 5, 3) == 0
    assert q(GOOD, 9, -1, 5, 3) == 0
    no_out = [r[:3] + [0] for r in GOOD]
    assert MC.plan(no_out, 9, 0, 0) is not None and q(no_out, 9, 4, 0, 0) == 0


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = arr(GOOD[:1])
    assert lib.hgl_rle_merge_device(None, 4, None, 0, a.ctypes.data, 1, None, 0, None, None, None, 4, None, 0, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_merge_rule():
    for k in (0, 1, 2, 3, 4, 255):
        assert ops.rle_merge_rule("union", k) == (1, max(k, 1))
        assert ops.rle_merge_rule("intersect", k) == (k, k)
        assert ops.rle_merge_rule("majority", k) == (k // 2 + 1, max(k, k // 2 + 1))
        for T in (0, 1, 2, 3, 300):
            assert ops.rle_merge_rule(f"at_least:{T}", k) == (T, max(T, k))
            assert ops.rle_merge_rule(f"exactly:{T}", k) == (T, T)
        # every pair is one the device accepts, and it means what its name says for every possible count
        for name in ("union", "intersect", "majority", "at_least:2", "exactly:1"):
            lo, hi = ops.rle_merge_rule(name, k)
            assert 0 <= lo <= hi
            for count in range(k + 1):
                want = {"union": count >= 1, "intersect": count == k, "majority": 2 * count > k, "at_least:2": count >= 2,
                        "exactly:1": count == 1}[name]
                assert (lo <= count <= hi) == want, (name, k, count)
    for bad in ("", "Union", "or", "at_least", "at_least:", "at_least:-1", "at_least:1.5", "exactly:x", "exactly:1:2", "most:2", None, 3):
        with pytest.raises(ValueError):
            ops.rle_merge_rule(bad, 3)
    with pytest.raises(ValueError):
        ops.rle_merge_rule("union", -1)


def test_merge_layout():
    images = ops.rle_merge_layout([(70, 37), (64, 64), (512, 640), (3, 50)], [3, 0, 5, 1], [2, 0, 3, 0])
    assert images.dtype == np.int64 and images.tolist() == GOOD
    for sizes, cs, co in [([(4, 4)], [1, 2], [1]), ([(4, 4)], [1], [1, 1]), ([(4, 4)], [-1], [1]), ([(4, 4)], [1], [-2])]:
        with pytest.raises(ValueError):
            ops.rle_merge_layout(sizes, cs, co)


def test_golden_is_what_a_dense_or_and_gives():
    cases = MC.golden_cases()
    shapes = sorted({(H, W) for H, W, *_ in cases})
    assert shapes == sorted([(70, 37), (64, 64), (3, 50), (129, 5), (1, 40), (40, 1)])
    assert sorted({m.shape[0] for _, _, m, _, _ in cases}) == [1, 2, 3, 5] and len(cases) == 6 * 4 * 4
    empty = full = first = 0
    for H, W, masks, union, inter in cases:
        assert masks.shape[1:] == (H, W) and set(np.unique(masks).tolist()) <= {0, 1}
        assert MC.counts_of(masks.any(axis=0)).tolist() == union.tolist()
        assert MC.counts_of(masks.all(axis=0)).tolist() == inter.tolist()
        for c in (union, inter):
            assert int(c.sum()) == H * W and not (c[1:] == 0).any()      # canonical: no zero count after index 0
        empty += int((masks.reshape(len(masks), -1).sum(axis=1) == 0).any())
        full += int((masks.reshape(len(masks), -1).sum(axis=1) == H * W).any())
        first += int(masks[:, 0, 0].all())
    assert empty >= 24 and full >= 24 and first >= 24
    assert os.path.getsize(MC.GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "rle_match_fuzz.npz"))
