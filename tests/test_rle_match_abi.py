"""CPU: the entries of the device RLE matcher (declared, bound, exported, refusing without a device, the workspace query's
arithmetic) and the fixture tests/golden/rle_match_fuzz.npz (tools/gen_rle_match_golden.py: the reference's rleIou matrices and
rleArea(rleMerge(.., intersect)) counts of seeded mask sets), re-derived from a dense count so that it is pinned wherever the
tests run, and compared with the compiled reference itself where oracle/_ref is built."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib
from oracle import gtmask_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_match_workspace_bytes", "hgl_rle_match_device"]
# the shapes and counts at which I / D in float64 was found equal to rleIou's double on every pair
SHAPES = [(70, 37, 19, 23), (64, 64, 17, 33), (3, 50, 3, 5), (129, 5, 40, 9)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rle_match_fuzz.npz"))


def dense(a, b):
    """(I [na,nb], area_a [na], area_b [nb]) in int64"""
    A, B = a.reshape(len(a), -1).astype(np.int64), b.reshape(len(b), -1).astype(np.int64)
    return A @ B.T, A.sum(1), B.sum(1)


def ratio(I, area_a, area_b, crowd):
    """I / D in float64 from the exact integers: D = area(a) under a crowd flag, the union elsewhere; 0 where D is 0"""
    D = np.where(np.asarray(crowd, bool)[None, :], area_a[:, None] + 0 * area_b[None, :], area_a[:, None] + area_b[None, :] - I)
    return np.where(D > 0, I / np.maximum(D, 1), 0.0)


def test_header_declares_library_exports_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert getattr(raw, name) is not None, name
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7
    # grouped from the start: no single-size twin
    assert not re.search(r"\bhgl_rle_match_(one|single)\w*\s*\(", code)


def test_workspace_query(lib):
    images = np.asarray([[70, 37, 0, 0, 0], [64, 64, 19, 23, 19 * 23]], dtype=np.int64)
    Sa, Sb, swa, swb = 19 + 17, 23 + 33, 10, 7
    words_a, words_b = 19 * 37 * 2 + 17 * 64, 23 * 37 * 2 + 33 * 64
    # 2 tiles: each is split over 32 workgroups, every one with a plane of partial counts of its own
    partial = 4 * 32 * (19 * 23 + 17 * 33)
    floor = 8 * (words_a + words_b) + 4 * (Sa * (swa + 1) + Sb * (swb + 1)) + 2 * 16 * (Sa + Sb) + partial
    with_m = lib.hgl_rle_match_workspace_bytes(images.ctypes.data, 2, Sa, swa, Sb, swb, 1)
    without = lib.hgl_rle_match_workspace_bytes(images.ctypes.data, 2, Sa, swa, Sb, swb, 0)
    assert floor <= with_m < floor + 9 * 256 and without == with_m
    # a geometry the call refuses has no size; neither has a call without an entry, which needs no workspace
    assert lib.hgl_rle_match_workspace_bytes(images.ctypes.data, 2, Sa - 18, swa, Sb, swb, 1) == 0
    assert lib.hgl_rle_match_workspace_bytes(images.ctypes.data, 65, Sa, swa, Sb, swb, 1) == 0
    assert lib.hgl_rle_match_workspace_bytes(None, 2, Sa, swa, Sb, swb, 1) == 0
    none = np.asarray([[70, 37, 0, 0, 0]], dtype=np.int64)
    assert lib.hgl_rle_match_workspace_bytes(none.ctypes.data, 1, 0, swa, 0, swb, 1) == 0


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    images = np.asarray([[70, 37, 0, 0, 0]], dtype=np.int64)
    assert lib.hgl_rle_match_device(None, 4, None, 1, None, 4, None, 1, images.ctypes.data, 1, None, None, 0, None, None, None, 0,
                                    None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_fixture_is_pinned_by_a_dense_count(gold):
    assert [tuple(int(v) for v in r) for r in gold["shapes"]] == SHAPES
    pairs = 0
    for k, (H, W, na, nb) in enumerate(SHAPES):
        for tag in "se":
            a, b = gold[f"{tag}{k}_a"], gold[f"{tag}{k}_b"]
            assert a.shape == (na, H, W) and b.shape == (nb, H, W) and a.max() <= 1 and b.max() <= 1
            I, _, _ = dense(a, b)
            assert np.array_equal(I, gold[f"{tag}{k}_inter"]), (tag, k)
        a, b = gold[f"s{k}_a"], gold[f"s{k}_b"]
        # the input rule of the rleIou comparison: first and last rows empty, so no run wraps and rleToBbox is tight
        assert not a[:, 0].any() and not a[:, -1].any() and not b[:, 0].any() and not b[:, -1].any()
        e_a, e_b = gold[f"e{k}_a"], gold[f"e{k}_b"]
        assert e_a[:, 0].any() and e_a[:, -1].any() and e_b[:, 0].any() and e_b[:, -1].any()
        I, area_a, area_b = dense(a, b)
        crowd = gold[f"s{k}_crowd"]
        assert crowd.shape == (nb,) and 0 < crowd.sum() < nb
        # bit for bit: == on float64, no tolerance
        assert np.array_equal(ratio(I, area_a, area_b, np.zeros(nb)), gold[f"s{k}_iou"]), k
        assert np.array_equal(ratio(I, area_a, area_b, crowd), gold[f"s{k}_iou_crowd"]), k
        pairs += 2 * na * nb
    assert pairs == 2746


def test_fixture_against_the_compiled_reference(gold):
    if not G.have_ref():
        pytest.skip("oracle/_ref is not built here")
    spec = importlib.util.spec_from_file_location("gen_rle_match_golden", os.path.join(ROOT, "tools", "gen_rle_match_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.SHAPES == SHAPES
    fresh = gen.build(gen.Ref())
    assert sorted(fresh) == sorted(gold.files)
    for name in gold.files:
        assert np.array_equal(fresh[name], gold[name]), name
