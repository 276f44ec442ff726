"""The entries of the device polygon rasteriser (csrc/rle_poly.hip): declared, bound, exported, the ABI version still 7; the
workspace query's arithmetic and its 0 for every geometry the call refuses; the refusal without a device; what
ops.rle_from_polygons raises before it uploads anything; the path threshold as the source states it.  With a device (marked
gpu): every refusal of the call itself comes back before a launch and leaves the outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_from_polygons_workspace_bytes", "hgl_rle_from_polygons_device"]
GOOD = np.asarray([[70, 37, 0], [64, 64, 3], [512, 640, 3]], dtype=np.int64)      # S = 5: 3 + 0 + 2 entries


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def lds_words():
    text = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle_group.h")).read()
    return int(re.search(r"constexpr\s+int\s+RLE_POLY_LDS_WORDS\s*=\s*(\d+)\s*;", text).group(1))


def bad_geometries():
    """(images, G, S) the call refuses"""
    def edit(g, col, v):
        im = GOOD.copy()
        im[g, col] = v
        return im
    many = np.tile(np.asarray([[4, 4, 0]], dtype=np.int64), (65, 1))
    return {"G = 0": (GOOD, 0, 5), "G = 65": (many, 65, 0), "entries step back": (edit(2, 2, 2), 3, 5),
            "first entry not 0": (edit(0, 2, 1), 3, 5), "entries beyond S": (GOOD, 3, 2), "H*W = 2^31": (edit(1, 0, 1 << 25), 3, 5),
            "H = 0": (edit(0, 0, 0), 3, 5), "W < 0": (edit(0, 1, -3), 3, 5), "S < 0": (GOOD[:1], 1, -1)}


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert getattr(raw, name) is not None, name
    # the declared parameter lists against the ctypes signatures
    decl = lambda name: [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    kind = lambda a: "p" if "*" in a else ("ll" if a.startswith("long long") else ("sz" if a.startswith("size_t") else "i"))
    ctype = {"p": C.c_void_p, "ll": C.c_longlong, "sz": C.c_size_t, "i": C.c_int}
    for name in NEW:
        res, args = _lib.PROTOTYPES[name]
        assert [ctype[kind(a)] for a in decl(name)] == list(args), name
    assert _lib.PROTOTYPES[NEW[0]][0] is C.c_size_t and _lib.PROTOTYPES[NEW[1]][0] is C.c_int
    assert len(decl(NEW[0])) == 4 and len(decl(NEW[1])) == 15
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_workspace_query(lib):
    L = lds_words()
    assert L == 10240      # 40 KB of LDS: the 480 x 640 plane of 9601 words fits
    words = lambda H, W: (H * W // 32 + 1) * (2 if H * W // 32 + 1 <= L else 3)
    floor = 4 * (3 * words(70, 37) + 2 * words(512, 640))
    got = lib.hgl_rle_from_polygons_workspace_bytes(GOOD.ctypes.data, 3, 5, 9)
    assert floor <= got < floor + 256
    assert 512 * 640 // 32 + 1 == L + 1 and words(512, 640) == 3 * (L + 1)      # the first plane LDS does not hold
    one = np.asarray([[508, 645, 0]], dtype=np.int64)      # the last it does
    assert 508 * 645 // 32 + 1 == L
    assert 8 * L <= lib.hgl_rle_from_polygons_workspace_bytes(one.ctypes.data, 1, 1, 1) < 8 * L + 256
    # a geometry the call refuses has no size; neither has a call without an entry
    for what, (images, G, S) in bad_geometries().items():
        assert lib.hgl_rle_from_polygons_workspace_bytes(images.ctypes.data, G, S, 4) == 0, what
    assert lib.hgl_rle_from_polygons_workspace_bytes(None, 3, 5, 4) == 0
    assert lib.hgl_rle_from_polygons_workspace_bytes(GOOD.ctypes.data, 3, 5, -1) == 0
    assert lib.hgl_rle_from_polygons_workspace_bytes(GOOD[:1].ctypes.data, 1, 0, 0) == 0


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert lib.hgl_rle_from_polygons_device(None, None, 0, None, 0, GOOD.ctypes.data, 1, 0, None, 4, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_ops_raises_before_the_upload():
    # no device is touched: every one of these raises while the polygons are still lists
    sq = [1.0, 1.0, 5.0, 1.0, 5.0, 5.0]
    for entries, sizes, counts, what in [
            ([[[1.0, float("nan"), 5.0, 1.0]]], [(8, 8)], [1], "NaN"),
            ([[sq, [1.0, 1.0e5]]], [(8, 8)], [1], "1e5"),
            ([[sq], [[2.0, -1.0e5, 3.0, 3.0]]], [(8, 8)], [2], "-1e5"),
            ([[sq, []]], [(8, 8)], [1], "coordinates"),
            ([[[1.0, 2.0, 3.0]]], [(8, 8)], [1], "coordinates"),
            ([[sq]], [(8, 8), (9, 9)], [1], "sizes"),
            ([[sq]], [(8, 8)], [2], "counts sum"),
    ]:
        with pytest.raises(ValueError) as e:
            ops.rle_from_polygons(entries, sizes, counts)
        assert what.lower() in str(e.value).lower(), (what, str(e.value))
    with pytest.raises(ValueError):
        ops.rle_from_polygons([[sq]], [(8, 8)], [1], rule="twice")


@pytest.mark.gpu
def test_every_refusal_of_the_call_comes_back_before_a_launch(lib, cuda):
    import torch
    xy = torch.tensor([1.0, 1.0, 20.0, 2.0, 9.0, 30.0], dtype=torch.float64, device=cuda)
    po = torch.tensor([0, 3], dtype=torch.int32, device=cuda)
    ep = torch.tensor([0, 1, 1, 1, 1, 1], dtype=torch.int32, device=cuda)
    S, sw = 5, 40
    out = torch.full((S * (8 + sw),), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    before = out.clone()
    need = lib.hgl_rle_from_polygons_workspace_bytes(GOOD.ctypes.data, 3, S, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    base, stream = out.data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(images=GOOD, G=3, S=S, rule=0, sw=sw, ws_bytes=need, wsp=None):
        return lib.hgl_rle_from_polygons_device(xy.data_ptr(), po.data_ptr(), 1, ep.data_ptr(), S, images.ctypes.data, G, rule,
                                                base + 16 * 5, sw, base, base + 4 * 5 * (4 + 40), ws.data_ptr() if wsp is None else wsp,
                                                ws_bytes, stream)

    for what, (images, G, s) in bad_geometries().items():
        assert call(images=images, G=G, S=s) == -1, what      # HGL_EINVAL
    assert call(sw=0) == -1 and b"slot_words" in lib.hgl_last_error()
    assert call(rule=2) == -1 and b"rule" in lib.hgl_last_error()
    assert call(rule=-1) == -1
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.hgl_last_error()      # HGL_EWORKSPACE
    assert call(wsp=0, ws_bytes=need) == -3
    torch.cuda.synchronize()
    assert torch.equal(out, before)      # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    table = out[:4 * S].reshape(S, 4).cpu().numpy()
    assert table[:, 1].tolist() == [0] * S and table[1:, 0].tolist() == [1] * 4 and table[0, 2] > 0
