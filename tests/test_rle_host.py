"""CPU: the host side of the device RLE encoder -- the entry refuses without a device, the workspace query, and
sam.rle_from_slot (what turns a slot of hgl_rle_encode_device into counts) against the vectors the reference's maskApi.c
produced (tests/golden/gtmask.npz)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hybridgl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "gtmask.npz"))


def bit_plane(mask):
    """the form-1 slot of a mask, packed by numpy: bit p % 32 of word p / 32 over the column-major order p = x*H + y"""
    flat = (np.asarray(mask) != 0).T.reshape(-1).astype(np.uint8)
    flat = np.concatenate([flat, np.zeros((-len(flat)) % 32, np.uint8)])
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)


def test_device_entry_refuses_without_a_device(lib):
    """HGL_ENODEVICE (-2) before anything else; where a GPU is visible the same null arguments are HGL_EINVAL (-1)"""
    import torch
    rc = lib.hgl_rle_encode_device(None, 1, 4, 4, None, 1, None, 1, None, None, 0, None)
    if torch.cuda.is_available():
        assert rc == -1
    else:
        assert rc == -2
        assert b"no HIP device" in lib.hgl_last_error()


def test_workspace_query_is_positive_and_monotone(lib):
    f = lib.hgl_rle_encode_workspace_bytes
    assert f(1, 1, 1) > 0
    for S, H, W in [(1, 1, 1), (3, 63, 64), (6, 640, 640), (2, 1024, 1024), (7, 129, 65)]:
        here = f(S, H, W)
        assert here >= S * W * ((H + 63) // 64) * 8      # every column of every entry padded to whole 64-bit words
        assert f(S + 1, H, W) >= here and f(S, H + 1, W) >= here and f(S, H, W + 1) >= here
        # the size is rounded up to 256 bytes: strictly larger once the growth exceeds the rounding
        assert f(S + 32, H, W) > here and f(S, H + 64 * 32, W) > here and f(S, H, W + 32) > here


def test_rle_from_slot_form_0_takes_the_counts(lib, gold):
    from hybridgl_amd import sam as hsam
    for j in range(int(gold["n_rle"][0])):
        H, W = (int(v) for v in gold[f"r{j}_size"])
        counts = gold[f"r{j}_counts"]
        slot = np.concatenate([counts, np.full(5, 0xDEADBEEF, np.uint32)])      # words beyond n_counts are not the slot's
        assert hsam.rle_from_slot(slot, len(counts), 0, H, W) == counts.tolist()
        assert hsam.rle_from_slot(slot.view(np.int32), len(counts), 0, H, W) == counts.tolist()      # as the device buffer is typed


def test_rle_from_slot_form_1_unpacks_the_bit_plane(lib, gold):
    from hybridgl_amd import sam as hsam
    strs = [str(s) for s in gold["r_strings"]]
    for j in range(int(gold["n_rle"][0])):
        H, W = (int(v) for v in gold[f"r{j}_size"])
        mask, counts = gold[f"r{j}_mask"], gold[f"r{j}_counts"].tolist()
        slot = np.concatenate([bit_plane(mask), np.full(3, 0xFFFFFFFF, np.uint32)])
        got = hsam.rle_from_slot(slot.view(np.int32), len(counts), 1, H, W)
        assert got == counts
        assert hsam.coco_encode_rle({"size": [H, W], "counts": got}) == {"size": [H, W], "counts": strs[j]}


def test_rle_from_slot_bit_order_on_a_non_square_mask(lib):
    """3 x 2, pixels (1,0) and (0,1) set: p = 1 and p = 3 -> word 0b001010"""
    from hybridgl_amd import sam as hsam
    m = np.zeros((3, 2), np.uint8)
    m[1, 0] = m[0, 1] = 1
    assert bit_plane(m).tolist() == [0b001010]
    assert hsam.rle_from_slot(np.array([0b001010], np.uint32), 5, 1, 3, 2) == [1, 1, 1, 1, 2] == hsam.mask_to_rle(m)["counts"]


def test_rle_from_slot_refuses_the_forms_without_a_mask(lib):
    from hybridgl_amd import sam as hsam
    for form in (2, 3):
        with pytest.raises(ValueError):
            hsam.rle_from_slot(np.zeros(4, np.uint32), 9, form, 8, 8)
