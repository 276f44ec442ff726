"""CPU: the entries of the device RLE decoder (declared, bound, refusing without a device), the host string parser
hgl_rle_from_string against the reference's vectors and the oracle, and predictions.load on hand-written files."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib
from hybridgl_amd import sam as hsam
from oracle import gen_gtmask_golden as GG
from oracle import gtmask_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_decode_workspace_bytes", "hgl_rle_decode_device", "hgl_rle_iou_workspace_bytes", "hgl_rle_iou_device",
       "hgl_rle_from_string"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def from_string(lib, s, cap=None, null=False):
    """(rc, m, counts written into a buffer of `cap` words followed by 4 guard words)"""
    b = s.encode("ascii") if isinstance(s, str) else s
    m = C.c_longlong(-7)
    if null:
        return lib.hgl_rle_from_string(C.c_char_p(b), None, 0, C.byref(m)), m.value, None
    cap = len(b) if cap is None else cap
    buf = np.full(cap + 4, 0xDEADBEEF, dtype=np.uint32)
    rc = lib.hgl_rle_from_string(C.c_char_p(b), buf.ctypes.data, cap, C.byref(m))
    assert (buf[cap:] == 0xDEADBEEF).all(), "wrote beyond cap"
    return rc, m.value, buf[:cap]


def test_header_declares_and_binding_binds_the_new_entries(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_device_entries_refuse_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert lib.hgl_rle_decode_device(None, 4, None, 1, 4, 4, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()
    assert lib.hgl_rle_iou_device(None, 4, None, None, 4, None, 1, 4, 4, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()
    # the workspace queries are host arithmetic: the run starts (slot_words + 1 words per entry) for the decoder; for the IoU
    # those of both sides, two sets of planes (one 64-bit word per 64 rows of a column) and two status tables
    assert lib.hgl_rle_decode_workspace_bytes(2, 65, 3, 10) >= 2 * 11 * 4
    assert lib.hgl_rle_iou_workspace_bytes(2, 65, 3, 10, 7) >= 2 * (2 * 3 * 2 * 8) + 2 * 11 * 4 + 2 * 8 * 4 + 2 * (2 * 16)
    assert lib.hgl_rle_decode_workspace_bytes(0, 4, 4, 4) == 0


def test_from_string_on_the_reference_vectors(lib, golden_dir):
    gold = np.load(os.path.join(golden_dir, "gtmask.npz"))
    for j, s in enumerate(str(v) for v in gold["r_strings"]):
        rc, m, counts = from_string(lib, s)
        want = gold[f"r{j}_counts"]
        assert rc == 0 and m == len(want) and np.array_equal(counts[:m], want), j
        assert np.array_equal(hsam.rle_counts_from_string(s), want)
        assert np.array_equal(hsam.rle_counts_from_string(s.encode("ascii")), want)


def test_from_string_fuzz_against_the_oracle(lib):
    ref = G.RefMaskApi() if G.have_ref() else None
    for t, mask in enumerate(GG.fuzz_rle_masks()):
        H, W = mask.shape
        rle = hsam.mask_to_rle(mask)
        s = hsam.coco_encode_rle(rle)["counts"]
        rc, m, counts = from_string(lib, s)
        assert rc == 0 and counts[:m].tolist() == rle["counts"], t
        assert counts[:m].tolist() == G.rle_string_to_counts(s), t
        if ref is not None:
            assert np.array_equal(G.counts_to_mask(counts[:m].tolist(), H, W), ref.string_to_mask(s, H, W)), t


def test_from_string_size_query_empty_and_malformed(lib, golden_dir):
    gold = np.load(os.path.join(golden_dir, "gtmask.npz"))
    s, want = str(gold["r_strings"][0]), gold["r0_counts"]
    n = len(want)
    assert n > 3
    assert from_string(lib, s, null=True)[:2] == (0, n)
    rc, m, counts = from_string(lib, s, cap=n - 1)      # one too small: the true count, the first n - 1 written
    assert (rc, m) == (0, n) and np.array_equal(counts, want[:n - 1])
    rc, m, counts = from_string(lib, s, cap=0)
    assert (rc, m) == (0, n)
    assert from_string(lib, "")[:2] == (0, 0) and from_string(lib, "", null=True)[:2] == (0, 0)
    assert len(hsam.rle_counts_from_string("")) == 0
    # a continuation bit with nothing behind it; 8 characters in one group
    for bad, msg in (("5o", b"truncated"), ("oooooooo", b"more than 7")):
        rc, m, _ = from_string(lib, bad)
        assert rc == -1 and msg in lib.hgl_last_error(), bad
        with pytest.raises(_lib.HybridGLError):
            hsam.rle_counts_from_string(bad)
    # the old entry reports the same two errors under its own name
    out = np.zeros((4, 4), np.uint8)
    assert lib.hgl_gt_mask_from_rle_string(b"5o", 4, 4, out.ctypes.data, None) == -1
    assert lib.hgl_last_error() == b"gt_mask_from_rle_string: truncated string"
    assert lib.hgl_gt_mask_from_rle_string(b"oooooooo", 4, 4, out.ctypes.data, None) == -1
    assert lib.hgl_last_error() == b"gt_mask_from_rle_string: malformed count (more than 7 characters)"


def _rec(index, sentence, **kw):
    r = {"index": index, "sentence": sentence, "size": [4, 5], "pure": "D", "final": "D", "I": 0, "U": 0, "I_final": 0, "U_final": 0}
    r.update(kw)
    return r


def _write(path, recs):
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


def test_predictions_load(tmp_path):
    from hybridgl_amd import predictions as P
    d = tmp_path / "a"
    d.mkdir()
    _write(d / "masks.rank0.jsonl", [_rec(2, 1), _rec(0, 0), _rec(2, 0)])
    _write(d / "masks.rank1.jsonl", [_rec(1, 1), _rec(1, 0)])
    (d / "other.jsonl").write_text("not read\n")
    got = P.load(str(d))
    assert [(r["index"], r["sentence"]) for r in got] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert got[0] == _rec(0, 0)
    _write(d / "masks.rank1.jsonl", [_rec(1, 1), _rec(2, 0)])
    with pytest.raises(ValueError, match="already occurs"):
        P.load(d)
    for bad in ([4], [4, 0], [4, 5, 6], "4x5", [4.0, 5], [1 << 16, 1 << 16]):
        _write(d / "masks.rank1.jsonl", [_rec(1, 1, size=bad)])
        with pytest.raises(ValueError, match="size"):
            P.load(d)
    r = _rec(1, 1)
    del r["final"]
    _write(d / "masks.rank1.jsonl", [r])
    with pytest.raises(ValueError, match="keys"):
        P.load(d)
    with pytest.raises(FileNotFoundError):
        P.load(tmp_path / "nowhere")
