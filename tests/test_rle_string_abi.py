"""The two entries of the device string codec (csrc/rle_string.hip: hgl_rle_to_strings_device, hgl_rle_from_strings_device):
declared with the reference lines they replace, bound, exported, the ABI version still 7; their parameter lists against the
ctypes signatures and the definitions; the refusal without a device; ops.rle_strings_pack, which is host work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import rle_string_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "hgl_rle_to_strings_device": ["slots", "slot_words", "table", "S", "bytes", "cap", "offsets", "status", "stream"],
    "hgl_rle_from_strings_device": ["bytes", "total_bytes", "offsets", "S", "slots", "slot_words", "table", "status", "stream"],
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle_string.hip")).read()
    raw = C.CDLL(lib._name)

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    for name, params in NAMES.items():
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and getattr(raw, name) is not None
        decl = [" ".join(a.split()) for a in re.search(r"\bint " + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and [kind(a) for a in decl] == list(args)
        assert [a.rsplit(" ", 1)[1].lstrip("*") for a in decl] == params
        defn = [" ".join(a.split()) for a in re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*\{", src).group(1).split(",")]
        assert defn == decl
    assert "int64_t* offsets" in code and "long long cap" in code and "long long total_bytes" in code
    # the comment names what the entries replace and the hazard of the writer
    comment = text[text.index("COCO's compressed RLE strings written and read on the DEVICE"):text.index("int hgl_rle_to_strings_device")]
    for word in ("maskApi.c:203-216", "maskApi.c:217-230", "hgl_rle_to_string", "hgl_rle_from_string", "stores bytes, never words",
                 "THREE launches", "ONE launch"):
        assert word in comment, word
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7
    mk = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "Makefile")).read()
    assert "rle_string.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^build/rle_string.o build/diag/rle_string.o: .*rle_string.h", mk, re.M)


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    off = np.zeros(1, np.int64)
    assert lib.hgl_rle_to_strings_device(None, 4, None, 0, None, 0, off.ctypes.data, None, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()
    assert lib.hgl_rle_from_strings_device(None, 0, off.ctypes.data, 0, None, 4, None, None, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_strings_pack_is_the_contract_s_layout():
    strings = RC.good_strings()[-40:] + [b"", b"", "12".encode(), "0N5"] + [b""]
    buf, offsets, n_counts = ops.rle_strings_pack(strings)
    S = len(strings)
    raw = [s.encode("ascii") if isinstance(s, str) else s for s in strings]
    import torch
    assert buf.dtype == torch.uint8 and buf.is_pinned() == torch.cuda.is_available() and buf.numel() == 8 * (S + 1) + sum(map(len, raw))
    assert offsets.dtype == np.int64 and offsets.tolist() == [0] + np.cumsum([len(s) for s in raw]).tolist()
    assert np.array_equal(buf.numpy()[:8 * (S + 1)].view(np.int64), offsets)
    assert bytes(buf.numpy()[8 * (S + 1):]) == b"".join(raw)
    assert n_counts.tolist() == [len(RC.parse(s)[1]) for s in raw] and n_counts.dtype == np.int64
    b0, o0, n0 = ops.rle_strings_pack([])
    assert b0.numel() == 8 and o0.tolist() == [0] and n0.tolist() == []
    assert ops.rle_strings_pack([b"", b""])[2].tolist() == [0, 0]
    assert ops.rle_strings_pack([b"", b"oo1", b""])[2].tolist() == [0, 1, 0]
    for bad, k in (([b"12", b"3\x004"], 1), (["12", "3é4"], 1), ([b"\x00"], 0)):
        with pytest.raises(ValueError, match=f"entry {k}"):
            ops.rle_strings_pack(bad)
