"""CPU: the ABI entry of the overflow rescue, hgl_split_overflow_snapshot_async (all three fp16 range counters in stream order
into pinned memory).  No GPU here: the entry is declared, bound and exported, and refuses to do anything without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hgl_split_overflow_snapshot_async"


@pytest.fixture(scope="module")
def lib():
    from hybridgl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def header():
    return open(os.path.join(ROOT, "include", "hybridgl.h")).read()


def test_header_declares_the_entry_with_its_contract():
    text = header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*unsigned\s+int\s*\*\s*host3\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    # the contract sits in the comment right above: three words, pinned, stream order, no wait, no reset, the decoder's counter
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("host3[0..2]", "pinned", "STREAM ORDER", "without waiting", "without a reset", "decoder"):
        assert word in comment, word
    # additive: the version the earlier added entries left is the version still
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    # the two-word peek is as it was
    assert re.search(r"\bint\s+hgl_split_overflow_peek_async\s*\(\s*unsigned\s+int\s*\*\s*host2\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)


def test_binding_table_and_library_know_the_entry(lib):
    from hybridgl_amd import _lib
    assert NAME in _lib.PROTOTYPES
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and list(argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.PROTOTYPES[NAME] == _lib.PROTOTYPES["hgl_split_overflow_peek_async"]
    assert hasattr(ctypes.CDLL(lib._name), NAME)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_without_a_device_the_entry_refuses(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    words = (ctypes.c_uint * 3)(7, 7, 7)
    assert lib.hgl_split_overflow_snapshot_async(ctypes.cast(words, ctypes.c_void_p), None) == -2      # HGL_ENODEVICE
    assert b"no HIP device" in lib.hgl_last_error()
    assert list(words) == [7, 7, 7]      # nothing written


def test_null_pointer_is_refused(lib):
    """HGL_EINVAL with a device; without one the device check comes first, as in every entry -- refused either way, and the
    source puts the null check before any copy is enqueued."""
    import torch
    rc = lib.hgl_split_overflow_snapshot_async(None, None)
    assert rc == (-1 if torch.cuda.is_available() else -2)
    src = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "api_core.hip")).read()
    body = src.split("int " + NAME, 1)[1].split("\n}\n", 1)[0]
    assert body.index("HGL_REQUIRE(host3 != nullptr") < body.index("hgl_split_overflow_gemm_peek")
    for unit in ("gemm", "attention", "decoder"):
        assert f"hgl_split_overflow_{unit}_peek(host3" in body


def test_ops_front_end_and_forced_precision_exist_without_a_gpu():
    from hybridgl_amd import ops
    assert callable(ops.split_overflow_snapshot)
    with pytest.raises(ValueError):
        ops.forced_precision("f8")
    assert ops.effective_precision("f16x3") == "f16x3"
