"""CPU: the library exports hgl_synthesize_views_prompt with the signature the binding declares, the struct has the header's layout,
and the ABI version did not move."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hybridgl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_symbol_signature_and_version(lib):
    from hybridgl_amd import _lib
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7
    fn = lib.hgl_synthesize_views_prompt
    VP, I = C.c_void_p, C.c_int
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [VP, VP, VP, VP, VP, I, I, I, I, C.POINTER(_lib.HglViewPrompt), VP, VP, VP]
    assert hasattr(C.CDLL(lib._name), "hgl_synthesize_views_prompt")
    # the old entry is still there, unchanged
    assert list(lib.hgl_synthesize_views.argtypes) == [VP, VP, VP, VP, I, I, I, I, VP, VP, VP]


def test_struct_follows_the_header():
    """field for field, in order, against the typedef of include/hybridgl.h; natural alignment on both sides"""
    from hybridgl_amd import _lib
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    body = re.search(r"typedef struct HglViewPrompt \{(.*?)\} HglViewPrompt;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(int|float|uint8_t)\s+(\w+)(?:\[(\d)\])?;", body)
    kinds = {"int": C.c_int, "float": C.c_float, "uint8_t": C.c_uint8}
    want = [(name, kinds[t] * int(n) if n else kinds[t]) for t, name, n in decl]
    got = list(_lib.HglViewPrompt._fields_)
    assert [n for n, _ in got] == [n for n, _ in want] and len(got) == 11
    for (_, a), (_, b) in zip(got, want):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_type_", a) == getattr(b, "_type_", b)
    assert C.sizeof(_lib.HglViewPrompt) == 52 and _lib.HglViewPrompt.marker.offset == 40


def test_refuses_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from hybridgl_amd import ops
    rc = lib.hgl_synthesize_views_prompt(None, None, None, None, None, 1, 4, 4, 2, C.byref(ops.view_prompt()), None, None, None)
    assert rc == -2 and b"no HIP device" in lib.hgl_last_error()
