"""The entries of the clean-up of encoded sets (csrc/rle_clean.hip: hgl_rle_clean_device, hgl_rle_clean_workspace_bytes):
declared, bound, exported, the ABI version still 7; the parameter lists against the ctypes signatures; the refusal without a
device; every HGL_EINVAL of the contract through rle_clean_plan (csrc/rle_group.h), the one place the entry validates in --
compiled as the stand-alone program tests/native/rle_clean_sanitize.cpp, without a sanitizer here -- against
tests/rle_clean_cases.py; the workspace query against the same arithmetic in Python; ops.rle_clean_layout."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import rle_clean_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hgl_rle_clean_device"
QUERY = "hgl_rle_clean_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle_clean.hip")).read()
    raw = C.CDLL(lib._name)

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "double": C.c_double, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    names = {}
    for name, res_c, res in ((NAME, "int", C.c_int), (QUERY, "size_t", C.c_size_t)):
        assert re.search(r"\b" + name + r"\s*\(", code)
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and getattr(raw, name) is not None
        decl = [" ".join(a.split()) for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
        got_res, args = _lib.PROTOTYPES[name]
        assert got_res is res and [kind(a) for a in decl] == list(args)
        defn = [" ".join(a.split()) for a in re.search(r"\b" + res_c + " " + name + r"\s*\(([^)]*)\)\s*\{", src).group(1).split(",")]
        assert defn == decl      # the definition takes the same list
        names[name] = [a.rsplit(" ", 1)[1].lstrip("*") for a in decl]
    assert names[NAME] == ["slots", "slot_words", "table", "S", "images_host", "G", "area_thresh", "modes", "seg_cap", "out_slots",
                           "out_slot_words", "out_table", "boxes_xyxy", "result", "ws", "ws_bytes", "stream"]
    assert names[QUERY] == ["images_host", "G", "S", "slot_words", "seg_cap"]
    # next to the compaction in the header, in the Makefile's sources, and no new version
    assert code.index("hgl_rle_select_device") < code.index(QUERY) < code.index(NAME)
    mk = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\brle_clean\.hip\b", mk, flags=re.M)
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = np.asarray([[70, 37, 0]], dtype=np.int64)
    assert lib.hgl_rle_clean_device(None, 4, None, 0, a.ctypes.data, 1, 20, 3, 100, None, 4, None, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_every_einval_of_the_contract_through_the_plan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "the plan is checked as a compiled program: g++ is needed"
    exe = tmp_path / "rle_clean_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "rle_clean_sanitize.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    images, S = RC.packed(RC.SIZES, RC.N)
    good = [RC.case(images, S), RC.case(images, S, sw=0, osw=0, thresh=0, modes=1, cap=1), RC.case(images, S, modes=2, cap=(1 << 31) - 1),
            RC.case([[5, 5, 0]], 0)]
    todo = good + [c for _, c in RC.refusals()]
    path = tmp_path / "cases.txt"
    path.write_text("".join(RC.line_of(c) + "\n" for c in todo))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and len(lines) == len(todo), r.stderr[-2000:]
    for c, line in zip(good, lines):
        assert RC.want_of(c) is not None and line.startswith("0 "), line
    seen = set()
    for (why, c), line in zip(RC.refusals(), lines[len(good):]):
        assert RC.want_of(c) is None and line.startswith("-1 ") and why in line, (why, line)
        seen.add(why)
    # one per rule: the group at either end, the set, the sizes, the entries, the per-image limit, the plane words, either slot
    # size at either end, the threshold, the modes at either end, the segment limit at either end
    assert len(seen) == 16


def test_the_workspace_query_is_the_arithmetic_of_the_header(lib):
    images, S = RC.packed(RC.SIZES, RC.N)
    a = np.asarray(images, dtype=np.int64)
    for sw, cap in ((8, 100), (0, 1), (2049, 1 << 20), (77, (1 << 31) - 1)):
        got = lib.hgl_rle_clean_workspace_bytes(a.ctypes.data, len(images), S, sw, cap)
        assert got == RC.workspace_bytes(images, S, sw, cap) > 0, (sw, cap, got)
    # O(bit planes + S * seg_cap) words: at the segment limit of packed form-0 rows, far below one byte per pixel
    one = np.asarray([[640, 640, 0]], dtype=np.int64)
    got = lib.hgl_rle_clean_workspace_bytes(one.ctypes.data, 1, 64, 512, 512 // 2 + 640 + 1)
    assert 0 < got == RC.workspace_bytes([[640, 640, 0]], 64, 512, 897) < 64 * 640 * 640 // 4
    # 0 for S = 0, for a refused geometry and for a refused limit
    assert lib.hgl_rle_clean_workspace_bytes(a.ctypes.data, len(images), 0, 8, 100) == 0
    assert lib.hgl_rle_clean_workspace_bytes(a.ctypes.data, len(images), S - 513, 8, 100) == 0
    assert lib.hgl_rle_clean_workspace_bytes(a.ctypes.data, len(images), S, 8, 0) == 0
    assert lib.hgl_rle_clean_workspace_bytes(a.ctypes.data, len(images), S, -1, 100) == 0
    assert lib.hgl_rle_clean_workspace_bytes(None, 1, 4, 8, 100) == 0


def test_clean_layout_and_the_wrappers_refusals():
    images = ops.rle_clean_layout([(70, 37), (64, 64), (512, 640), (3, 50)], [3, 0, 5, 1])
    assert images.dtype == np.int64 and images.tolist() == [[70, 37, 0], [64, 64, 3], [512, 640, 3], [3, 50, 8]]
    for sizes, counts in [([(4, 4)], [1, 2]), ([(4, 4)], [-1])]:
        with pytest.raises(ValueError):
            ops.rle_clean_layout(sizes, counts)
    assert ops.CLEAN_MODES == {"holes": 1, "islands": 2, "both": 3}
