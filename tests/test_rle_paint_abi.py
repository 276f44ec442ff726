"""The entries of the paint call (csrc/rle_paint.hip: hgl_rle_paint_workspace_bytes, hgl_rle_paint_device): declared, bound,
exported, the ABI version still 7; the parameter lists against the ctypes signatures; the refusal without a device; every
HGL_EINVAL of the contract through rle_paint_plan (csrc/rle_group.h), the one place the entry validates in -- compiled as the
stand-alone program tests/native/rle_paint_sanitize.cpp, without a sanitizer here -- against tests/paint_cases.py; the workspace
query's 0 for refused geometries; ops.rle_paint_layout and ops.rle_paint_style."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import paint_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, QUERY = "hgl_rle_paint_device", "hgl_rle_paint_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    src = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle_paint.hip")).read()

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "double": C.c_double, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    names = {NAME: ["slots", "slot_words", "table", "S", "order", "style", "K", "images_host", "G", "base", "out", "canvas_pixels",
                    "labels", "status", "ws", "ws_bytes", "stream"],
             QUERY: ["images_host", "G", "S", "slot_words", "K", "canvas_pixels"]}
    for name, res_c, res in ((NAME, "int", C.c_int), (QUERY, "size_t", C.c_size_t)):
        assert re.search(r"\b" + name + r"\s*\(", code)
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and getattr(raw, name) is not None
        decl = [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
        got_res, args = _lib.PROTOTYPES[name]
        assert got_res is res and [kind(a) for a in decl] == list(args)
        assert [a.rsplit(" ", 1)[1].lstrip("*") for a in decl] == names[name]
        # the definition takes the same list
        defn = [" ".join(a.split()) for a in re.search(r"\b" + res_c + " " + name + r"\s*\(([^)]*)\)\s*\{", src).group(1).split(",")]
        assert defn == decl
    decl = [a.strip() for a in re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    assert decl[4] == "const int32_t* order" and decl[5] == "const uint32_t* style" and decl[7] == "const int64_t* images_host"
    assert decl[9] == "const uint8_t* base" and decl[11] == "long long canvas_pixels"
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7
    # the file is built through the Makefile, with its headers as prerequisites
    make = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\brle_paint\.hip\b", make, re.M) and re.search(r"^build/rle_paint\.o .*rle_group\.h rle_scan\.h", make, re.M)
    # the blend's function binds the contraction whatever the command line says
    body = src[src.index("uint32_t paint_blend("):]
    assert body[:body.index("\n}")].split("{", 1)[1].lstrip().startswith("#pragma clang fp contract(off)")


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = np.asarray([[70, 37, 0, 0, 0]], dtype=np.int64)
    assert lib.hgl_rle_paint_device(None, 4, None, 0, None, None, 0, a.ctypes.data, 1, None, None, 70 * 37, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_every_einval_of_the_contract_through_the_plan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "the plan is checked as a compiled program: g++ is needed"
    exe = tmp_path / "rle_paint_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "rle_paint_sanitize.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    images, S, K, total = PC.plan_packed(PC.PLAN_SIZES, PC.PLAN_N, PC.PLAN_M)
    good = [PC.plan_case(images, S, K), PC.plan_case(images, S, K, base=0, out=0),
            PC.plan_case(PC.plan_packed(PC.PLAN_SIZES, [0] * 8, PC.PLAN_M)[0], 0, K),               # no entry: every position is code 3
            PC.plan_case(PC.plan_packed(PC.PLAN_SIZES, PC.PLAN_N, [0] * 8)[0], S, 0, sw=0),         # no position: plain copies
            PC.plan_case([[5, 5, 0, 0, 3]], 0, 0, canvas=29)]
    todo = good + [c for _, c in PC.plan_refusals()]
    path = tmp_path / "cases.txt"
    path.write_text("".join(PC.plan_line_of(c) + "\n" for c in todo))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and len(lines) == len(todo), r.stderr[-2000:]
    for c, line in zip(good, lines):
        assert PC.plan_want_of(c) is not None and line.startswith("0 "), line
    seen = set()
    for (why, c), line in zip(PC.plan_refusals(), lines[len(good):]):
        assert PC.plan_want_of(c) is None and line.startswith("-1 ") and why in line, (why, line)
        seen.add(why)
    # one per rule: the group at either end, S, K, the slot size at either end, the canvas size, a size of 0 and one too large,
    # entries (a step back, beyond S, a first entry that is not 0), list positions (the same three), a canvas outside at either
    # end, two that overlap, the plane words, the tiles, out over base from either side
    assert len(PC.plan_refusals()) == 22 and len(seen) == 19


def test_the_workspace_query_returns_0_for_refused_geometries(lib):
    images, S, K, total = PC.plan_packed(PC.PLAN_SIZES, PC.PLAN_N, PC.PLAN_M)
    ask = lambda c: lib.hgl_rle_paint_workspace_bytes(np.asarray(c["images"], dtype=np.int64).reshape(-1, 5).ctypes.data
                                                      if c["images"] else None, len(c["images"]), c["S"], c["sw"], c["K"], c["canvas"])
    c = PC.plan_case(images, S, K, sw=8)
    (tiles, words, blocks), _ = PC.plan_want_of(c)
    up = lambda n: (n + 255) // 256 * 256
    assert ask(c) == up(K * 9 * 4) + up(words * 8)      # a row of run starts and the planes of every list position
    for why, c in PC.plan_refusals():
        if "out overlaps base" in why:      # where the buffers lie is the call's business, not the query's
            assert ask(c) > 0
        else:
            assert ask(c) == 0, why
    assert lib.hgl_rle_paint_workspace_bytes(None, 1, 0, 8, 1, 10) == 0


def test_paint_layout_style_and_block():
    images, total = ops.rle_paint_layout([(70, 37), (64, 64), (3, 5)], [3, 0, 5], [2, 1, 0])
    assert images.dtype == np.int64 and total == 70 * 37 + 64 * 64 + 15
    assert images.tolist() == [[70, 37, 0, 0, 0], [64, 64, 3, 2, 2590], [3, 5, 3, 3, 2590 + 4096]]
    assert images.tolist() == PC.layout([(70, 37), (64, 64), (3, 5)], [3, 0, 5], [2, 1, 0])[0]
    for sizes, counts, oc in [([(4, 4)], [1, 2], [1]), ([(4, 4)], [1], [1, 1]), ([(4, 4)], [-1], [0]), ([(4, 4)], [1], [-2])]:
        with pytest.raises(ValueError):
            ops.rle_paint_layout(sizes, counts, oc)
    for kw in (dict(fill=(1, 2, 3)), dict(fill=(255, 0, 9), a=0.5, b=-2.0, outline=(4, 5, 6)), dict(outline=(0, 0, 0)), dict()):
        assert ops.rle_paint_style(**kw).tolist() == PC.style_row(**kw).tolist()
    row = ops.rle_paint_style(fill=(0x12, 0x34, 0x56), a=1.0, b=0.7, outline=(1, 2, 3))
    assert row.dtype == np.uint32 and row[0] == 0x03123456 and row[3] == 0x010203
    assert row[1:3].view(np.float32).tolist() == [1.0, float(np.float32(0.7))]
    # the status is a tensor of its own, so the table of flat-buffer layouts is the one tests/test_rle_layout_host.py restates
    assert "paint" not in ops.RLE_BLOCKS
