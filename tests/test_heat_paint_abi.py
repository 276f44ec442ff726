"""The entries of the heat-map painter (csrc/rle_paint.hip: hgl_heat_paint_workspace_bytes, hgl_heat_paint_device): declared,
bound, exported, the ABI version still 7; the parameter lists against the ctypes signatures and the definitions; dir_ramp.h as the
one home of linspace_at / dir_weight and a prerequisite of both objects; the refusal without a device; every HGL_EINVAL of the
contract through heat_paint_plan (csrc/rle_group.h), the one place the entry and the query validate in -- compiled as the
stand-alone program tests/native/heat_paint_sanitize.cpp, without a sanitizer here -- against tests/heat_cases.py; the workspace
query; ops.heat_paint_layout and ops.heat_ramp; render.ramp."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import heat_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybridgl_amd", "csrc")
NAME, QUERY = "hgl_heat_paint_device", "hgl_heat_paint_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    src = open(os.path.join(CSRC, "rle_paint.hip")).read()

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "double": C.c_double, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    names = {NAME: ["heat", "heat_elems", "maps_host", "M", "ramp", "base", "out", "canvas_pixels", "levels", "status", "ws", "ws_bytes",
                    "stream"],
             QUERY: ["maps_host", "M", "heat_elems", "canvas_pixels"]}
    for name, res_c, res in ((NAME, "int", C.c_int), (QUERY, "size_t", C.c_size_t)):
        assert re.search(r"\b" + name + r"\s*\(", code)
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and getattr(raw, name) is not None
        decl = [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
        got_res, args = _lib.PROTOTYPES[name]
        assert got_res is res and [kind(a) for a in decl] == list(args)
        assert [a.rsplit(" ", 1)[1].lstrip("*") for a in decl] == names[name]
        defn = [" ".join(a.split()) for a in re.search(r"\b" + res_c + " " + name + r"\s*\(([^)]*)\)\s*\{", src).group(1).split(",")]
        assert defn == decl
    decl = [a.strip() for a in re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    assert decl[0] == "const float* heat" and decl[2] == "const int64_t* maps_host" and decl[4] == "const uint32_t* ramp"
    assert decl[5] == "const uint8_t* base" and decl[6] == "uint8_t* out" and decl[8] == "uint8_t* levels" and decl[9] == "int32_t* status"
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_dir_ramp_is_shared_and_a_prerequisite_of_both_objects():
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^build/rle_paint\.o .*:.*\bdir_ramp\.h\b", make, re.M) and re.search(r"^build/scoring\.o .*:.*\bdir_ramp\.h\b", make, re.M)
    scoring = open(os.path.join(CSRC, "scoring.hip")).read()
    paint = open(os.path.join(CSRC, "rle_paint.hip")).read()
    shared = open(os.path.join(CSRC, "dir_ramp.h")).read()
    for fn in ("linspace_at", "dir_weight"):
        define = re.compile(r"\bfloat\s+" + fn + r"\s*\(")
        assert len(define.findall(shared)) == 1 and not define.search(scoring) and not define.search(paint)
    assert '#include "dir_ramp.h"' in scoring and '#include "dir_ramp.h"' in paint
    # the functions that hold the pixel rule bind the contraction whatever the command line says, as paint_blend does
    for fn in ("float heat_guided(", "uint32_t at(", "int heat_fold_minmax("):
        body = paint[paint.index(fn):]
        assert body[:body.index("\n}")].split("{", 1)[1].lstrip().startswith("#pragma clang fp contract(off)"), fn


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = np.asarray([[7, 5, 0, 0, 0, 0]], dtype=np.int64)
    assert lib.hgl_heat_paint_device(None, 35, a.ctypes.data, 1, None, None, None, 35, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_every_einval_of_the_contract_through_the_plan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "the plan is checked as a compiled program: g++ is needed"
    exe = tmp_path / "heat_paint_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "heat_paint_sanitize.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    im, heat, total = HC.plan_packed(HC.PLAN_SIZES)
    good = [HC.plan_case(im, heat, total), HC.plan_case(im, heat, total, base=0, out=0),
            HC.plan_case([[7, 64, d, 0, 0, 448 * d + d] for d in range(4)]),      # one map under four directions over one base
            HC.plan_case([[5, 5, 2, 3, 9, 3]], heat=28, canvas=29)]
    todo = good + [c for _, c in HC.plan_refusals()]
    path = tmp_path / "cases.txt"
    path.write_text("".join(HC.plan_line_of(c) + "\n" for c in todo))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and len(lines) == len(todo), r.stderr[-2000:]
    for c, line in zip(good, lines):
        assert HC.plan_want_of(c) is not None and line.startswith("0 "), line
    seen = set()
    for (why, c), line in zip(HC.plan_refusals(), lines[len(good):]):
        assert HC.plan_want_of(c) is None and line.startswith("-1 ") and why in line, (why, line)
        seen.add(why)
    # one per rule: the group at either end, the heat size, the canvas size at either end, a size of 0, a negative one and one too
    # large, a dirflag on either side, a heat extent outside at either end, a negative base pixel, a canvas outside at either
    # end, two that overlap, out over base from either side
    assert len(HC.plan_refusals()) == 18 and len(seen) == 16


def test_the_workspace_query(lib):
    im, heat, total = HC.plan_packed(HC.PLAN_SIZES)
    ask = lambda c: lib.hgl_heat_paint_workspace_bytes(np.asarray(c["maps"], dtype=np.int64).reshape(-1, 6).ctypes.data
                                                       if c["maps"] else None, len(c["maps"]), c["heat"], c["canvas"])
    c = HC.plan_case(im, heat, total)
    blocks, _ = HC.plan_want_of(c)
    up = lambda n: (n + 255) // 256 * 256
    assert blocks == 85 and ask(c) == up(blocks * 8) + up(blocks * 4) + up(len(im) * 16)      # (min, max), peak, four words per map
    for why, c in HC.plan_refusals():
        if "out overlaps base" in why:      # where the buffers lie is the call's business, not the query's
            assert ask(c) > 0
        else:
            assert ask(c) == 0, why
    assert lib.hgl_heat_paint_workspace_bytes(None, 1, 10, 10) == 0


def test_layout_and_ramp():
    maps, heat, base, total = ops.heat_paint_layout([(7, 5), (7, 5), (3, 4)], ["left", "right", 3], shared_heat=[0, 0, 1], shared_base=["i", "i", "i2"])
    assert maps.dtype == np.int64 and (heat, base, total) == (47, 47, 82)
    assert maps.tolist() == [[7, 5, 1, 0, 0, 0], [7, 5, 2, 0, 0, 35], [3, 4, 3, 35, 35, 70]]
    maps, heat, base, total = ops.heat_paint_layout([(2, 2), (1, 3)])
    assert maps.tolist() == [[2, 2, 0, 0, 0, 0], [1, 3, 0, 4, 4, 4]] and (heat, base, total) == (7, 7, 7)
    assert HC.plan_want_of(HC.plan_case(maps.tolist(), heat, total)) is not None
    for sizes, kw in [([(4, 4)], dict(dirflags=[0, 1])), ([(0, 4)], {}), ([(4, 4)], dict(dirflags=[4])),
                      ([(4, 4), (4, 5)], dict(shared_base=[0, 0])), ([(4, 4)], dict(shared_heat=[0, 0]))]:
        with pytest.raises(ValueError):
            ops.heat_paint_layout(sizes, **kw)
    rng = np.random.default_rng(0)
    colours, a, b = rng.integers(0, 256, (256, 3)), rng.standard_normal(256).astype(np.float32), np.float32(0.25)
    rows = ops.heat_ramp(colours, a, b)
    assert rows.dtype == np.uint32 and rows.shape == (256, 3) and np.array_equal(rows, HC.ramp_rows(colours, a, b))
    assert rows[5, 0] == (colours[5, 0] << 16 | colours[5, 1] << 8 | colours[5, 2]) and rows[5, 2] == np.float32(0.25).view(np.uint32)
    with pytest.raises(ValueError):
        ops.heat_ramp(colours[:255], a, b)


def test_the_named_ramps():
    from hybridgl_amd import render
    grey = render.ramp("grey")
    assert np.array_equal(grey, HC.grey_ramp())
    heat = render.ramp("heat")
    colours, a, b = HC.ramp_parts(heat)
    assert heat.dtype == np.uint32 and heat.shape == (256, 3)
    assert b[0] == 0 and b[255] == np.float32(0.7) and np.all(np.diff(b) > 0) and np.array_equal(a, (np.float32(1) - b).astype(np.float32))
    # blue -> cyan -> yellow -> red, piecewise linear between the file's stops
    stops = render.HEAT_STOPS
    assert [tuple(c) for _, c in stops] == [(0, 0, 255), (0, 255, 255), (255, 255, 0), (255, 0, 0)] and stops[0][0] == 0 and stops[-1][0] == 255
    for at, c in stops:
        assert tuple(int(v) for v in colours[at]) == tuple(c)
    assert np.all(np.abs(np.diff(colours.astype(int), axis=0)) <= 4)      # no jump between neighbouring levels
    with pytest.raises(ValueError):
        render.ramp("rainbow")
