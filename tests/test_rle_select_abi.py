"""The entry of the compaction of an encoded set (csrc/rle.hip: hgl_rle_select_device): declared, bound, exported, the ABI version
still 7; its parameter list against the ctypes signature; the refusal without a device; every HGL_EINVAL of the contract through
rle_select_plan (csrc/rle_group.h), the one place the entry validates in -- compiled as the stand-alone program
tests/native/rle_select_sanitize.cpp, without a sanitizer here -- against tests/rle_select_cases.py; ops.rle_select_layout; and
the numpy statement of the contract (rle_select_cases.select) against a naive loop over the entries."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hybridgl_amd import _lib, ops

import rle_select_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hgl_rle_select_device"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_library_and_bindings_agree_and_the_abi_is_still_7(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(lib._name)
    assert re.search(r"\b" + NAME + r"\s*\(", code)
    assert NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    assert getattr(raw, NAME) is not None
    decl = [a.strip() for a in re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", code).group(1).split(",")]

    def kind(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "size_t": C.c_size_t, "double": C.c_double, "int": C.c_int}[a.rsplit(" ", 1)[0]]

    res, args = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and [kind(a) for a in decl] == list(args)
    assert [a.rsplit(" ", 1)[1].lstrip("*") for a in decl] == [
        "slots", "slot_words", "table", "S", "images_host", "G", "keep", "nms_result", "cols", "C", "out_slots", "out_table", "out_cols",
        "out_src", "out_n", "stream"]
    assert decl[1] == "long long slot_words" and decl[6] == "const uint8_t* keep" and decl[7] == "const int32_t* nms_result"
    # the definition takes the same list
    src = open(os.path.join(ROOT, "hybridgl_amd", "csrc", "rle.hip")).read()
    defn = [" ".join(a.split()) for a in re.search(r"\bint " + NAME + r"\s*\(([^)]*)\)\s*\{", src).group(1).split(",")]
    assert defn == decl
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7


def test_refusal_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    a = np.asarray([[70, 37, 0, -1]], dtype=np.int64)
    assert lib.hgl_rle_select_device(None, 4, None, 0, a.ctypes.data, 1, None, None, None, 0, None, None, None, None, None, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_every_einval_of_the_contract_through_the_plan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "the plan is checked as a compiled program: g++ is needed"
    exe = tmp_path / "rle_select_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "rle_select_sanitize.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    images, S = SC.packed(SC.SIZES, SC.N, SC.LIMITS)
    good = [SC.case(images, S), SC.case(images, S, has_keep=0, has_nms=1, C=0), SC.case(images, S, C=8, sw=1),
            SC.case([[5, 5, 0, 0]], 0, sw=0, C=0)]
    todo = good + [c for _, c in SC.refusals()]
    path = tmp_path / "cases.txt"
    path.write_text("".join(SC.line_of(c) + "\n" for c in todo))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and len(lines) == len(todo), r.stderr[-2000:]
    for c, line in zip(good, lines):
        assert SC.want_of(c) is not None and line.startswith("0 "), line
    seen = set()
    for (why, c), line in zip(SC.refusals(), lines[len(good):]):
        assert SC.want_of(c) is None and line.startswith("-1 ") and why in line, (why, line)
        seen.add(why)
    # one per rule: the group, the set, the sizes, the entries, the per-image limit, the NMS's plane words, the slot size at
    # either end and 0, the columns at either end, keep / nms_result both and neither, either overlap, the grid
    assert len(seen) == 17


def test_select_layout():
    images = ops.rle_select_layout([(70, 37), (64, 64), (512, 640), (3, 50)], [3, 0, 5, 1])
    assert images.dtype == np.int64 and images.tolist() == [[70, 37, 0, -1], [64, 64, 3, -1], [512, 640, 3, -1], [3, 50, 8, -1]]
    assert ops.rle_select_layout([(4, 4), (5, 5)], [2, 3], 1)[:, 3].tolist() == [1, 1]
    assert ops.rle_select_layout([(4, 4), (5, 5), (6, 6)], [2, 3, 1], [0, None, -5])[:, 3].tolist() == [0, -1, -1]
    for sizes, counts, mk in [([(4, 4)], [1, 2], None), ([(4, 4)], [-1], None), ([(4, 4)], [1], [1, 2])]:
        with pytest.raises(ValueError):
            ops.rle_select_layout(sizes, counts, mk)


def naive(slots, table, images, keep, cols, fence):
    """the contract entry by entry, into buffers filled with `fence`"""
    S, sw = slots.shape
    C = cols.shape[0]
    o_slots = np.full((S, sw), fence, np.uint32)
    o_table = np.full((S, 4), fence, np.int32)
    o_cols = np.full((C, S), fence, np.uint32)
    o_src = np.full(S, fence, np.int32)
    o_n = np.full(len(images), fence, np.int32)
    if S == 0:
        return o_slots, o_table, o_cols, o_src, o_n
    for g, (H, W, e, mk) in enumerate(images):
        end = images[g + 1][2] if g + 1 < len(images) else S
        p = 0
        for i in range(end - e):
            if not keep[e + i] or (mk >= 0 and p >= mk):
                continue
            d = e + p
            o_table[d] = table[e + i]
            o_src[d] = i
            for c in range(C):
                o_cols[c, d] = cols[c, e + i]
            n, form = int(table[e + i, 0]), int(table[e + i, 1])
            words = n if form == 0 else ((H * W + 31) // 32 if form == 1 else -1)
            if n >= 0 and 0 <= words <= sw:
                for w in range(words):
                    o_slots[d, w] = slots[e + i, w]
            p += 1
        o_n[g] = p
        for d in range(e + p, end):
            o_table[d] = (1, 0, 0, 0)
            o_slots[d, 0] = H * W
            o_src[d] = -1
            for c in range(C):
                o_cols[c, d] = 0
    return o_slots, o_table, o_cols, o_src, o_n


def test_the_numpy_statement_against_a_naive_loop():
    rng = np.random.default_rng(3)
    FENCE = 0x7E7E7E7E
    met = set()
    for trial in range(120):
        G = int(rng.integers(1, 6))
        sizes = [(int(rng.integers(1, 12)), int(rng.integers(1, 12))) for _ in range(G)]
        counts = [int(rng.integers(0, 9)) for _ in range(G)]
        if trial == 0:
            counts = [0] * G
        S, sw, C = sum(counts), int(rng.integers(1, 8)), int(rng.integers(0, 4))
        images = ops.rle_select_layout(sizes, counts, [int(rng.integers(-1, 6)) for _ in range(G)]).tolist()
        slots = rng.integers(0, 1 << 32, (S, sw), dtype=np.uint64).astype(np.uint32)
        table = np.zeros((S, 4), np.int32)
        table[:, 0] = rng.integers(-1, sw + 3, S)      # counts that fit, that do not, and a negative one
        table[:, 1] = rng.choice([0, 0, 0, 1, 1, 2, 3, 7], S)
        table[:, 2:] = rng.integers(0, 100, (S, 2))
        keep = rng.integers(0, 3, S).astype(np.uint8)
        cols = rng.integers(0, 1 << 32, (C, S), dtype=np.uint64).astype(np.uint32)
        want = naive(slots, table, images, keep, cols, FENCE)
        got = SC.select(slots, table, images, keep, cols, *[np.full_like(w, FENCE) for w in want])
        for a, b, what in zip(got, want, ("slots", "table", "cols", "src", "n")):
            assert np.array_equal(a, b), (trial, what)
        for (H, W, e, mk), n, k in zip(images, counts, got[4]):
            if S:
                met.add("none" if k == 0 else ("all" if k == n else "some"))
                met.add("cut" if 0 <= mk < int((keep[e:e + n] != 0).sum()) else "uncut")
                assert (got[3][e:e + k] >= 0).all() and (np.diff(got[3][e:e + k]) > 0).all() and (got[3][e + k:e + n] == -1).all()
        for s in range(S):
            met.add(("words", SC.defined_words(table[s], 1, 1, sw) is None))
    assert met >= {"none", "all", "some", "cut", "uncut", ("words", True), ("words", False)}
    # who survives an NMS result: code 0 or 1 and nobody suppressed it
    res = np.asarray([[0, 5, 0, -1], [1, 5, 1, -1], [2, 0, -1, -1], [0, 5, 2, 0], [3, 0, -1, -1], [1, 4, 3, 1]])
    assert SC.kept_from_nms(res).tolist() == [True, True, False, False, False, False]
