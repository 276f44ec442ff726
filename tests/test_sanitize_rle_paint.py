"""The host side of hgl_rle_paint_device -- rle_paint_plan (csrc/rle_group.h): validation of the caller's image rows, the list
positions as a set for the plane kernel, the canvases' extents and their overlap, the tiles of the paint kernel, out against
base -- under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_paint_sanitize.cpp)
built with g++ -fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python
(tests/paint_cases.py), one refusal per rule of the contract, seeded random rows with one number broken."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from paint_cases import A, PLAN_M, PLAN_N, PLAN_SIZES, plan_case, plan_line_of, plan_packed, plan_refusals, plan_want_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_paint") / "rle_paint_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_paint_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def cases():
    im, S, K, total = plan_packed(PLAN_SIZES, PLAN_N, PLAN_M)
    gapped, _, _, total_g = plan_packed(PLAN_SIZES, PLAN_N, PLAN_M, gaps=[0, 3, 0, 1, 7, 0, 0, 2])
    big = (1 << 31) - 1
    out = [plan_case(im, S, K), plan_case(gapped, S, K, canvas=total_g + 5), plan_case(im, S, K, sw=0), plan_case(im, S, K, base=0, out=0),
           plan_case(im, S, K, out=A["base"] + 3 * total), plan_case(im, S, K, out=A["base"] - 3 * total),      # back to back
           plan_case([[4, 4, 0, 0, 16 * g] for g in range(64)], 0, 0),            # 64 images without an entry or a position
           plan_case([[1, big, 0, 0, 0]], 5, 2, canvas=big),                      # the largest image: 2 * (2^31 - 1) plane words
           plan_case([[big, 1, 0, 0, 0]], 0, 64, canvas=big),
           plan_case([[1, big, 0, 0, g * big] for g in range(63)], 0, 0, base=0)]      # one image short of the tile limit
    out += [c for _, c in plan_refusals()]
    rng = np.random.default_rng(23)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        rows, S, K, total = plan_packed(sz, [int(rng.integers(0, 200)) for _ in range(G)], [int(rng.integers(0, 50)) for _ in range(G)],
                                        gaps=[int(rng.integers(0, 4)) for _ in range(G)])
        if rng.random() < 0.4:      # break one number
            g, col = int(rng.integers(0, G)), int(rng.integers(0, 5))
            rows[g][col] += int(rng.integers(-300, 301))
        c = plan_case(rows, S, K, sw=int(rng.integers(0, 5000)), canvas=total + int(rng.integers(0, 3)))
        if rng.random() < 0.3:      # out near base, any alignment
            c["out"] = c["base"] + int(rng.integers(-4, 5)) * max(total, 1) + int(rng.integers(-2, 3))
        out.append(c)
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for c in todo:
            f.write(plan_line_of(c) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    accepted = 0
    for k, (c, line) in enumerate(zip(todo, lines)):
        want = plan_want_of(c)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        totals, rows = want
        assert line == "0 " + " ".join(str(v) for v in totals) + "".join(" | " + " ".join(str(v) for v in row) for row in rows) \
            + f" | {c['K']}", (k, line)
    assert 40 < accepted < len(todo) - 60
    # every refusal, by its message
    for why, c in plan_refusals():
        line = next(l for d, l in zip(todo, lines) if d == c)
        assert line.startswith("-1 ") and why in line, (why, line)
    # by hand: 70 x 37 is 2 row words x 37 columns = 74 plane words a position and 1 x 2 tiles; 480 x 640 is 8 x 10 tiles
    assert lines[0].split(" | ")[0] == "0 90 328132 1295"
    assert lines[0].split(" | ")[1] == "70 37 0 0 0 0 0 3" and lines[0].split(" | ")[2] == "64 64 2 148 2 2590 3 0"
    assert lines[0].split(" | ")[4] == "480 640 3 212 4 6687 8 64" and lines[0].split(" | ")[5].split()[4] == "84"
    assert lines[9].split(" | ")[0] == f"0 {63 * (1 << 25)} 0 0"
