"""The host side of hgl_heat_paint_device -- heat_paint_plan (csrc/rle_group.h): validation of the caller's map rows, the heat
and canvas extents and the canvases' overlap, the workgroups of the three launches, out against the bytes of base the maps name
-- under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/heat_paint_sanitize.cpp) built
with g++ -fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python
(tests/heat_cases.py), one refusal per rule of the contract, seeded random rows with one number broken."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from heat_cases import A, PLAN_SIZES, plan_case, plan_line_of, plan_packed, plan_refusals, plan_want_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_heat_paint") / "heat_paint_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "heat_paint_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def cases():
    im, heat, total = plan_packed(PLAN_SIZES)
    gapped, _, total_g = plan_packed(PLAN_SIZES, gaps=[0, 3, 0, 1, 7, 0, 0, 2])
    big = (1 << 31) - 1
    shared = [[7, 64, d, 0, 0, 448 * d] for d in range(4)]      # one map under four directions over one base
    out = [plan_case(im, heat, total), plan_case(gapped, heat, total_g + 5), plan_case(im, heat, total, base=0, out=0),
           plan_case(im, heat, total, out=A["base"] + 3 * heat), plan_case(im, heat, total, out=A["base"] - 3 * total),      # back to back
           plan_case(shared), plan_case([[4, 4, m % 4, 0, 16 * m, 16 * m] for m in range(64)]),
           plan_case([[1, big, 1, 0, 0, 0]]), plan_case([[big, 1, 2, 5, 9, 3]]),                                    # the largest map: 256 shares
           plan_case([[1, big, 0, 0, 0, m * big] for m in range(64)]),
           plan_case([[2, 2, 0, 0, 1 << 40, 0]], out=A["base"] + 12)]      # out beside the named bytes of base, not beside base itself
    out += [c for _, c in plan_refusals()]
    rng = np.random.default_rng(29)
    for _ in range(300):
        M = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(M)]
        rows, heat, total = plan_packed(sz, dirs=[int(rng.integers(0, 4)) for _ in range(M)], gaps=[int(rng.integers(0, 4)) for _ in range(M)])
        if rng.random() < 0.4:      # break one number
            m, col = int(rng.integers(0, M)), int(rng.integers(0, 6))
            rows[m][col] += int(rng.integers(-300, 301))
        c = plan_case(rows, heat + int(rng.integers(0, 3)), total + int(rng.integers(0, 3)))
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
        blocks, rows = want
        assert line == f"0 {blocks}" + "".join(" | " + " ".join(str(v) for v in row) for row in rows) + f" | {blocks}", (k, line)
    assert 40 < accepted < len(todo) - 60
    # every refusal, by its message
    for why, c in plan_refusals():
        line = next(l for d, l in zip(todo, lines) if d == c)
        assert line.startswith("-1 ") and why in line, (why, line)
    # by hand: 70 x 37 = 2590 pixels is one share, 480 x 640 is 75 of 4096, 97 x 131 = 12707 is 4; 2^31 - 1 pixels take shares of
    # 2^23 pixels, 256 of them
    assert lines[0].split(" | ")[0] == "0 85"
    assert lines[0].split(" | ")[1] == "70 37 0 0 0 0 0" and lines[0].split(" | ")[4] == "480 640 3 6687 6687 6687 3"
    assert lines[0].split(" | ")[7].split()[6] == "80" and lines[0].split(" | ")[8].split()[6] == "84"
    assert lines[7].split(" | ")[0] == "0 256" and lines[9].split(" | ")[0] == f"0 {64 * 256}"
