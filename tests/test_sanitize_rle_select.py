"""The host side of hgl_rle_select_device -- rle_select_plan (csrc/rle_group.h): validation of the caller's image rows, the
per-image limit, max_keep as the kernels take it, the overlap of source and destination, the chunks and blocks of the move
kernel and the choice of its 16-byte path -- under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
(tests/native/rle_select_sanitize.cpp) built with g++ -fsanitize=address,undefined -fno-sanitize-recover: accepted geometries
against the same arithmetic in Python (tests/rle_select_cases.py), one refusal per rule of the contract, seeded random rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rle_select_cases import A, LIMITS, N, SIZES, case, line_of, packed, refusals, want_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_select") / "rle_select_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_select_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def cases():
    images, S = packed(SIZES, N, LIMITS)
    out = [case(images, S), case(images, S, sw=2048), case(images, S, sw=2049, C=0, has_keep=0, has_nms=1),
           case(images, S, sw=7), case(images, S, slots=A["slots"] + 4), case(images, S, out_slots=A["out_slots"] + 8),
           case(images, S, out_slots=A["slots"] + S * 8 * 4), case(images, S, out_table=A["table"] - 16 * S),      # back to back
           case([[4, 4, 0, 0]] * 64, 0, sw=0, C=0),                   # 64 images without an entry: no word is needed
           case([[640, 640, 0, 9]], 0, out_slots=A["slots"], out_table=A["table"]),      # nothing to overlap
           case([[8, 8, 0, 4096]], 4096, sw=2, C=8),                  # the per-image limit itself
           case([[2, 2, 4096 * g, 4095] for g in range(64)], 64 * 4096, sw=1),      # ... in every image: the largest S there is
           case([[(1 << 31) - 1, 1, 0, 1 << 40]], 3, sw=(1 << 26)),
           case([[1, (1 << 31) - 1, 0, -(1 << 40)]], 2, sw=(1 << 31) - 1)]
    out += [c for _, c in refusals()]
    rng = np.random.default_rng(17)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        im, S = packed(sz, [int(rng.integers(0, 200)) for _ in range(G)], [int(rng.integers(-3, 220)) for _ in range(G)])
        if rng.random() < 0.4:      # break one number
            g, col = int(rng.integers(0, G)), int(rng.integers(0, 3))
            im[g][col] += int(rng.integers(-300, 301))
        c = case(im, S, sw=int(rng.integers(0, 5000)), C=int(rng.integers(-1, 10)), has_keep=int(rng.integers(0, 2)),
                 has_nms=int(rng.integers(0, 2)))
        if rng.random() < 0.3:      # destinations near the sources, any alignment
            c["out_slots"] = c["slots"] + int(rng.integers(-4, 5)) * max(S * c["sw"], 1) + int(rng.integers(-2, 3)) * 4
            c["out_table"] = c["table"] + int(rng.integers(-3, 4)) * 8 * max(S, 1)
        out.append(c)
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for c in todo:
            f.write(line_of(c) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    accepted = 0
    for k, (c, line) in enumerate(zip(todo, lines)):
        want = want_of(c)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        totals, rows = want
        assert line == "0 " + " ".join(str(v) for v in totals) + "".join(" | " + " ".join(str(v) for v in row) for row in rows) \
            + f" | {c['S']}", (k, line)
    assert 40 < accepted < len(todo) - 100
    # every refusal, by its message
    for why, c in refusals():
        line = next(l for d, l in zip(todo, lines) if d is c or d == c)
        assert line.startswith("-1 ") and why in line, (why, line)
    # by hand: 818 entries of 8 words -> one chunk, 205 blocks, the 16-byte path; max_keep clamped to the image's entries
    assert lines[0].split(" | ")[0] == "0 1 205 1"
    assert [r.split()[-1] for r in lines[0].split(" | ")[1:-1]] == ["4", "0", "0", "65", "5", "1", "70", "511"]
    assert lines[1].split(" | ")[0] == "0 1 205 1" and lines[2].split(" | ")[0] == "0 2 410 0" and lines[3].split(" | ")[0] == "0 1 205 0"
    assert lines[4].split(" | ")[0] == "0 1 205 0" and lines[5].split(" | ")[0] == "0 1 205 0"      # a base 4 / 8 bytes off
    assert lines[11].split(" | ")[0] == f"0 1 {64 * 1024} 0" and lines[11].split(" | ")[1] == "2 2 0 4095"
