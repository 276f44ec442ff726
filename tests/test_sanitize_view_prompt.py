"""The rules of a visual prompt -- hybridgl_amd/csrc/view_prompt.h: the entry's refusals, box clamping, window, taps, marker bands,
gray -- under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/view_prompt_sanitize.cpp) built
with g++ -fsanitize=address,undefined -fno-sanitize-recover: the shared case table, a few hundred seeded random boxes, prompts
and pixels, and the extremes of every range (8192 x 8192, grow 4096, thickness 64, pad 4000) against the same arithmetic in
Python (tests/view_prompt_cases.py), line for line; one refusal per rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import view_prompt_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_view_prompt") / "view_prompt_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "view_prompt_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def cases():
    """(prompt, H, W, res, box, pixels, have_blurred, have_boxes)"""
    rng = np.random.default_rng(41)
    pix = lambda H, W, k: [(int(rng.integers(0, W)), int(rng.integers(0, H))) + tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(k)]
    out = []
    for H, W, res in VC.SHAPES:
        boxes = list(VC.mask_boxes(VC.case_masks(H, W))) + list(VC.caller_boxes(H, W))
        for fields in [VC.PRESETS[k] for k in VC.PRESETS] + VC.VARIATIONS:
            for box in boxes:
                out.append((VC.prompt(**fields), H, W, res, box, pix(H, W, 6), 1, 1))
    # the extremes: the largest image, margin, band and growth; boxes on the far corner, over the whole image, of one pixel
    big = 8192
    for box in ([0, 0, big - 1, big - 1], [big - 1, big - 1, big - 1, big - 1], [-5, -5, 2 * big, 2 * big], [0, 0, 0, 0], [100, 8000, 8191, 8100],
                [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1], [2 ** 31 - 1, 0, -2 ** 31, 5]):
        for marker in (1, 2):
            for square in (0, 1):
                p = VC.prompt(window=1, pad_permille=4000, square=square, marker=marker, thickness=64, grow=4096, global_bg=2)
                corner = [(0, 0, 255, 255, 255), (big - 1, big - 1, 0, 0, 0), (big - 1, 0, 1, 2, 3), (0, big - 1, 254, 0, 255), (4096, 4096, 9, 9, 9)]
                out.append((p, big, big, 224, box, corner + pix(big, big, 8), 1, 1))
    out.append((VC.prompt(window=1, square=1, pad_permille=250), 40, 40, 16, [3, 7, 3, 30], pix(40, 40, 2), 1, 1))      # by hand below
    for why, fields, H, W, hb, hx in VC.REFUSALS:
        out.append((VC.prompt(**fields), H, W, 8, [1, 1, 5, 5], [(0, 0, 1, 2, 3)], hb, hx))
    for _ in range(400):
        H, W, res = int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.integers(1, 80))
        p = VC.prompt(window=int(rng.integers(0, 2)), pad_permille=int(rng.integers(0, 4001)), square=int(rng.integers(0, 2)),
                      local_bg=int(rng.integers(0, 2)), global_bg=int(rng.integers(0, 4)), marker=int(rng.integers(0, 3)),
                      thickness=int(rng.integers(1, 65)), grow=int(rng.integers(0, 60)))
        if rng.random() < 0.15:      # one field out of its range
            k = VC.FIELDS[int(rng.integers(0, len(VC.FIELDS)))]
            p[k] = int(rng.choice([-1, -7, 5000, 65, 4]))
        x0, x1 = sorted(int(v) for v in rng.integers(-20, W + 20, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(-20, H + 20, 2))
        box = [x1, y0, x0, y1] if rng.random() < 0.1 and x1 > x0 else [x0, y0, x1, y1]
        out.append((p, H, W, res, box, pix(H, W, 5), int(rng.random() < 0.9), int(rng.random() < 0.9)))
    return out


def test_rules_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for c in todo:
            f.write(VC.harness_line(*c) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    refused = 0
    for k, (c, line) in enumerate(zip(todo, lines)):
        assert line == VC.harness_want(*c), (k, c[0], c[1:5], line)
        refused += line.startswith("-1 ")
    assert len(VC.REFUSALS) < refused < len(todo) // 4
    # every refusal, by its message
    seen = {line[3:] for line in lines if line.startswith("-1 ")}
    assert seen == {why for why, *_ in VC.REFUSALS}
    # by hand: box (3, 7, 3, 30) is 1 x 24, m = 24 * 250 / 1000 = 6, s = 36, origin (floor(-29 / 2), floor(2 / 2))
    hand = next(line for c, line in zip(todo, lines) if list(c[4]) == [3, 7, 3, 30])
    assert hand.split(" | ")[:2] == ["0 0 3 7 3 30", "-15 1 36 36"]
