"""The host-callable side of hgl_rle_clean_device -- rle_clean_plan (csrc/rle_group.h) and the segment logic of csrc/ccl_runs.h
that the kernel of csrc/rle_clean.hip is made of -- under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program (tests/native/rle_clean_sanitize.cpp) built with g++ -fsanitize=address,undefined -fno-sanitize-recover: the plan
against the same arithmetic in Python (tests/rle_clean_cases.py), one refusal per rule of the contract, seeded random rows; and
the algorithm -- segments from column words, the two-pointer links, the decision rule, the rewrite -- over every (case,
threshold) pair of the case list in all three modes against the flood fill, with the segment limit at and one below what a mask
needs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rle_clean_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_clean") / "rle_clean_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_clean_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def run(harness, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("".join(l + "\n" for l in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


def plan_cases():
    images, S = RC.packed(RC.SIZES, RC.N)
    out = [RC.case(images, S), RC.case(images, S, sw=0, osw=0, thresh=0, modes=1, cap=1), RC.case(images, S, modes=2, cap=(1 << 31) - 1),
           RC.case([[4, 4, 0]] * 64, 0),                              # 64 images without an entry
           RC.case([[8, 8, 0]], 4096, cap=33),                        # the per-image limit itself; one over the 8 x 8 bound of 32
           RC.case([[(1 << 31) - 1, 1, 0]], 3, sw=(1 << 26), cap=1 << 30),
           RC.case([[1, (1 << 31) - 1, 0]], 2, sw=(1 << 31) - 1, osw=(1 << 31) - 1, thresh=(1 << 31) - 1)]
    out += [c for _, c in RC.refusals()]
    rng = np.random.default_rng(23)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        im, S = RC.packed(sz, [int(rng.integers(0, 200)) for _ in range(G)])
        if rng.random() < 0.4:      # break one number
            g, col = int(rng.integers(0, G)), int(rng.integers(0, 3))
            im[g][col] += int(rng.integers(-300, 301))
        out.append(RC.case(im, S, sw=int(rng.integers(-1, 5000)), osw=int(rng.integers(-1, 5000)), thresh=int(rng.integers(-2, 900)),
                           modes=int(rng.integers(0, 5)), cap=int(rng.integers(0, 60000))))
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = plan_cases()
    lines = run(harness, tmp_path, [RC.line_of(c) for c in todo])
    accepted = 0
    for k, (c, line) in enumerate(zip(todo, lines)):
        want = RC.want_of(c)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        rows = "".join(f" | {H} {W} {e}" for H, W, e in c["images"])
        assert line == f"0 {want[0]} {want[1]}{rows} | {c['S']}", (k, line)
    assert 40 < accepted < len(todo) - 100
    for i, (why, c) in enumerate(RC.refusals()):      # they follow the seven accepted cases
        assert todo[7 + i] == c and lines[7 + i].startswith("-1 ") and why in lines[7 + i], (why, lines[7 + i])
    # by hand: the largest image that owns an entry is 640 x 640 -> 640 * 320 segments at most; seg_cap below it stands
    assert lines[0].split(" | ")[0].split()[:2] == ["0", "100"] and lines[2].split(" | ")[0].split()[:2] == ["0", str(640 * 320)]
    assert lines[3].split(" | ")[0].split()[:2] == ["0", "1"] and lines[4].split(" | ")[0].split()[:2] == ["0", "32"]


@pytest.mark.parametrize("mode", ["holes", "islands", "both"])
def test_the_segment_logic_reproduces_the_flood_fill(harness, tmp_path, mode):
    pairs, wants = RC.pairs(), RC.wants(mode)
    big = 1 << 30
    lines = run(harness, tmp_path, [RC.mask_line(m, t, mode, big) for _, m, t in pairs])
    for (name, m, t), w, line in zip(pairs, wants, lines):
        f = line.split()
        H, W = m.shape
        assert [int(v) for v in f[:7]] == [0, w["result"][2], w["result"][1], *w["box"]], (name, f[:7], w["result"], w["box"])
        got = RC.mask_of_words([int(v, 16) for v in f[7:]], H, W)
        assert np.array_equal(got, w["mask"]), name
        assert [int(v, 16) for v in f[7:]] == RC.column_words(w["mask"]), name      # padding bits stay clear


def test_the_segment_limit_refuses_and_never_truncates(harness, tmp_path):
    todo = []
    for name, m, t in RC.pairs()[::7]:
        for mode in ("holes", "islands", "both"):
            need = []      # the segments every pass that runs meets
            cur = m
            if mode != "islands":
                need.append(RC.segments(cur, True))
                cur = RC.remove(cur, t, "holes")[0]
            if mode != "holes":
                need.append(RC.segments(cur, False))
            for cap in {max(max(need), 1), max(max(need) - 1, 1), max(min(need), 1), max(min(need) - 1, 1)}:
                todo.append((name, m, t, mode, cap))
    lines = run(harness, tmp_path, [RC.mask_line(m, t, mode, cap) for _, m, t, mode, cap in todo])
    seen = set()
    for (name, m, t, mode, cap), line in zip(todo, lines):
        w = RC.clean(m, t, mode, seg_cap=cap)
        f = line.split()
        seen.add(w["code"])
        if w["code"] == 3:
            assert f == ["3", "0", "0", "0", "0", "0", "0"], (name, mode, cap, line)
        else:
            assert int(f[0]) == 0 and [int(v, 16) for v in f[7:]] == RC.column_words(w["mask"]), (name, mode, cap)
    assert seen == {0, 3}
