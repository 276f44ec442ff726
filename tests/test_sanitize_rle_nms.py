"""The host side of hgl_rle_nms_device -- rle_nms_plan (csrc/rle_group.h): validation of the caller's image rows, the per-image
limit, the prefix sums of tiles, plane blocks, plane words, pair counts and suppression words -- under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_nms_sanitize.cpp) built with g++
-fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python
(tests/rle_nms_cases.py), every refusal of the contract, seeded random rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rle_nms_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_nms") / "rle_nms_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_nms_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def packed(sizes, counts):
    images, e = [], 0
    for (H, W), n in zip(sizes, counts):
        images.append([H, W, e])
        e += n
    return images, e


SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (70, 37), (640, 640)]
N = [4, 33, 0, 65, 5, 129, 70, 512]


def refusals():
    """(why, case): one case per check of the contract"""
    images, S = packed(SIZES, N)

    def edit(g, col, value, S=S):
        im = [list(r) for r in images]
        im[g][col] = value
        return im, S

    return [
        ("65 images", ([[4, 4, 0]] * 65, 0)),
        ("0 images", ([], 0)),
        ("-1 entries", (images[:1], -1)),
        ("bad size", edit(1, 0, 0)),
        ("bad size", edit(1, 1, -3)),
        ("bad size", edit(7, 0, 1 << 31)),
        ("bad size", ([[1 << 16, 1 << 15, 0]], 1)),                  # H*W = 2^31
        ("entries", edit(0, 2, 1)),                                  # does not start at 0
        ("entries", edit(3, 2, images[2][2] - 1)),                   # steps back
        ("entries", edit(7, 2, S + 1)),
        ("entries", (images, S - 513)),                              # the last image starts beyond S
        ("owns 4097 entries", ([[4, 4, 0]], 4097)),
        ("owns 4097 entries", ([[4, 4, 0], [9, 9, 2], [4, 4, 4099]], 4100)),
        ("owns 2147483647 entries", ([[4, 4, 0]], (1 << 31) - 1)),   # S at its upper limit
        ("plane words", ([[64, 1 << 20, 0]], 4096)),                 # 2^12 * 2^20 words
    ]


def cases():
    out = []
    images, S = packed(SIZES, N)
    out.append((images, S))
    out.append(([[4, 4, 0]] * 64, 0))                                # 64 images without an entry: S at its lower limit
    out.append(([[640, 640, 0]], 0))
    out.append(([[8, 8, 0]], 4096))                                  # the per-image limit itself
    out.append(([[2, 2, 4096 * g] for g in range(64)], 64 * 4096))   # ... in every image: the largest S there is
    out.append(([[(1 << 31) - 1, 1, 0]], 3))
    out.append(([[1, (1 << 31) - 1, 0]], 2))                         # one word per column: 2 * (2^31 - 1) plane words
    out += [c for _, c in refusals()]
    rng = np.random.default_rng(12)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        im, S = packed(sz, [int(rng.integers(0, 200)) for _ in range(G)])
        if rng.random() < 0.5:      # break one number
            g, col = int(rng.integers(0, G)), min(int(rng.integers(0, 4)), 2)      # the entry column as often as both sizes
            im[g][col] += int(rng.integers(-300, 301))
        out.append((im, S))
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for images, S in todo:
            f.write(" ".join(str(v) for v in [len(images), S] + [x for row in images for x in row]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    accepted = 0
    for k, ((images, S), line) in enumerate(zip(todo, lines)):
        want = NC.plan(images, S)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        totals, rows = want
        assert line == "0 " + " ".join(str(v) for v in totals) + "".join(" | " + " ".join(str(v) for v in row) for row in rows) \
            + f" | {S} 1", (k, line)
    assert 100 < accepted < len(todo) - 50      # about 150 broken rows: a first entry hardly survives, a size three times in four
    # every refusal, by its message
    for why, case in refusals():
        line = next(l for c, l in zip(todo, lines) if c == case)
        assert line.startswith("-1 ") and why in line, (why, line)
    # by hand: 159 = 1 + 2 + 0 + 6 + 1 + 15 + 6 + 128 tiles -> 7 splits; the suppression words of 4, 33, 0, 65, 5, 129, 70, 512 entries
    head = lines[0].split(" | ")[0].split()
    assert head[1] == "159" and head[5] == "7" and int(head[6]) == 4 + 33 + 0 + 65 * 2 + 5 + 129 * 3 + 70 * 2 + 512 * 8
    assert [r.split()[-1] for r in lines[0].split(" | ")[1:-1]] == [str(v) for v in np.cumsum([0, 4, 33, 0, 130, 5, 387, 140])]
    assert lines[3].split(" | ")[0].split()[1:] == ["8192", "4096", "32768", str(4096 * 4096), "1", str(4096 * 64)]
    assert lines[4].split(" | ")[0].split()[4] == str(64 * 4096 * 4096)
