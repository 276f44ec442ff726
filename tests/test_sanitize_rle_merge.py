"""The host side of hgl_rle_merge_device -- rle_merge_plan (csrc/rle_group.h): validation of the caller's image rows, the prefix
sums of plane blocks and plane words of the source set and of the merged set -- under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_merge_sanitize.cpp) built with g++
-fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python
(tests/rle_merge_cases.py), every refusal of the contract by its message, seeded random rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rle_merge_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_merge") / "rle_merge_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_merge_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def packed(sizes, counts_src, counts_out):
    images, es, eo = [], 0, 0
    for (H, W), ns, no in zip(sizes, counts_src, counts_out):
        images.append([H, W, es, eo])
        es += ns
        eo += no
    return images, es, eo


SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (70, 37), (640, 640)]
NS = [4, 33, 0, 2, 5, 9, 19, 384]
NO = [4, 11, 3, 0, 5, 1, 23, 128]


def refusals():
    """(why, case): one case per check of the contract"""
    images, Ssrc, S = packed(SIZES, NS, NO)
    M = 1000

    def edit(g, col, value, Ssrc=Ssrc, S=S, M=M):
        im = [list(r) for r in images]
        im[g][col] = value
        return im, Ssrc, S, M

    return [
        ("65 images", ([[4, 4, 0, 0]] * 65, 0, 0, 0)),
        ("0 images", ([], 0, 0, 0)),
        ("bad set sizes", (images, -1, S, M)),
        ("bad set sizes", (images, Ssrc, -1, M)),
        ("bad set sizes", (images, Ssrc, S, -1)),
        ("bad size", edit(1, 0, 0)),
        ("bad size", edit(1, 1, -3)),
        ("bad size", edit(7, 0, 1 << 31)),
        ("bad size", ([[1 << 16, 1 << 15, 0, 0]], 1, 1, 1)),                    # H*W = 2^31
        ("source entries", edit(0, 2, 1)),                                      # does not start at 0
        ("source entries", edit(3, 2, images[2][2] - 1)),                       # steps back
        ("source entries", edit(7, 2, Ssrc + 1)),
        ("source entries", (images, Ssrc - 385, S, M)),                         # the last image starts beyond Ssrc
        ("output entries", edit(0, 3, 1)),
        ("output entries", edit(4, 3, images[3][3] - 1)),
        ("output entries", edit(7, 3, S + 1)),
        ("output entries", (images, Ssrc, S - 129, M)),
        ("plane words", ([[64, 1 << 20, 0, 0]], 1 << 12, 1, 1)),                # 2^12 * 2^20 source words
        ("plane words", ([[64, 1 << 20, 0, 0]], 1, 1 << 12, 1)),                # ... merged words
        # 2^23 entries of two blocks and 2^31 - 1 - 2^23 of one: 2^31 - 1 + 2^23 blocks, 2^32 - 1 words
        ("one launch", ([[1, 257, 0, 0], [1, 1, 1 << 23, 0]], (1 << 31) - 1, 1, 1)),
    ]


def cases():
    out = []
    images, Ssrc, S = packed(SIZES, NS, NO)
    out.append((images, Ssrc, S, 1000))
    out.append((images, Ssrc, S, 0))
    out.append(([[4, 4, 0, 0]] * 64, 0, 0, 0))                       # 64 images without an entry
    out.append(([[640, 640, 0, 0]], 0, 7, 0))                        # one side empty
    out.append(([[640, 640, 0, 0]], 7, 0, 5))
    out.append(([[1, 1, 0, 0]], (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1))      # the largest sets: 2^31 - 1 blocks
    out.append(([[(1 << 31) - 1, 1, 0, 0]], 3, 5, 15))
    out.append(([[64, 1 << 20, 0, 0]], (1 << 12) - 1, (1 << 12) - 1, 1))      # one entry short of 2^32 words on either side
    out += [c for _, c in refusals()]
    rng = np.random.default_rng(12)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        cs = [int(rng.integers(0, 70)) for _ in range(G)]
        co = [int(rng.integers(0, 40)) for _ in range(G)]
        im, ssrc, s = packed(sz, cs, co)
        M = int(rng.integers(0, 500))
        if rng.random() < 0.5:      # break one number
            what, g, r = int(rng.integers(0, 6)), int(rng.integers(0, G)), int(rng.integers(0, 40))
            if what < 2:
                im[g][what] = -r                                              # a size that is not positive
            elif what < 4:
                im[g][what] = im[g - 1][what] - 1 - r if g else 1 + r         # a step back; a first entry that is not 0
            elif what == 4:
                ssrc = im[-1][2] - 1 - r                                      # the last image starts beyond the set
            else:
                s = im[-1][3] - 1 - r
        out.append((im, ssrc, s, M))
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for images, Ssrc, S, M in todo:
            f.write(" ".join(str(v) for v in [len(images), Ssrc, S, M] + [x for row in images for x in row]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    accepted = 0
    for k, ((images, Ssrc, S, M), line) in enumerate(zip(todo, lines)):
        want = MC.plan(images, Ssrc, S, M)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        totals, rows = want
        assert line == "0 " + " ".join(str(v) for v in totals) + "".join(" | " + " ".join(str(v) for v in row) for row in rows) \
            + f" | {Ssrc} {S}", (k, line)
    assert 100 < accepted < len(todo) - 100
    # every refusal, by its message
    for why, case in refusals():
        line = next(l for c, l in zip(todo, lines) if c == case)
        assert line.startswith("-1 ") and why in line, (why, line)
    # the first case by hand: the words of an image's first entry are the running sums of n * W * ceil(H / 64)
    Q = [W * ((H + 63) // 64) for H, W in SIZES]
    rows = lines[0].split(" | ")[1:-1]
    assert [int(r.split()[4]) for r in rows] == np.cumsum([0] + [n * q for n, q in zip(NS, Q)])[:-1].tolist()
    assert [int(r.split()[5]) for r in rows] == np.cumsum([0] + [n * q for n, q in zip(NO, Q)])[:-1].tolist()
    assert [int(r.split()[6]) for r in rows] == np.cumsum([0] + [n * ((q + 255) // 256) for n, q in zip(NS, Q)])[:-1].tolist()
    assert lines[0].split(" | ")[0] == lines[1].split(" | ")[0]      # M does not enter the plan
