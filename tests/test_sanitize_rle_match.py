"""The host side of hgl_rle_match_device -- rle_match_plan (csrc/rle_group.h): validation of the caller's image rows, the prefix
sums of tiles, plane blocks, plane words and partial counts, the split of a call with few tiles -- under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_match_sanitize.cpp) built with g++
-fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python, every refusal of
the contract, seeded random rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TA, TB = 32, 64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_match") / "rle_match_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_match_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def plan(images, Sa, Sb, elems):
    """rle_match_plan in Python: None when the geometry is refused, else (totals, rows, (Sa, Sb))"""
    G = len(images)
    if not 1 <= G <= 64:
        return None
    if Sa < 0 or Sb < 0 or Sa + Sb >= 2 ** 31:
        return None
    packed = elems < 0
    tiles = blocks_a = blocks_b = words_a = words_b = pairs = 0
    rows, ext = [], []
    for g, (H, W, ea, eb, o) in enumerate(images):
        ea_next = images[g + 1][2] if g + 1 < G else Sa
        eb_next = images[g + 1][3] if g + 1 < G else Sb
        if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31 and H * W < 2 ** 31):
            return None
        if not (0 <= ea <= ea_next <= Sa and (g > 0 or ea == 0)):
            return None
        if not (0 <= eb <= eb_next <= Sb and (g > 0 or eb == 0)):
            return None
        na, nb = ea_next - ea, eb_next - eb
        n = na * nb
        if packed:
            o = 0
        else:
            if not (0 <= o <= elems and n <= elems - o):
                return None
            lo, hi = o, o + n
            if any(lo != hi and a != b and not (b <= lo or hi <= a) for a, b in ext):
                return None
            ext.append((lo, hi))
        HW64 = (H + 63) // 64
        Q = W * HW64
        q_tiles = (Q + 255) // 256
        rows.append((H, W, ea, eb, o, words_a, words_b, tiles, blocks_a, blocks_b, pairs))
        pairs += n
        words_a += na * Q
        words_b += nb * Q
        blocks_a += na * q_tiles
        blocks_b += nb * q_tiles
        tiles += ((na + TA - 1) // TA) * ((nb + TB - 1) // TB)
        if words_a >= 2 ** 32 or words_b >= 2 ** 32 or blocks_a >= 2 ** 31 or blocks_b >= 2 ** 31 or tiles >= 2 ** 31:
            return None
    splits = min(max((1024 + tiles - 1) // tiles, 1), 32) if tiles else 1      # about 1024 workgroups, at most 32 per tile
    return (tiles, blocks_a, blocks_b, words_a, words_b, pairs, splits), rows, (Sa, Sb)


def packed(sizes, counts_a, counts_b, gaps=None):
    images, ea, eb, o = [], 0, 0, 0
    for g, ((H, W), na, nb) in enumerate(zip(sizes, counts_a, counts_b)):
        o += gaps[g] if gaps else 0
        images.append([H, W, ea, eb, o])
        ea += na
        eb += nb
        o += na * nb
    return images, ea, eb, o


SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (70, 37), (640, 640)]
NA = [4, 33, 0, 2, 5, 9, 19, 512]
NB = [4, 65, 3, 0, 5, 1, 23, 500]


def refusals():
    """(why, case): one case per check of the contract"""
    images, Sa, Sb, total = packed(SIZES, NA, NB)

    def edit(g, col, value, Sa=Sa, Sb=Sb, elems=total):
        im = [list(r) for r in images]
        im[g][col] = value
        return im, Sa, Sb, elems

    big = 1 << 40
    return [
        ("65 images", ([[4, 4, 0, 0, 0]] * 65, 0, 0, 0)),
        ("0 images", ([], 0, 0, 0)),
        ("bad set sizes", (images, -1, Sb, total)),
        ("bad set sizes", (images, Sa, -1, total)),
        ("bad set sizes", ([[1, 1, 0, 0, 0]], 1 << 30, 1 << 30, -1)),
        ("bad size", edit(1, 0, 0)),
        ("bad size", edit(1, 1, -3)),
        ("bad size", edit(7, 0, 1 << 31)),
        ("bad size", ([[1 << 16, 1 << 15, 0, 0, 0]], 1, 1, 1)),                 # H*W = 2^31
        ("A entries", edit(0, 2, 1)),                                           # does not start at 0
        ("A entries", edit(3, 2, images[2][2] - 1)),                            # steps back
        ("A entries", edit(7, 2, Sa + 1)),
        ("A entries", (images, Sa - 513, Sb, total)),                           # the last image starts beyond Sa
        ("B entries", edit(0, 3, 1)),
        ("B entries", edit(4, 3, images[3][3] - 1)),
        ("B entries", edit(7, 3, Sb + 1)),
        ("B entries", (images, Sa, Sb - 501, total)),
        ("outside", edit(1, 4, -4)),
        ("outside", edit(7, 4, images[7][4] + 1)),
        ("outside", (images, Sa, Sb, total - 1)),
        ("outside", edit(7, 4, total + 5)),
        ("overlap", edit(1, 4, images[1][4] - 1)),
        ("overlap", edit(6, 4, images[0][4])),
        ("plane words", ([[64, 1 << 20, 0, 0, 0]], 1 << 12, 1, -1)),            # 2^12 * 2^20 words on side A
        ("plane words", ([[64, 1 << 20, 0, 0, 0]], 1, 1 << 12, big)),
        ("one launch", ([[1, 1, 0, 0, 0]], 1 << 26, 1 << 16, -1)),              # 2^21 * 2^10 tiles
    ]


def cases():
    out = []
    images, Sa, Sb, total = packed(SIZES, NA, NB)
    out.append((images, Sa, Sb, total))
    out.append((images, Sa, Sb, total + 7))
    out.append((images, Sa, Sb, -1))                                 # no matrix: packed, column 4 not read
    junk = [r[:4] + [-99] for r in images]
    out.append((junk, Sa, Sb, -1))
    g_images, _, _, g_total = packed(SIZES, NA, NB, gaps=[5, 1, 2, 7, 0, 3, 1, 9])
    out.append((g_images, Sa, Sb, g_total))
    rev = [list(r) for r in images]                                  # the matrices in any order, as long as none overlaps
    o = 0
    for g in reversed(range(len(rev))):
        rev[g][4] = o
        o += NA[g] * NB[g]
    out.append((rev, Sa, Sb, total))
    out.append(([[4, 4, 0, 0, 0]] * 64, 0, 0, 0))                    # 64 images without an entry
    out.append(([[640, 640, 0, 0, 0]], 0, 7, 0))                     # one side empty
    out.append(([[640, 640, 0, 0, 0]], 7, 0, -1))
    out.append(([[1, 1, 0, 0, 0]], (1 << 26) - 32, 1 << 16, -1))     # one tile short of 2^31
    out.append(([[(1 << 31) - 1, 1, 0, 0, 0]], 3, 5, 15))
    out += [c for _, c in refusals()]
    rng = np.random.default_rng(11)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        ca = [int(rng.integers(0, 70)) for _ in range(G)]
        cb = [int(rng.integers(0, 130)) for _ in range(G)]
        im, sa, sb, tot = packed(sz, ca, cb, gaps=[int(v) for v in rng.integers(0, 4, G)])
        if rng.random() < 0.5:      # break one number
            g, col = int(rng.integers(0, G)), int(rng.integers(0, 5))
            im[g][col] += int(rng.integers(-40, 41))
        elems = tot + int(rng.integers(-3, 4))
        out.append((im, sa, sb, -1 if rng.random() < 0.2 else elems))
    return out


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for images, Sa, Sb, elems in todo:
            f.write(" ".join(str(v) for v in [len(images), Sa, Sb, elems] + [x for row in images for x in row]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo)
    accepted = 0
    for k, ((images, Sa, Sb, elems), line) in enumerate(zip(todo, lines)):
        want = plan(images, Sa, Sb, elems)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        totals, rows, ends = want
        assert line == "0 " + " ".join(str(v) for v in totals) + "".join(" | " + " ".join(str(v) for v in row) for row in rows) \
            + f" | {ends[0]} {ends[1]}", (k, line)
    assert 100 < accepted < len(todo) - 100
    # every refusal, by its message
    for why, case in refusals():
        line = next(l for c, l in zip(todo, lines) if c == case)
        assert line.startswith("-1 ") and why in line, (why, line)
    # a call that wants no matrix does not read column 4; the partial counts are packed by the running sum of na*nb either way
    assert lines[2] == lines[3] and [r.split()[-1] for r in lines[2].split(" | ")[1:-1]] == [r.split()[-1] for r in lines[0].split(" | ")[1:-1]]
    assert [r.split()[-1] for r in lines[0].split(" | ")[1:-1]] == [str(v) for v in np.cumsum([0] + [a * b for a, b in zip(NA, NB)])[:-1]]
    assert lines[0].split(" | ")[0].split()[-1] == "8" and lines[9].split(" | ")[0].split()[-1] == "1"      # 136 tiles; 2^31 - 2^10
