"""The host side of the RLE decode entries -- rle_group_plan (csrc/rle_group.h): validation of the caller's image rows, tile
prefix sums, the choice of the store path per image -- and the tiling all RLE entries share (rle_tiles) under AddressSanitizer
+ UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_group_sanitize.cpp) built with g++
-fsanitize=address,undefined -fno-sanitize-recover: accepted geometries against the same arithmetic in Python, every refusal of
the contract, seeded random rows, the one-image rows of the single-size entries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_group") / "rle_group_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_group_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def tiles_of(H, W, base):
    """rle_tiles in Python: (wide, 64-row words per column, blocks across, blocks down)"""
    wide = W % 4 == 0 and base % 4 == 0
    HW64 = (H + 63) // 64
    return wide, HW64, (W + (255 if wide else 63)) // (256 if wide else 64), (HW64 + 3) // 4


def plan(images, S, base, nbytes):
    """rle_group_plan in Python: None when the geometry is refused, else (tiles, wide bits, rows of H W first tile0 off)"""
    G = len(images)
    if not 1 <= G <= 64:
        return None
    tiles, wide_bits, rows, ext = 0, 0, [], []
    for g, (H, W, e, o) in enumerate(images):
        e_next = images[g + 1][2] if g + 1 < G else S
        if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31 and H * W < 2 ** 31):
            return None
        if not (0 <= e <= e_next <= S and (g > 0 or e == 0)):
            return None
        n = e_next - e
        if n * H * W >= 2 ** 31 or not (0 <= o <= nbytes and n * H * W <= nbytes - o):
            return None
        lo, hi = o, o + n * H * W
        if any(lo != hi and a != b and not (b <= lo or hi <= a) for a, b in ext):
            return None
        ext.append((lo, hi))
        wide, _, col, row = tiles_of(H, W, base + o)
        rows.append((H, W, e, tiles, o))
        wide_bits |= int(wide) << g
        tiles += n * col * row
        if tiles >= 2 ** 31:
            return None
    return tiles, wide_bits, rows


def packed(sizes, counts, gaps=None):
    images, e, o = [], 0, 0
    for g, ((H, W), n) in enumerate(zip(sizes, counts)):
        o += gaps[g] if gaps else 0
        images.append([H, W, e, o])
        e += n
        o += n * H * W
    return images, e, o


def cases():
    out = []
    sizes = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (64, 64), (640, 640)]
    counts = [4, 4, 0, 2, 5, 9, 1, 64]
    images, S, total = packed(sizes, counts)
    for base in (4096, 4097, 4099):
        out.append((images, S, base, total))
    g_images, _, g_total = packed(sizes, counts, gaps=[5, 1, 2, 7, 0, 3, 1, 9])
    out.append((g_images, S, 4096, g_total + 100))
    out.append((images[:1], 4, 0, 4))
    out.append(([[4, 4, 0, 0]] * 64, 0, 0, 0))                  # 64 images without an entry
    out.append(([[4, 4, 0, 0]] * 65, 0, 0, 0))                  # G > 64
    out.append(([], 0, 0, 0))                                   # G = 0

    def edit(g, col, value, S=S, nbytes=total):
        im = [list(r) for r in images]
        im[g][col] = value
        return im, S, 4096, nbytes

    out += [edit(1, 3, images[1][3] - 1), edit(7, 3, images[7][3] + 1), (images, S, 4096, total - 1), edit(3, 2, images[2][2] - 1),
            edit(0, 2, 1), edit(7, 2, S + 1), edit(1, 3, -4), edit(1, 0, 0), edit(1, 1, -3), edit(7, 0, 1 << 31), edit(7, 1, 1 << 15),
            (images, S - 1, 4096, total), (images, S + 1, 4096, total), ([[1 << 15, 1 << 15, 0, 0]], 2, 0, 1 << 40),
            ([[64, 64, 0, 0]], 1 << 20, 0, 1 << 40), ([[1, 1, 0, 0]], (1 << 31) - 1, 0, 1 << 40)]
    rng = np.random.default_rng(7)
    for _ in range(300):
        G = int(rng.integers(1, 9))
        sz = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(G)]
        cn = [int(rng.integers(0, 5)) for _ in range(G)]
        im, s, tot = packed(sz, cn, gaps=[int(v) for v in rng.integers(0, 4, G)])
        if rng.random() < 0.5:      # break one number
            g, col = int(rng.integers(0, G)), int(rng.integers(0, 4))
            im[g][col] += int(rng.integers(-40, 41))
        out.append((im, s, int(rng.integers(0, 8)), tot + int(rng.integers(-3, 4))))
    # what hgl_rle_decode_device makes of (S, H, W, masks): one row (H, W, 0, 0) and S*H*W bytes, at any address
    for H, W in ONE_IMAGE_SIZES:
        for base in (0, 1, 4096, 4099):
            out.append(([[H, W, 0, 0]], 3, base, 3 * H * W))
    out.append(([[1 << 16, 1 << 15, 0, 0]], 1, 0, 1 << 31))      # H*W = 2^31
    out.append(([[1 << 15, 1 << 15, 0, 0]], 2, 0, 1 << 31))      # S*H*W = 2^31
    return out


ONE_IMAGE_SIZES = [(65, 63), (65, 260), (640, 640), (1, 1), (3, 5), (130, 4)]
TILE_CASES = [(H, W, base) for H, W in ONE_IMAGE_SIZES + [(63, 256), (64, 257), (257, 64), ((1 << 31) - 1, 1), (1, (1 << 31) - 4),
                                                           (1, (1 << 31) - 1)] for base in (0, 1, 2, 4096, (1 << 48) + 4)]


def test_plan_under_asan_ubsan(harness, tmp_path):
    todo = cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for images, S, base, nbytes in todo:
            f.write(" ".join(str(v) for v in [len(images), S, base, nbytes] + [x for row in images for x in row]) + "\n")
        for H, W, base in TILE_CASES:
            f.write(f"T {H} {W} {base}\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(todo) + len(TILE_CASES)
    for (H, W, base), line in zip(TILE_CASES, lines[len(todo):]):
        wide, HW64, col, row = tiles_of(H, W, base)
        assert line == f"T {int(wide)} {HW64} {col} {row}", (H, W, base, line)
    lines = lines[:len(todo)]
    accepted = 0
    for k, ((images, S, base, nbytes), line) in enumerate(zip(todo, lines)):
        want = plan(images, S, base, nbytes)
        if want is None:
            assert line.startswith("-1 "), (k, line)
            continue
        accepted += 1
        tiles, wide, rows = want
        assert line == f"0 {tiles} {wide}" + "".join(f" | {H} {W} {e} {t0} {o}" for H, W, e, t0, o in rows), (k, line)
    assert 100 < accepted < len(todo) - 100
    # the messages of the refusals the device test reads
    assert "65 images" in lines[6] and "overlap" in lines[8]
    # 3 x 5 in front of 64 x 64 at an aligned base: the latter's first byte is odd, it takes the byte path
    images, S, base, nbytes = todo[0]
    assert (plan(images, S, base, nbytes)[1] >> 6) & 1 == 0 and (plan(images, S, base, nbytes)[1] >> 1) & 1 == 1
    # the one-image rows: accepted with the store path of (W, address) and S * tiles of one mask; 2^31 pixels or bytes refused
    one = todo[-(4 * len(ONE_IMAGE_SIZES) + 2):]
    for (images, S, base, nbytes), line in zip(one[:-2], lines[-len(one):-2]):
        H, W = images[0][:2]
        wide, _, col, row = tiles_of(H, W, base)
        assert wide == (W % 4 == 0 and base % 4 == 0) and line.startswith(f"0 {S * col * row} {int(wide)} |"), line
    assert all(l.startswith("-1 ") and "2^31" in l for l in lines[-2:]), lines[-2:]
