"""The contract of tests/heat_cases.py (numpy float32, operation by operation) against an independent float64 loop, pixel by
pixel: the levels agree wherever the float64 t * 255 lies farther than 1e-3 from a half-integer -- float32 carries t * 255 to
about 255 * 4 * 2^-24 = 6e-5, so only such pixels can round the other way -- and the excluded share stays under 1 % of a case.
The codes 1, 2, 3 on hand-built maps; rint's ties on a map of {0, 0.5, 1}; the blend against a float64 evaluation."""
import numpy as np
import pytest

import heat_cases as HC

f32 = np.float32
SEEDS = {(2, 5): 1, (7, 64): 2, (5, 67): 3, (97, 131): 4, (1, 3): 5, (1, 2): 6}


def w64(dirflag, W, i):
    """the column weight in float64, from the definition of linspace"""
    lin = lambda a, b, n, k: a if n == 1 else a + (b - a) * k / (n - 1)
    if dirflag == 1:
        return lin(1.0, 0.0, W, i)
    if dirflag == 2:
        return lin(0.0, 1.0, W, i)
    if dirflag == 3:
        w1 = W // 2
        return lin(0.0, 1.0, w1, i) if i < w1 else lin(1.0, 0.0, W - w1, i - w1)
    return 1.0


@pytest.mark.parametrize("size", sorted(SEEDS))
@pytest.mark.parametrize("dirflag", [0, 1, 2, 3])
def test_levels_against_a_float64_loop(size, dirflag):
    H, W = size
    x = HC.fill(np.random.default_rng(SEEDS[size]), H, W, "rand")
    code, mn, mx, peak, L = HC.levels_of(x, dirflag)
    xs = [[float(v) for v in row] for row in x]
    lo, hi = min(map(min, xs)), max(map(max, xs))
    g = [[(xs[y][i] - lo) / (hi - lo) * w64(dirflag, W, i) for i in range(W)] for y in range(H)]
    top = max(map(max, g))
    if top == 0:
        assert code == 3 and L is None
        return
    assert code == 0 and float(mn) == lo and float(mx) == hi and abs(float(peak) - top) <= 4e-7 * top
    skipped = 0
    for y in range(H):
        for i in range(W):
            v = g[y][i] / top * 255.0
            if abs(v - np.floor(v) - 0.5) <= 1e-3:
                skipped += 1
                continue
            assert int(L[y, i]) == int(np.floor(v + 0.5)), (y, i, v, L[y, i])
    assert skipped <= 0.01 * H * W, (skipped, H * W)


def test_codes_on_hand_built_maps():
    one = lambda x, d=0: HC.levels_of(np.asarray(x, f32), d)[0]
    assert one([[3.0]]) == 1 and one([[2.0, 2.0], [2.0, 2.0]], 1) == 1
    assert one([[1.0, np.nan]]) == 2 and one([[1.0, np.inf]]) == 2 and one([[-np.inf, 0.0]]) == 2
    assert one([[-3e38, 3e38]]) == 2      # finite values, an infinite range
    assert one([[1.0], [2.0], [0.0]], 2) == 3      # W = 1 under right: linspace(0, 1, 1) is 0
    assert one([[1.0], [2.0], [0.0]], 1) == 0 and one([[1.0], [2.0], [0.0]], 3) == 0      # ... under left and middle it is 1
    assert one([[5.0, 1.0]], 2) == 3      # everything above the minimum sits at weight 0
    assert one([[1.0, 5.0]], 2) == 0
    # a code other than 0: a plain copy of the base, levels 0, status (code, 0, 0, 0)
    call = HC.make_call(1, [dict(size=(3, 1), dir=2), dict(size=(2, 5), dir=0, kind="nan")], gaps=[1, 2])
    out, levels, status = HC.expect(call)
    assert status.tolist() == [[3, 0, 0, 0], [2, 0, 0, 0]]
    assert np.array_equal(out[1:4], call["base"][0:3]) and np.array_equal(out[6:16], call["base"][3:13])
    assert np.all(levels[1:4] == 0) and np.all(levels[6:16] == 0)
    assert np.all(out[0] == 0xA5) and np.all(out[4:6] == 0xA5) and levels[0] == 0xA5 and np.all(levels[4:6] == 0xA5)


def test_rint_ties_go_to_the_even_level():
    x = np.array([[0.0, 0.5, 1.0]], f32)
    code, mn, mx, peak, L = HC.levels_of(x, 0)
    assert code == 0 and (mn, mx, peak) == (0, 1, 1) and L.tolist() == [[0, 128, 255]]      # 127.5 -> 128
    # the other exact ties of a map in eighths: 0.125 * 255 = 31.875 is none, 0.1 * 255 in float32 neither; x / 2 keeps them
    L = HC.levels_of(np.array([[0.0, 0.25, 0.5, 1.0]], f32) * f32(0.5) + f32(3), 0)[4]
    assert L.tolist() == [[0, 64, 128, 255]]      # 63.75 -> 64, 127.5 -> 128
    # the peak normalises the guided map, not the map: under `right` over three columns the middle one is halved
    code, _, _, peak, L = HC.levels_of(np.array([[0.0, 1.0, 0.5]], f32), 2)
    assert code == 0 and peak == f32(0.5) and L.tolist() == [[0, 255, 255]]


def test_the_blend_against_float64():
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    L = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    ramp = HC.random_ramp()
    got = HC.blend_levels(base, L, ramp)
    colours, a, b = HC.ramp_parts(ramp)
    for y in range(9):
        for x in range(11):
            for c in range(3):
                v = float(base[y, x, c]) * float(a[L[y, x]]) + float(colours[L[y, x], c]) * float(b[L[y, x]])
                if abs(v - np.floor(v) - 0.5) > 1e-3:
                    assert int(got[y, x, c]) == int(min(max(np.floor(v + 0.5), 0), 255))
    # weights that are not finite: NaN (also inf - inf) gives 0, +inf 255, -inf 0
    ramp = HC.broken_ramp()
    px = np.full((1, 1, 3), 9, np.uint8)
    at = lambda level: HC.blend_levels(px, np.array([[level]], np.uint8), ramp)[0, 0].tolist()
    colours = HC.ramp_parts(ramp)[0]
    assert at(0) == [0, 0, 0] and at(128) == [0, 0, 0] and at(200) == [0, 0, 0] and at(255) == [0, 0, 0]
    assert at(7) == [255 if colours[7, c] else 0 for c in range(3)]      # colour * inf: inf, or NaN for a channel of 0
