"""The numpy contract of the clean-up of encoded sets (tests/rle_clean_cases.py), with no GPU and no native code: its codec
and box against a naive per-pixel loop, its rule against ccl_cases.flood_remove_small_regions, the bridges -- holes first,
islands on the RESULT -- and the non-vacuity of the case list."""
import numpy as np

import ccl_cases as CC
import rle_clean_cases as RC


def naive_counts(mask):
    H, W = mask.shape
    counts, cur, run = [], False, 0
    for x in range(W):
        for y in range(H):
            if bool(mask[y, x]) != cur:
                counts.append(run)
                cur, run = not cur, 0
            run += 1
    return counts + [run]


def naive_box(mask):
    H, W = mask.shape
    pts = [(x, y) for y in range(H) for x in range(W) if mask[y, x]]
    if not pts:
        return (0, 0, 0, 0)
    return (min(p[0] for p in pts), min(p[1] for p in pts), max(p[0] for p in pts), max(p[1] for p in pts))


def naive_segments(mask, holes):
    H, W = mask.shape
    n = 0
    for x in range(W):
        prev = False
        for y in range(H):
            cur = bool(mask[y, x]) != holes
            n += cur and not prev
            prev = cur
    return n


def test_codec_box_planes_and_segments_against_a_per_pixel_loop():
    seen_forms = set()
    for name, m, t in RC.pairs()[::9] + RC.bridges():
        H, W = m.shape
        c = RC.counts_of(m)
        assert c.tolist() == naive_counts(m), name
        back, exact = RC.mask_of(c, H, W)
        assert exact and np.array_equal(back, m), name
        assert RC.box_of(m) == naive_box(m), name
        assert RC.segments(m, False) == naive_segments(m, False) and RC.segments(m, True) == naive_segments(m, True), name
        words = RC.column_words(m)
        assert len(words) == W * ((H + 63) // 64) and np.array_equal(RC.mask_of_words(words, H, W), m), name
        plane = RC.plane_of(m)
        for p in range(H * W):
            assert (int(plane[p // 32]) >> (p % 32)) & 1 == int(m[p % H, p // H]), name
        for sw in (len(c), len(c) - 1, (H * W + 31) // 32 - 1):
            row, w = RC.encoded(m, max(sw, 0))
            seen_forms.add(row[1])
            assert row[0] == len(c) and row[2] == int(m.sum()) and len(w) == (len(c), (H * W + 31) // 32, 0)[row[1]], name
    assert seen_forms == {0, 1, 2}
    # counts that do not sum to H*W are clipped, and said so
    assert RC.mask_of([2, 100], 3, 3)[1] is False and RC.mask_of([2, 100], 3, 3)[0].sum() == 7


def test_the_shared_flood_fill_is_the_oracles_rule():
    for k, (name, m, t) in enumerate(RC.pairs()):
        if m.size > 2500 and k % 6:
            continue
        for mode in ("holes", "islands"):
            want, wc = CC.flood_remove_small_regions(m, t, mode)
            got, gc = RC.remove(m, t, mode)
            assert gc == wc and np.array_equal(got, want), (name, mode)


def test_bridges_holes_first_then_islands_on_the_result():
    for name, m, t in RC.bridges():
        w = RC.clean(m, t, "both")
        filled, hc = CC.flood_remove_small_regions(m, t, "holes")
        final, ic = CC.flood_remove_small_regions(filled, t, "islands")
        assert hc and not ic and np.array_equal(w["mask"], final) and w["result"][2] == 1, name
        # one island: the two of before and the hole between them
        assert CC.flood_components(final)[1] == [int(final.sum())] and final.sum() == m.sum() + (1 if m.size == 13 else 3), name
        # the wrong order -- islands of the unfilled mask -- keeps only the first of them
        wrong = CC.flood_remove_small_regions(m, t, "islands")[0]
        assert wrong.sum() == (2 if m.size == 13 else 6) and wrong.sum() < final.sum(), name


def test_the_case_list_is_not_vacuous():
    pairs = RC.pairs()
    n = len(pairs) - len(RC.bridges())
    assert n == 2004
    both = RC.wants("both")[:n]
    holes = sum(1 for w in both if w["result"][2] & 1)
    islands = sum(1 for w in both if w["result"][2] & 2)
    two = sum(1 for w in both if w["result"][2] == 3)
    assert holes >= 600 and islands >= 800 and two >= 500, (holes, islands, two)
    # changed and equal: the one small island that stays
    assert any(w["result"][2] == 2 and np.array_equal(w["mask"], m) for w, (_, m, _) in zip(RC.wants("islands")[:n], pairs))
    # shapes on either side of one and two column words, and every threshold rule
    assert {m.shape[0] for _, m, _ in pairs} >= {1, 63, 64, 65, 128, 129, 130}
    print(f"\n{n} pairs: holes pass changes {holes}, islands pass {islands}, both {two}")
