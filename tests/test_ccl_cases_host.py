"""CPU checks of the connected-component test cases (tests/ccl_cases.py) and of the oracle they are judged by.

* oracle/sam_oracle.py:remove_small_regions (scipy) against a pure-Python 8-neighbour flood fill with the rule of
  utils/amg.py:267-291 written out (strict `<`, first largest on ties, components numbered by first pixel in raster order):
  every pattern, both modes, every threshold of the device sweep, at small shapes.  This pins the oracle's tie order and
  threshold strictness without scipy.
* the generator: the seam links are single diagonal contacts, the serpentine is one component, the ties tie, every pattern is
  non-trivial at every shape of the device grid, and the shapes at which a pattern family does not exist are exactly the
  ones the generator's rules state (printed as a table with -s).
"""
import numpy as np
import pytest

import ccl_cases as C
from oracle import sam_oracle as S

SMALL_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (3, 3), (2, 7), (4, 9), (5, 17), (3, 23), (1, 41), (7, 41), (12, 70),
                (6, 76), (5, 95)]
MODES = ("holes", "islands")


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_equals_flood_fill(shape):
    H, W = shape
    for name, m in C.cases(H, W):
        mask = m != 0
        for mode in MODES:
            for thr in C.thresholds(H, W):
                ref, ch = C.flood_remove_small_regions(mask, thr, mode)
                got, gch = S.remove_small_regions(mask, thr, mode)
                assert bool(gch) == ch, (name, mode, thr)
                assert np.array_equal(got, ref), (name, mode, thr)


def test_every_family_is_covered_by_the_small_shapes():
    seen = {n for H, W in SMALL_SHAPES for n, _ in C.cases(H, W)}
    big = {n for n, _ in C.cases(33, 1088)}
    # (the second mask of a seam family exists only where two seam rows lie less than three rows apart: narrow strips)
    assert {n for n in big if not n.endswith(("_1", "_1_inv"))} <= seen, sorted(big - seen)


def test_flood_fill_numbers_components_in_raster_order_and_takes_the_first_largest():
    m = np.zeros((4, 8), dtype=bool)
    m[0, 5:7] = True            # first in raster order, two pixels
    m[1, 0:2] = True            # second, two pixels (left of the first)
    m[3, 0] = True
    lab, sizes = C.flood_components(m)
    assert sizes == [2, 2, 1] and lab[0, 5] == 1 and lab[1, 0] == 2 and lab[3, 0] == 3
    out, ch = C.flood_remove_small_regions(m, 100, "islands")
    assert ch and np.array_equal(out, lab == 1)
    out, ch = C.flood_remove_small_regions(m, 2, "islands")            # strict: an area of exactly 2 stays
    assert ch and np.array_equal(out, (lab == 1) | (lab == 2)) and not out[3, 0]
    out, ch = C.flood_remove_small_regions(m, 1, "islands")
    assert not ch and np.array_equal(out, m)
    out, ch = C.flood_remove_small_regions(~m, 2, "holes")             # the single pixel is the only small hole
    assert ch and np.array_equal(out, ~m | (lab == 3))


def size_at(mask, p):
    lab, sizes = C.flood_components(mask)
    return sizes[lab[p] - 1] if lab[p] else 0


SEAM_SHAPES = [(2, 66), (2, 75), (17, 127), (33, 768), (31, 769), (25, 1024), (23, 1088), (11, 2049), (7, 4096), (5, 6144),
               (33, 6145)]


@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_links_are_single_diagonal_contacts_on_the_seams(shape):
    H, W = shape
    s = C.strip_rows(W) or C.STRIP
    rows_seen, cols_seen = set(), set()
    for k in (1, 10):
        if not C.seam_cols(W, k + 1):
            continue
        for direction in ("se", "sw"):
            for rows in C.seam_pairs(H, W):
                m, contacts = C.seam_link_mask(H, W, k, rows, direction)
                assert len(contacts) == len(rows) * len(C.seam_cols(W, k + 1)) >= 1
                _, sizes = C.flood_components(m)
                assert sizes == [2 * k] * len(contacts)                  # every pair is one component, no two pairs touch
                for a, b in contacts:
                    assert abs(a[0] - b[0]) == 1 and abs(a[1] - b[1]) == 1 and {a[1], b[1]} in ({63, 64}, {1023, 1024})
                    rows_seen.add(a[0]), cols_seen.add(min(a[1], b[1]))
                    for gone, other in ((a, b), (b, a)):                 # without either contact pixel the pair falls apart
                        cut = m.copy()
                        cut[gone] = False
                        assert size_at(cut, other) == k, (k, direction, a, b)
    assert 0 in rows_seen and 63 in cols_seen
    assert (1023 in cols_seen) == (W >= 1026)
    assert (s - 1 in rows_seen) == (H >= s + 1) and (2 * s - 1 in rows_seen) == (H >= 2 * s + 1)
    if W >= 76:
        ctl = dict(C.cases(H, W))["seam_links_ctl"] != 0
        _, sizes = C.flood_components(ctl)
        assert sizes == [10] * (4 if H >= 4 else 2)                      # two columns apart: nothing links


def test_serpentine_is_one_component_and_its_complement_the_hole_structure():
    from scipy import ndimage
    for H, W in C.shapes():
        if H < 2 or W < 2:
            continue
        m = C.serpentine(H, W)
        if H * W <= 40000:
            _, sizes = C.flood_components(m)
            n = len(sizes)
        else:           # (the flood fill above holds scipy's labelling to account at the small shapes)
            n = ndimage.label(m, structure=np.ones((3, 3), int))[1]
        assert n == 1, (H, W)
        bars = len(range(0, H, 4))
        assert int(m.sum()) == bars * W + 3 * (len(range(0, H - 4, 4)))
        holes = ndimage.label(~m, structure=np.ones((3, 3), int))[1]
        assert holes == (len(range(0, H - 4, 4)) + (1 if H % 4 != 1 else 0) if W > 1 else 0), (H, W)


def test_tie_really_ties():
    for H, W in C.shapes():
        if W < 7 or H < 2:
            continue
        s = C.strip_rows(W) or C.STRIP
        a, b = C.tie_masks(H, W)
        for m, first_col, other_col in ((a, 4, 0), (b, 0, 4)):
            lab, sizes = C.flood_components(m)
            assert max(sizes) == 3 < C.THRESH and sizes.count(3) >= 2 and sizes[0] == 3
            assert lab[0, first_col] == 1 and sizes[lab[1, other_col] - 1] == 3                 # the pair of the block-order question
            if H >= s + 1 and s >= 3:
                assert sizes[lab[s, 4] - 1] == 3                                            # a tied one in the second strip
            out, ch = C.flood_remove_small_regions(m, H * W + 1, "islands")
            assert ch and np.array_equal(out, lab == 1)
        # in `a` the raster-first component is not the leftmost of the tied ones
        assert np.nonzero(a[1])[0].min() == 0 and np.nonzero(a[0])[0].min() == 4


def expected_skips(H, W):
    """the generator's rules, restated: which families cannot exist at a shape"""
    e = set()
    if H * W < 2:
        e |= {"diag", "checker", "alt"}
    if H < 2 or W < 2:
        e |= {"comb", "serpentine"}
    if H < 3 or W < 3:
        e.add("rings")
    if W < 66 or H < 2:
        e.add("seam_links")
    if not (W >= 41 or (W >= 23 and H >= 2)):
        e.add("thresh_exact")
    if W < 7 or H < 2:
        e.add("tie")
    if H * W < 16:
        e.add("speckle")
    return e


def test_every_pattern_is_non_trivial_at_every_shape_of_the_grid():
    table = {}
    ns = set()
    for H, W in C.shapes():
        names, b = C.batch(H, W)
        assert len(set(names)) == len(names) and b.dtype == np.uint8 and b.shape == (len(names), H, W)
        for name, m in zip(names, b):
            if name in C.TRIVIAL_ON_PURPOSE:
                assert m.all() if name == "corners_full" else not m.any()
            else:
                assert m.any() and (H * W == 1 or not m.all()), (name, H, W)
            assert set(np.unique(m)) <= ({0, 2, 255} if name == "nonbinary" else {0, 1}), (name, H, W)
        if H * W >= 2:
            nb = b[names.index("nonbinary")]
            assert 255 in nb and (2 in nb or np.count_nonzero(nb) == 1)
        sk = C.skipped(H, W)
        assert set(sk) == expected_skips(H, W), (H, W, sk)
        for fam in sk:
            table.setdefault(fam, []).append(f"{H}x{W}")
        ns.add(len(names) * H % 4)
    assert ns == {0, 1, 2, 3}           # workgroups of four row-waves that straddle two masks or run off the end
    # nothing is left out where the mechanisms it aims at exist: two rows and a step seam with room
    for H, W in C.shapes():
        if H >= 3 and W >= 76:
            assert not C.skipped(H, W)
    for fam, where in sorted(table.items()):
        print(f"{fam}: absent at {' '.join(where)}")


def test_the_grid_is_the_branch_points_of_the_host_code():
    assert [C.strip_rows(W) for W in (1, 768, 769, 1024, 1025, 2049, 4096, 4097, 6144, 6145)] == [16, 16, 15, 12, 11, 5, 3, 2, 2, 0]
    assert C.heights(1024) == [1, 2, 11, 12, 13, 24, 25] and C.heights(6144) == [1, 2, 3, 4, 5] and C.heights(6145) == C.heights(64)
    assert len(C.shapes()) == sum(len(C.heights(W)) for W in C.WIDTHS) == 156


def test_the_block_order_case_of_the_opencv_fixture_holds_both_layouts():
    """oracle/gen_thirdparty_golden.py writes the tie patterns into cv_cc.npz as its last connected-component case: a pair of
    equal areas whose raster-first member starts in row 0 at a later column while the other starts in row 1 at column 0, and the
    reverse; every component lies below the case's threshold, so islands mode keeps the first largest label of the labeller"""
    from oracle import gen_thirdparty_golden as G
    m, thr = G.cc_masks(G.N_CC - 1)
    assert m.dtype == np.uint8 and len(m) == 2
    for k, (first_col, other_col) in enumerate(((4, 0), (0, 4))):
        lab, sizes = C.flood_components(m[k] != 0)
        assert lab[0, first_col] == 1 and sizes[0] == sizes[lab[1, other_col] - 1] == max(sizes) < thr
        assert not m[k][0, :first_col].any() and not m[k][1, :other_col].any()
        out, ch = S.remove_small_regions(m[k] != 0, thr, "islands")
        assert ch and np.array_equal(out, lab == 1)
