"""Deterministic mask patterns for the connected-component clean-up (csrc/sam_ccl.hip), plain numpy, no GPU code.

Every pattern targets ONE mechanism of the device code (named in its docstring) and exists for any H, W at which it can be
built; `cases(H, W)` returns the ones that exist, `skipped(H, W)` says which do not and why.  The grid of shapes comes from
the branch points of the host code: `strip_rows(W)` restates its strip selection.

tests/test_ccl_cases_host.py checks the generator and the oracle on the CPU, tests/test_gpu_ccl_shapes.py runs the device
code over the grid.
"""
import numpy as np

# the branch points of sam_ccl.hip: < 16 (a 16-byte chunk of box_kernel spans rows), 64 (one step), 768 (last width of 16-row
# strips), 1024 (one group of RowScan steps), 4096 / 6144 (3- and 2-row strips), > 6144 (no strips: the global pass alone)
WIDTHS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1023, 1024, 1025, 1088, 2049, 4096, 4097, 6144, 6145]
STRIP = 16
STRIP_PIX = 12288
THRESH = 20         # the threshold the sized patterns (seam_links, thresh_exact) are built for


def strip_rows(W):
    """rows per LDS strip as remove_small_regions_impl computes them; 0: rows too wide, the global pass alone"""
    return min(STRIP, STRIP_PIX // W) if W <= STRIP_PIX // 2 else 0


def heights(W):
    s = strip_rows(W) or STRIP
    return sorted({h for h in (1, 2, s - 1, s, s + 1, 2 * s, 2 * s + 1) if h >= 1})


def shapes(widths=WIDTHS):
    return [(H, W) for W in widths for H in heights(W)]


def thresholds(H, W):
    """1: nothing is small; 2; 20; H*W+1: everything is small"""
    return [1, 2, THRESH, H * W + 1]


def seam_cols(W, room):
    """columns c whose left neighbour c-1 ends a 64-pixel step (63|64) or a 1024-pixel group (1023|1024), with `room` columns
    to either side"""
    return [c for c in (64, 1024) if c - room >= 0 and c + room <= W]


def seam_rows(H, W):
    """rows r whose pair r | r+1 is the top of the mask or straddles two strips"""
    s = strip_rows(W) or STRIP
    return [r for r in (s - 1, 2 * s - 1, 0) if r + 1 < H]


def _grid(H, W):
    return np.mgrid[:H, :W]


# ---------------------------------------------------------------------------------------------------------- the patterns
# each returns a list of (name, bool [H,W]) or a string: the reason it does not exist at this shape
def p_diag(H, W):
    """one-pixel diagonals: ONLY south-east / south-west links, across every step, group and strip seam"""
    if H * W < 2:
        return "a single pixel"
    yy, xx = _grid(H, W)
    return [(f"diag{p}", (xx - yy) % p == 0) for p in (3, 7)] + [(f"anti{p}", (xx + yy) % p == 0) for p in (3, 7)]


def p_comb(H, W):
    """teeth joined by a spine in the last / first row: hundreds of runs per row of ONE component that meet only through
    another row (the carried (root, sum) of the count pass, the atomics of the stats pass)"""
    if H < 2 or W < 2:
        return "needs two rows and two columns"
    yy, xx = _grid(H, W)
    out = []
    for q in (2, 3):
        out.append((f"comb_down{q}", (xx % q == 0) | (yy == H - 1)))
        out.append((f"comb_up{q}", (xx % q == 0) | (yy == 0)))
    return out


def serpentine(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[::4] = True
    for i, y in enumerate(range(0, H - 4, 4)):
        m[y + 1:y + 4, W - 1 if i % 2 == 0 else 0] = True
    return m


def p_serpentine(H, W):
    """full-width bars every 4th row joined alternately at the right and left edge: ONE union chain through all strips; its
    complement is the matching hole structure"""
    if H < 2 or W < 2:
        return "needs two rows and two columns"
    m = serpentine(H, W)
    return [("serpentine", m), ("serpentine_inv", ~m)]


def p_rings(H, W):
    """concentric one-pixel rectangles at spacing 2: many components, each crossing every strip"""
    if H < 3 or W < 3:
        return "needs three rows and three columns"
    yy, xx = _grid(H, W)
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    return [("rings", d % 2 == 0)]


def p_checker(H, W):
    """1x1 checkerboard: one 8-connected component of diagonal links only, its complement likewise; 2x2-block checkerboard"""
    if H * W < 2:
        return "a single pixel"
    yy, xx = _grid(H, W)
    out = [("checker", (xx + yy) % 2 == 0)]
    if H >= 3 or W >= 3:
        out.append(("checker2", (xx // 2 + yy // 2) % 2 == 0))
    return out


def p_alt(H, W):
    """every other row full (runs of length W over all steps and groups), every other column full"""
    yy, xx = _grid(H, W)
    out = []
    if H >= 2:
        out.append(("rows_alt", yy % 2 == 0))
    if W >= 2:
        out.append(("cols_alt", xx % 2 == 0))
    return out or "a single pixel"


def seam_pairs(H, W):
    """the rows of seam_rows packed greedily into as few masks as keep three rows between two pairs -> list of row lists"""
    masks = []
    for r in seam_rows(H, W):
        for used in masks:
            if all(abs(r - q) >= 3 for q in used):
                used.append(r)
                break
        else:
            masks.append([r])
    return masks


def seam_link_mask(H, W, k, rows, direction):
    """pairs of 1 x k blobs whose ONLY contact is one diagonal pixel pair on a seam: `se` (r, c-1)-(r+1, c), `sw`
    (r, c)-(r+1, c-1), at every seam column and every row of `rows` -> (mask, [((r, x), (r+1, x'))] the contacts)"""
    m = np.zeros((H, W), dtype=bool)
    contacts = []
    for c in seam_cols(W, k + 1):
        for r in rows:
            top, bot = (slice(c - k, c), slice(c, c + k)) if direction == "se" else (slice(c, c + k), slice(c - k, c))
            m[r, top] = True
            m[r + 1, bot] = True
            contacts.append(((r, c - 1), (r + 1, c)) if direction == "se" else ((r, c), (r + 1, c - 1)))
    return m, contacts


def p_seam_links(H, W):
    """blob pairs linked by a single diagonal contact exactly on a step / group seam, at the top of the mask and on the strip
    boundary rows.  k = 10: each blob alone is below THRESH, the pair reaches it; k = 1: the same at threshold 2.  A missed
    link flips every pixel of both blobs.  `_inv`: the same as holes.  `ctl`: blobs two columns apart (same row, and a
    knight's move) that must stay unlinked."""
    if W < 66 or H < 2:
        return "needs W >= 66 (a seam with a column to either side and one spare) and two rows"
    out = []
    for k in (1, 10):
        if not seam_cols(W, k + 1):
            continue
        for direction in ("se", "sw"):
            for i, rows in enumerate(seam_pairs(H, W)):
                m, _ = seam_link_mask(H, W, k, rows, direction)
                out.append((f"seam_links_{direction}_k{k}_{i}", m))
                if k == 10:
                    out.append((f"seam_links_{direction}_k{k}_{i}_inv", ~m))
    for c in seam_cols(W, 12)[-1:]:
        m = np.zeros((H, W), dtype=bool)
        m[0, c - 11:c - 1] = True                   # ten pixels, columns c-1 and c unset, ten pixels
        m[0, c + 1:c + 11] = True
        if H >= 4:
            m[2, c - 10:c] = True                   # (2, c-1) and (3, c+1): a knight's move apart
            m[3, c + 1:c + 11] = True
        out.append(("seam_links_ctl", m))
    return out


def p_thresh_exact(H, W):
    """components of exactly THRESH-1 and THRESH pixels: single runs laid across a seam column, two-row components that
    straddle a strip boundary; `_inv`: holes of the same sizes in a full mask"""
    out = []
    t = THRESH
    if W >= 2 * t + 1:
        m = np.zeros((H, W), dtype=bool)
        cs = seam_cols(W, 2 * t) or [t // 2]
        for c in cs:
            m[0, c - t // 2:c + t // 2] = True                          # t pixels over c-1 | c
            m[0, c + t // 2 + 2:c + t // 2 + 2 + t - 1] = True          # t-1 pixels, two columns on
            if H >= 3:
                m[2, c - t // 2:c + t // 2 - 1] = True                  # t-1 pixels over c-1 | c
        out += [("thresh_exact_runs", m), ("thresh_exact_runs_inv", ~m)]
    if W >= t + 3 and H >= 2:
        m = np.zeros((H, W), dtype=bool)
        for r in seam_rows(H, W)[:1]:
            m[r:r + 2, 1:1 + t // 2] = True                             # t pixels in two rows
            m[r:r + 2, t // 2 + 3:t + 3] = True
            m[r + 1, t + 2] = False                                     # t-1
        out += [("thresh_exact_rows", m), ("thresh_exact_rows_inv", ~m)]
    return out or "needs W >= 23"


def tie_masks(H, W):
    """-> [bool [H,W]] x 2: (a) the raster-first of the tied components starts in row 0 at a LATER column, the other in row 1
    at column 0; (b) the reverse.  Three pixels each; a third tied one in the first row of the second strip, a single pixel
    as a smaller bystander."""
    s = strip_rows(W) or STRIP
    out = []
    for first, second in ((4, 0), (0, 4)):
        m = np.zeros((H, W), dtype=bool)
        m[0, first:first + 3] = True
        m[1, second:second + 3] = True
        if H >= s + 1 and s >= 3:
            m[s, 4:7] = True
        elif H >= 4:
            m[3, 4:7] = True
        if W >= 10:
            m[0, W - 1] = True
        out.append(m)
    return out


def p_tie(H, W):
    """all components small and several tied for the largest area: above every area islands mode keeps exactly the first
    in raster order (which in `tie_a` is not the leftmost)"""
    if W < 7 or H < 2:
        return "needs W >= 7 and two rows"
    a, b = tie_masks(H, W)
    return [("tie_a", a), ("tie_b", b)]


def p_corners(H, W):
    """single pixels at the four corners, single pixels in the last column of a step / group and the first of the next, the
    empty and the full mask"""
    four = np.zeros((H, W), dtype=bool)
    four[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = True
    cols = np.zeros((H, W), dtype=bool)
    for i, x in enumerate(sorted({x for x in (63, 64, 1023, 1024, W - 1) if x < W})):
        cols[(2 * i) % H, x] = True
    out = [("corners_empty", np.zeros((H, W), dtype=bool)), ("corners_full", np.ones((H, W), dtype=bool))]
    if H * W >= 2:
        out.append(("corners_cols", cols))
    if H * W >= 5:
        out.append(("corners_four", four))
    return out


def p_speckle(H, W):
    """seeded noise around the percolation threshold of 8-connectivity, and 2x2 blobs"""
    if H * W < 16:
        return "fewer than 16 pixels"
    out = []
    for p in (0.3, 0.41, 0.5, 0.59):
        rng = np.random.default_rng([H, W, int(p * 100)])
        out.append((f"speckle{int(p * 100)}", rng.random((H, W)) < p))
    coarse = np.random.default_rng([H, W, 2]).random((H // 2 + 1, W // 2 + 1)) < 0.5
    out.append(("speckle_blobs", np.repeat(np.repeat(coarse, 2, axis=0), 2, axis=1)[:H, :W]))
    return out


PATTERNS = {"diag": p_diag, "comb": p_comb, "serpentine": p_serpentine, "rings": p_rings, "checker": p_checker,
            "alt": p_alt, "seam_links": p_seam_links, "thresh_exact": p_thresh_exact, "tie": p_tie, "corners": p_corners,
            "speckle": p_speckle}
TRIVIAL_ON_PURPOSE = ("corners_empty", "corners_full")


def cases(H, W):
    """[(name, uint8 [H,W])]: every pattern that exists at this shape, set pixels as 1 -- except `nonbinary`, the 2x2-blob
    checkerboard (or, where that does not exist, the first pattern) with its set bytes written as 255 and 2"""
    out = []
    for fn in PATTERNS.values():
        r = fn(H, W)
        if not isinstance(r, str):
            out += [(name, m.astype(np.uint8)) for name, m in r]
    base = dict(out).get("checker2", out[0][1])
    nb = base.copy()
    nb[base != 0] = np.where(np.arange(int((base != 0).sum())) % 2 == 0, 255, 2).astype(np.uint8)
    if nb.any():
        out.append(("nonbinary", nb))
    return out


def skipped(H, W):
    """{pattern family: reason} of the families that do not exist at this shape"""
    return {k: r for k, fn in PATTERNS.items() for r in [fn(H, W)] if isinstance(r, str)}


def batch(H, W):
    """-> (names, uint8 [N,H,W])"""
    c = cases(H, W)
    return [n for n, _ in c], np.stack([m for _, m in c])


# ---------------------------------------------------------------------------------------------------------- flood fill
def flood_components(work):
    """8-neighbour flood fill -> (labels int [H,W], 0 = background, numbered by first pixel in raster order; sizes list)"""
    H, W = work.shape
    lab = np.zeros((H, W), dtype=np.int64)
    sizes = []
    for y, x in zip(*(a.tolist() for a in np.nonzero(work))):        # (raster order)
        if True:
            if not lab[y, x]:
                sizes.append(0)
                stack = [(y, x)]
                lab[y, x] = len(sizes)
                while stack:
                    cy, cx = stack.pop()
                    sizes[-1] += 1
                    for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                        for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                            if work[ny, nx] and not lab[ny, nx]:
                                lab[ny, nx] = len(sizes)
                                stack.append((ny, nx))
    return lab, sizes


def flood_remove_small_regions(mask, thresh, mode):
    """the rule of utils/amg.py:267-291 on the flood fill: strict `<`, the FIRST largest component on ties"""
    holes = mode == "holes"
    lab, sizes = flood_components(mask != holes)
    small = [i + 1 for i, s in enumerate(sizes) if s < thresh]
    if not small:
        return mask, False
    if holes:
        return mask | np.isin(lab, small), True
    keep = [i + 1 for i, s in enumerate(sizes) if s >= thresh] or [sizes.index(max(sizes)) + 1]
    return np.isin(lab, keep), True
