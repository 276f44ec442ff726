"""CPU checks of the post-processing cases (tests/post_cases.py): the routes, the reference and the checker.

* every geometry reaches the kernel and the tile route named beside it (the classifier restates csrc/post_geom.h and reads the
  table constants from it: a retune fails here instead of silently moving the cases), and together the cases reach every
  route of the list: two kernels x remap on / off, staged, unstaged and mixed tiles, vector and bytewise stores;
* the restatement equals the header: tests/native/post_geom_routes.cpp, a stand-alone program over post_geom.h built with g++
  under AddressSanitizer + UndefinedBehaviorSanitizer, gives the same kernel and the same tiles for all 18 geometries, and the
  same fit decision, strip counts and source indices for every output extent from 1 to 1100 on each axis combination in use;
* the float64-blend reference agrees within tol = 2^-20 max|low_res| with the two float32 CPU implementations of the operation,
  torch's F.interpolate and oracle/sam_oracle.py:postprocess_masks, on every geometry (printed with -s);
* the checker accepts, on every case, the outputs derived from the torch float32 result -- a correct implementation passes --
  and rejects each planted error: two candidates swapped, a mask shifted by a pixel, one tile's share missing from a counter,
  a box edge off by one, a box for an empty mask, a filtered candidate with mask pixels;
* the share of undecided pixels stays below the cap for the committed seeds.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import post_cases as P
from oracle import sam_oracle as S

GEOM_IDS = [P.geom_id(g) for g in P.GEOMS]
BY_ID = dict(zip(GEOM_IDS, P.GEOMS))
geoms = pytest.mark.parametrize("gid", GEOM_IDS)


@functools.lru_cache(maxsize=2)
def world(gid):
    """-> (names, low, float64 reference, torch float32 result, tol) of the K = 16 batch of one geometry"""
    g = BY_ID[gid]
    names, low = P.planes(g)
    ref = P.reference(low, g.inp, g.orig, g.S)
    with torch.no_grad():
        m = F.interpolate(torch.from_numpy(low)[:, None], (g.S, g.S), mode="bilinear", align_corners=False)
        m = m[..., :g.inp[0], :g.inp[1]]
        tf = F.interpolate(m, tuple(g.orig), mode="bilinear", align_corners=False)[:, 0].numpy()
    return names, low, ref, tf, P.tolerance(low)


# ------------------------------------------------------------------------------------------------------------------- routes
def test_table_constants_parse_from_the_kernel_source():
    c = P.table_constants()
    assert set(c) == {"PTW", "PTH", "PR", "PX1"} and all(isinstance(v, int) and v > 0 for v in c.values())
    assert c["PTW"] == c["PTH"] == 64              # post_cases.batch_sizes and store_routes count 64 x 64 tiles of 16-pixel segments


def test_ids_are_unique_and_every_group_is_present():
    assert len(set(GEOM_IDS)) == len(P.GEOMS) == 18
    assert {(g.kernel, g.tiles) for g in P.GEOMS} == {("sep", "staged"), ("pix", "staged"), ("pix", "unstaged"), ("pix", "mixed")}


@geoms
def test_geometry_reaches_its_route(gid):
    g, c = BY_ID[gid], P.table_constants()
    r = P.classify(g, c)
    assert r.sep == (g.kernel == "sep"), r
    want = {"staged": (len(r.tiles), 0), "unstaged": (0, len(r.tiles))}.get(g.tiles)
    if want is None:
        assert r.n_staged > 0 and r.n_unstaged > 0, r
    else:
        assert (r.n_staged, r.n_unstaged) == want, r
    if r.sep:                                       # what the shared tables hold
        assert r.max_cols <= c["PX1"] and r.max_patch <= c["PR"] and r.n_unstaged == 0
    assert len(r.tiles) == -(-g.orig[0] // c["PTH"]) * -(-g.orig[1] // c["PTW"])
    assert g.inp[0] <= g.S and g.inp[1] <= g.S


# ------------------------------------------------------------------------------- the restatement against csrc/post_geom.h
SWEEP = range(1, 1101)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """-> run(requests) -> (lines of text, int16 array of index pairs): the stand-alone program over post_geom.h"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("post_geom_routes")
    exe = d / "post_geom_routes"
    # -ffp-contract=off: src_idx's one fma is written as fmaf; nothing else may fuse
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(P.ROOT, "tests", "native", "post_geom_routes.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(requests):
        src, dst = d / "requests.txt", d / "indices.bin"
        src.write_text("".join(q + "\n" for q in requests))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
        lines = r.stdout.splitlines()
        c = P.table_constants()
        assert lines[0].split() == ["C", str(c["PTW"]), str(c["PTH"]), "16", str(c["PR"]), str(c["PX1"])]
        assert len(lines) == 1 + len(requests)
        return lines[1:], np.fromfile(dst, dtype=np.int16)
    return run


def test_the_header_chooses_the_kernel_and_bounds_the_tiles_as_classify_says(routes):
    c = P.table_constants()
    lines, _ = routes([f"G {g.orig[0]} {g.orig[1]} {g.inp[0]} {g.inp[1]} {g.S} {g.low}" for g in P.GEOMS])
    assert len(lines) == len(P.GEOMS) == 18
    for g, line in zip(P.GEOMS, lines):
        r = P.classify(g, c)
        want = ["G", int(r.sep), len(r.tiles)] + [int(v) for t in r.tiles for v in t]
        assert line.split() == [str(v) for v in want], (P.geom_id(g), line[:200])


def test_the_header_agrees_on_every_extent_from_1_to_1100(routes):
    """per axis: the (crop, low-res, plane) combinations of GEOMS against every output extent -- the fit decision, the stage-1
    count and the patch side of every strip, and src_idx index for index (output -> stage 1 and stage 1 -> low-res)"""
    c = P.table_constants()
    combos = sorted({(g.inp[ax], g.low, g.S) for g in P.GEOMS for ax in (0, 1)})
    assert len(combos) >= 10 and {g.orig[ax] for g in P.GEOMS for ax in (0, 1)} <= set(SWEEP)
    req = [f"L {crop} {low} {S}" for crop, low, S in combos]
    req += [f"A {out} {crop} {low} {S}" for crop, low, S in combos for out in SWEEP]
    lines, idx = routes(req)
    o, fits = 0, 0
    for (crop, low, S), line in zip(combos, lines):
        assert line.split() == ["L", str(crop)]
        i0, i1 = P.src_idx(P._scale(low, S), np.arange(crop), low)
        assert np.array_equal(idx[o:o + 2 * crop].reshape(crop, 2), np.stack([i0, i1], 1)), (crop, low, S)
        o += 2 * crop
    k = len(combos)
    for crop, low, S in combos:
        for out in SWEEP:
            strips = P._axis(out, crop, low, S, c["PTW"])
            fit = P.sep_fits(out, crop, low, S, c)
            want = ["A", int(fit), len(strips)] + [v for s in strips for v in s]
            assert lines[k].split() == [str(v) for v in want], (out, crop, low, S, lines[k][:200])
            i0, i1 = P.src_idx(P._scale(crop, out), np.arange(out), crop)
            assert np.array_equal(idx[o:o + 2 * out].reshape(out, 2), np.stack([i0, i1], 1)), (out, crop, low, S)
            o += 2 * out
            k += 1
            fits += fit
    assert o == len(idx) and k == len(lines)
    assert 0 < fits < len(combos) * len(SWEEP)              # both decisions occur


def test_the_boundaries_and_tile_counts_are_the_named_ones():
    c = P.table_constants()
    R = {gid: P.classify(g, c) for gid, g in BY_ID.items()}
    PR, PX1 = c["PR"], c["PX1"]
    # the column table: exactly PX1 columns fit, one more sends the call to the per-pixel kernel although its patch fits
    assert R["147x110-in256x192-S256"].sep and R["147x110-in256x192-S256"].max_cols == PX1
    r = R["146x109-in256x192-S256"]
    assert not r.sep and r.max_cols == PX1 + 1 and r.max_patch <= PR and r.n_unstaged == 0
    # the patch: exactly PR is staged, PR + 1 columns are not
    r = R["87x65-in256x192-S256"]
    assert r.max_patch == PR and r.n_unstaged == 0 and len(r.tiles) == 4
    r = R["53x40-in256x192-S256"]
    assert len(r.tiles) == 1 and r.tiles[0].pw == PR + 1 and not r.tiles[0].staged
    r = R["64x64-in256x256-S256"]
    assert len(r.tiles) == 1 and (r.tiles[0].ph, r.tiles[0].pw) == (64, 64)          # the whole low-res plane
    assert len(R["13x9-in256x177-S256"].tiles) == 1 and len(R["1x1-in256x256-S256"].tiles) == 1
    r = R["700x900-in199x256-S256"]
    assert len(r.tiles) == 165 and r.max_patch == 7
    assert len(R["427x640-in683x1024-S1024"].tiles) == 70 and len(R["300x400-in768x1024-S1024"].tiles) == 35
    r = R["97x130-in764x1024-S1024"]
    assert (r.n_staged, r.n_unstaged) == (0, 6)
    # staged and unstaged tiles in ONE launch, with a patch that is too wide only, too tall only, and both
    r = R["65x65-in256x256-S256"]
    assert (r.n_staged, r.n_unstaged) == (1, 3)
    assert any(t.ph <= PR < t.pw for t in r.tiles) and any(t.pw <= PR < t.ph for t in r.tiles)
    assert any(t.ph > PR and t.pw > PR for t in r.tiles)


def test_the_cases_reach_every_route_of_the_list():
    """two kernels x remap on / off (the shared-table geometries also run with HGL_SAM_POST_SEP=0, so the per-pixel kernel sees
    every tile kind under both), vector and bytewise stores under each kernel, the one-tile launches with K = 8"""
    seen = set()
    for g in P.GEOMS:
        r = P.classify(g)
        assert 16 in P.batch_sizes(g) and 15 in P.batch_sizes(g)
        assert (8 in P.batch_sizes(g)) == (len(r.tiles) == 1)
        for K in P.batch_sizes(g):
            remap = K % 8 == 0
            for store, on in P.store_routes(g, K).items():
                if on:
                    seen.add((g.kernel, g.tiles, remap, store))
    for kernel, tiles in (("sep", "staged"), ("pix", "staged"), ("pix", "unstaged"), ("pix", "mixed")):
        for remap in (True, False):
            for store in ("vector", "bytewise"):
                assert (kernel, tiles, remap, store) in seen, (kernel, tiles, remap, store)
    small = BY_ID["13x9-in256x177-S256"]
    assert P.store_routes(small, 16) == {"vector": False, "bytewise": True}          # W < 16: no thread holds 16 pixels
    assert P.store_routes(BY_ID["192x256-in192x256-S256"], 15) == {"vector": True, "bytewise": False}
    assert [P.NAMES[i] for i in P.PICK8][4:] == ["const_off", "const_on", "corner_br", "ramp_y"]


def test_batches_are_slices_of_the_sixteen():
    g = P.GEOMS[2]
    n16, l16, _ = P.batch(g, 16)
    n15, l15, i15 = P.batch(g, 15)
    n8, l8, i8 = P.batch(g, 8)
    assert n15 == n16[:15] and np.array_equal(l15, l16[:15]) and i15 == tuple(range(15))
    assert n8 == tuple(n16[i] for i in P.PICK8) and np.array_equal(l8, l16[list(P.PICK8)])
    assert len({l.tobytes() for l in l16}) == 16                                     # distinct per candidate
    alive = P.passes_iou(P.IOU16, 0.7)
    assert alive.tolist() == [True, False, False, False, True, True, False, True, True, True, True, False, True, False, True, False]
    assert P.passes_iou(P.IOU16, -1e30).all()
    assert P.IOU16[2] == np.float32(0.7) and np.isnan(P.IOU16[3])                    # exactly the threshold, and NaN: dropped


# ---------------------------------------------------------------------------------------------------------------- reference
@geoms
def test_reference_agrees_with_the_float32_cpu_implementations(gid):
    g = BY_ID[gid]
    names, low, ref, tf, tol = world(gid)
    assert ref.dtype == np.float64 and ref.shape == (16,) + g.orig
    e_torch = np.abs(tf - ref).max()
    e_numpy = np.abs(S.postprocess_masks(low, g.inp, g.orig, g.S) - ref).max()
    print(f"{gid}: tol {tol:.3e}, torch float32 {e_torch:.3e}, numpy oracle {e_numpy:.3e}")
    assert e_torch <= tol and e_numpy <= tol


@geoms
def test_structured_planes_do_what_they_are_for(gid):
    g = BY_ID[gid]
    names, low, ref, tf, tol = world(gid)
    H, W = g.orig
    s = {n: i for i, n in enumerate(names)}
    # (the rounded weight 1 - l1 makes a blend of a constant differ from it in the last float32 bits)
    assert np.abs(ref[s["const_off"]] + 5).max() <= tol and np.abs(ref[s["const_on"]] - 5).max() <= tol
    if H * W == 1:
        return
    # one low-res pixel at a corner of the surviving region: the box touches the two edges of that corner and no other.
    # The pixel is on over the 3.5 stage-1 pixels next to the edge at weight >= 0.875 per axis up to 2.5 of them; the first
    # output pixel samples (ratio - 1) / 2 stage-1 pixels from the edge: below 5 : 1 the corner cannot be missed
    near = max(g.inp[0] / H, g.inp[1] / W) < 5
    for n, (top, left) in (("corner_tl", (True, True)), ("corner_tr", (True, False)), ("corner_bl", (False, True)),
                           ("corner_br", (False, False))):
        box = P.box_of(ref[s[n]] > tol)
        assert (box is not None) or not near, n
        if box is None:
            continue
        x0, y0, x1, y1 = box
        assert (y0 == 0) == top and (y1 == H - 1) == (not top or y1 - y0 + 1 == H), (n, (x0, y0, x1, y1))
        assert (x0 == 0) == left and (x1 == W - 1) == (not left or x1 - x0 + 1 == W), (n, (x0, y0, x1, y1))
    for n in ("ramp_x", "ramp_y"):
        assert (ref[s[n]] > 1).any() and (ref[s[n]] < -1).any()


@pytest.mark.parametrize("gid", ["20x193-in100x193-S256", "53x40-in256x192-S256"])
def test_both_kernels_see_masks_with_pixels_in_one_edge_row_or_column_only(gid):
    """the box reduction's "has pixels" bit (maxy | 0x80000000 with maxy == 0) and its maxima at H - 1 and W - 1: a corner
    plane whose only on-pixel is (0, W - 1), another at (H - 1, W - 1), one in row 0 only, one in the last row only -- under
    the shared-table kernel (and, forced, the per-pixel one) and under the per-pixel kernel's unstaged route"""
    g = BY_ID[gid]
    names, low, ref, tf, tol = world(gid)
    H, W = g.orig
    assert P.classify(g).sep == (gid == "20x193-in100x193-S256")
    box = {n: P.box_of(ref[names.index(n)] > tol) for n in names if n.startswith("corner")}
    assert box["corner_tr"] == (W - 1, 0, W - 1, 0) and box["corner_br"] == (W - 1, H - 1, W - 1, H - 1)
    assert box["corner_tl"][1::2] == (0, 0) and box["corner_bl"][1::2] == (H - 1, H - 1)
    for n, b in box.items():                     # ... and nothing undecided next to them: the checker fixes these boxes exactly
        assert b == P.box_of(ref[names.index(n)] > -tol), n


@geoms
def test_undecided_share_is_below_the_cap(gid):
    names, low, ref, tf, tol = world(gid)
    for off in sorted({p.off for p in P.PARAMS}):
        share = P.Bounds(ref, tol, off).undecided_share
        print(f"{gid}: offset {off}: undecided share max {share.max():.3e}")
        assert (share <= P.UNDECIDED_CAP).all(), (off, share.max())


# ------------------------------------------------------------------------------------------------------------------ checker
@geoms
def test_checker_accepts_a_correct_float32_implementation(gid):
    g = BY_ID[gid]
    names, low, ref, tf, tol = world(gid)
    for off in sorted({p.off for p in P.PARAMS}):
        b16 = P.Bounds(ref, tol, off)
        for K in P.batch_sizes(g):
            kn, _, idx = P.batch(g, K)
            b, iou = b16.take(idx), P.IOU16[list(idx)]
            for p in P.PARAMS:
                if p.off != off:
                    continue
                bad = P.check_outputs(b, kn, *P.outputs_from_logits(tf[list(idx)], iou, p), iou, p)
                assert not bad, (gid, K, p.name, bad[:8])


def test_outputs_from_logits_on_a_case_worked_by_hand():
    full = np.full((3, 2, 3), -2.0, dtype=np.float32)
    full[0, 0, 1] = 0.5; full[0, 1, 2] = 3.0            # box 1,0,2,1; inter 1 (> 1), union 2 (> -1): 0.5
    full[1] = 4.0                                       # all on: stability 1
    iou = np.array([0.9, 0.9, 0.1], dtype=np.float32)
    p = P.Params("hand", 1.0, 0.7, 1.0)
    masks, boxes, stab, keep = P.outputs_from_logits(full, iou, p)
    assert boxes.tolist() == [[1, 0, 2, 1], [0, 0, 2, 1], [0, 0, 0, 0]]
    assert stab.tolist() == [0.5, 1.0, 0.0] and keep.tolist() == [0, 1, 0] and masks.sum((1, 2)).tolist() == [2, 6, 0]
    _, boxes, stab, keep = P.outputs_from_logits(full, iou, P.Params("hand", 1.0, -1e30, 0.0))
    assert np.isnan(stab[2]) and keep.tolist() == [1, 1, 1] and boxes[2].tolist() == [0, 0, 0, 0]       # 0/0 survives


def test_stability_admissible_is_exact_on_points_and_an_interval_otherwise():
    f = np.float32
    assert P.stability_admissible(f(7) / f(9), (7, 7), (9, 9))
    assert not P.stability_admissible(f(6) / f(9), (7, 7), (9, 9))
    assert not P.stability_admissible(np.nextafter(f(7) / f(9), f(1)), (7, 7), (9, 9))
    assert P.stability_admissible(f(8) / f(10), (7, 8), (9, 10)) and not P.stability_admissible(f(6) / f(10), (7, 8), (9, 10))
    assert P.stability_admissible(f("nan"), (0, 0), (0, 3)) and not P.stability_admissible(f("nan"), (0, 0), (1, 3))
    assert not P.stability_admissible(f(0), (0, 0), (0, 0))


PLANT_GEOMS = ["160x200-in205x256-S256", "65x65-in256x256-S256", "333x500-in171x256-S256"]
NOFILTER, FILTER = P.PARAMS[0], P.PARAMS[1]


def good(gid, p):
    names, low, ref, tf, tol = world(gid)
    out = [np.array(a) for a in P.outputs_from_logits(tf, P.IOU16, p)]
    b = P.Bounds(ref, tol, p.off)
    assert not P.check_outputs(b, names, *out, P.IOU16, p)
    return names, tf, b, out


def hits(bad, name, quantity):
    return any(t[0] == name and t[1] == quantity for t in bad)


@pytest.mark.parametrize("gid", PLANT_GEOMS)
def test_checker_rejects_two_candidates_swapped(gid):
    """all four outputs of two candidates exchanged consistently -- what a wrong candidate map under the XCD remap would give"""
    for i, j in ((0, 1), (2, 7), (10, 11)):
        names, tf, b, out = good(gid, NOFILTER)
        for a in out:
            a[[i, j]] = a[[j, i]]
        bad = P.check_outputs(b, names, *out, P.IOU16, NOFILTER)
        assert hits(bad, names[i], "mask") and hits(bad, names[j], "mask"), bad


@pytest.mark.parametrize("gid", PLANT_GEOMS)
def test_checker_rejects_a_mask_shifted_by_one_pixel(gid):
    names, tf, b, out = good(gid, NOFILTER)
    for k in (3, P.NAMES.index("ramp_x"), P.NAMES.index("corner_tl")):
        masks = out[0].copy()
        masks[k] = np.roll(masks[k], 1, axis=1)
        boxes = out[1].copy()
        boxes[k] = P.box_of(masks[k]) or (0, 0, 0, 0)
        bad = P.check_outputs(b, names, masks, boxes, out[2], out[3], P.IOU16, NOFILTER)
        assert hits(bad, names[k], "mask") and {t[0] for t in bad} == {names[k]}, bad


@pytest.mark.parametrize("gid", PLANT_GEOMS)
@pytest.mark.parametrize("p", [P.PARAMS[0], P.PARAMS[2]], ids=lambda p: p.name)
def test_checker_rejects_a_counter_without_one_tiles_share(gid, p):
    """a workgroup's atomicAdd lost: inter or union lacks what one 64 x 64 tile counted"""
    names, tf, b, out = good(gid, p)
    H, W = tf.shape[1:]
    f = np.float32
    tried = 0
    for k in (0, 5, P.NAMES.index("const_on"), P.NAMES.index("ramp_y")):
        inter, union = int((tf[k] > f(p.off)).sum()), int((tf[k] > f(-p.off)).sum())
        ty, tx = range(0, H, 64), range(0, W, 64)
        for y0 in sorted({ty[0], ty[len(ty) // 2], ty[-1]}):           # the first, a middle and the last (partial) tile
            for x0 in sorted({tx[0], tx[-1]}):
                ti = int((tf[k, y0:y0 + 64, x0:x0 + 64] > f(p.off)).sum())
                tu = int((tf[k, y0:y0 + 64, x0:x0 + 64] > f(-p.off)).sum())
                for di, du in ((ti, 0), (0, tu)):
                    if di + du == 0 or union - du == 0:
                        continue
                    stab = out[2].copy()
                    stab[k] = f(inter - di) / f(union - du)
                    keep = out[3].copy()
                    keep[k] = 1 if (not p.stab_thr > 0 or stab[k] >= f(p.stab_thr)) else 0
                    bad = P.check_outputs(b, names, out[0], out[1], stab, keep, P.IOU16, p)
                    assert hits(bad, names[k], "stability"), (k, y0, x0, di, du, bad)
                    tried += 1
    assert tried >= 8


@pytest.mark.parametrize("gid", PLANT_GEOMS)
def test_checker_rejects_a_box_edge_off_by_one(gid):
    names, tf, b, out = good(gid, NOFILTER)
    H, W = tf.shape[1:]
    n = 0
    for k in (0, 6, P.NAMES.index("const_on"), P.NAMES.index("corner_br"), P.NAMES.index("ramp_x")):
        for e in range(4):
            for d in (-1, 1):
                boxes = out[1].copy()
                boxes[k, e] += d
                bad = P.check_outputs(b, names, out[0], boxes, out[2], out[3], P.IOU16, NOFILTER)
                assert hits(bad, names[k], "box") and hits(bad, names[k], "box of its own mask"), (k, e, d, bad)
                n += 1
    assert n == 40


@pytest.mark.parametrize("gid", PLANT_GEOMS)
def test_checker_rejects_a_box_for_an_empty_mask_and_pixels_of_a_filtered_candidate(gid):
    names, tf, b, out = good(gid, NOFILTER)
    H, W = tf.shape[1:]
    k = P.NAMES.index("const_off")
    for box in ((0, 0, W - 1, H - 1), (0, 0, 0, 1), (1, 0, 0, 0), (2**31 - 1, 2**31 - 1, 0, 0)):
        boxes = out[1].copy()
        boxes[k] = box
        assert hits(P.check_outputs(b, names, out[0], boxes, out[2], out[3], P.IOU16, NOFILTER), names[k], "box")
    stab = out[2].copy()
    stab[k] = 0.0                                        # 0/0 is NaN, not 0
    assert hits(P.check_outputs(b, names, out[0], out[1], stab, out[3], P.IOU16, NOFILTER), names[k], "stability")
    names, tf, b, out = good(gid, FILTER)
    dropped = np.nonzero(~P.passes_iou(P.IOU16, FILTER.iou_thr))[0]
    assert len(dropped) == 7
    for k in dropped[[0, 2, -1]]:
        masks = out[0].copy()
        masks[k, H - 1, W - 1] = 1
        assert hits(P.check_outputs(b, names, masks, *out[1:], P.IOU16, FILTER), names[k], "filtered mask")
        stab = out[2].copy()
        stab[k] = 0.5
        assert hits(P.check_outputs(b, names, out[0], out[1], stab, out[3], P.IOU16, FILTER), names[k], "filtered stability")
        keep = out[3].copy()
        keep[k] = 1
        assert hits(P.check_outputs(b, names, out[0], out[1], out[2], keep, P.IOU16, FILTER), names[k], "filtered keep")
    # ... and the survivors' keep flag follows from their stability (threshold 1.0: inter == union, as on the all-on plane)
    alive = P.passes_iou(P.IOU16, FILTER.iou_thr)
    assert out[3].tolist() == [int(a and s == 1.0) for a, s in zip(alive, out[2])] and out[3][names.index("const_on")] == 1
    assert out[3][0] == 0
    keep = out[3].copy()
    keep[0] = 1
    assert hits(P.check_outputs(b, names, out[0], out[1], out[2], keep, P.IOU16, FILTER), names[0], "keep")
