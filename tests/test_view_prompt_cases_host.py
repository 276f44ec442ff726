"""The numpy contract of a visual prompt (tests/view_prompt_cases.py) and the prompt builder / parser of hybridgl_amd.ops, on
the host: at the default prompt the contract is oracle.clip_oracle.synthesize_views bit for bit; windows, band pixel counts and
a box hanging over every image edge checked by hand; the presets and the parser's refusals; the result log's header names a
non-default prompt."""
import argparse

import numpy as np
import pytest

import view_prompt_cases as VC
from oracle import clip_oracle as O


@pytest.mark.parametrize("H,W,res", VC.SHAPES)
def test_default_prompt_is_the_oracle_bit_for_bit(H, W, res):
    img, blur, norm, masks = VC.case_inputs(H, W)
    rl, rg = O.synthesize_views(img, blur, norm, masks, res)
    for p, boxes in [(VC.prompt(), None), (VC.prompt("hybridgl", pad_permille=250, square=1, thickness=9, grow=11), VC.mask_boxes(masks))]:
        loc, glo = VC.views(img, blur, norm, masks, p, boxes, res)      # the box fields say nothing under a frame window
        assert loc.dtype == rl.dtype == np.float32 and np.array_equal(loc.view(np.uint32), rl.view(np.uint32))
        assert np.array_equal(glo.view(np.uint32), rg.view(np.uint32))


def test_windows_by_hand():
    sq = VC.prompt(window=1, square=1, pad_permille=250)
    assert VC.window(sq, [3, 7, 3, 30], 40, 40) == (-15, 1, 36, 36)      # 1 x 24: m = 6, s = 36, floor(-29 / 2), floor(2 / 2)
    assert VC.window(VC.prompt(window=1, pad_permille=250), [3, 7, 3, 30], 40, 40) == (-3, 1, 13, 36)
    assert VC.window(VC.prompt(window=1), [5, 5, 5, 5], 40, 40) == (5, 5, 1, 1)      # a 1 x 1 box has a 1 x 1 window
    assert VC.window(VC.prompt(window=1, square=1), [5, 5, 5, 5], 40, 40) == (5, 5, 1, 1)
    assert VC.window(VC.prompt(window=1, square=1), [10, 20, 19, 23], 40, 40) == (10, 17, 10, 10)      # 10 x 4 about its centre
    assert VC.window(VC.prompt(window=1, square=1), [10, 20, 18, 23], 40, 40) == (10, 17, 9, 9)        # floor((20 + 23 + 1 - 9) / 2)
    assert VC.window(VC.prompt(window=1, pad_permille=4000), [0, 0, 39, 39], 40, 40) == (-160, -160, 360, 360)
    assert VC.window(VC.prompt(window=0, pad_permille=250, square=1), [3, 7, 3, 30], 40, 31) == (0, 0, 31, 40)      # the frame
    assert VC.window(VC.prompt(window=1), [9, 4, 8, 20], 40, 31) == (0, 0, 31, 40)                   # the empty box: the frame
    assert VC.window(VC.prompt(window=1), None, 40, 31) == (0, 0, 31, 40)


def test_a_box_hanging_over_every_edge_is_the_image():
    H, W = 37, 53
    assert VC.clamp_box([-7, -9, W + 11, H + 3], H, W) == (0, 0, W - 1, H - 1, False)
    assert VC.window(VC.prompt(window=1), [-7, -9, W + 11, H + 3], H, W) == (0, 0, W, H)
    assert VC.clamp_box([-40, -30, -5, -2], H, W) == (0, 0, 0, 0, False)      # wholly outside: the corner pixel
    assert VC.clamp_box([60, 4, 55, 9], H, W)[4]                               # inverted as given: empty wherever it lies
    # with that window and the default colours the views are the frame's
    img, blur, norm, masks = VC.case_inputs(H, W)
    boxes = np.tile(np.array([[-7, -9, W + 11, H + 3]], np.int32), (len(masks), 1))
    a = VC.views(img, blur, norm, masks, VC.prompt(window=1), boxes, 32)
    b = VC.views(img, blur, norm, masks, VC.prompt(), None, 32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_taps_stay_in_the_window_and_leave_the_image_only_through_it():
    for extent, origin, res in [(1, 5, 8), (36, -15, 32), (360, -160, 64), (53, 0, 32), (8192 * 9, -32768, 224)]:
        i0, i1, l0, l1 = VC.taps(res, extent, origin)
        assert i0.min() >= origin and i1.max() <= origin + extent - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
        assert (l0 + l1 == 1).all() and (l1 >= 0).all() and (l1 < 1).all()


def _band(p, box, H=64, W=64):
    return VC.marker_band(p, box, H, W)


def test_band_pixel_counts_by_hand():
    box = [20, 30, 29, 35]      # 10 x 6
    for g, t in [(0, 1), (0, 3), (2, 1), (2, 3)]:
        n = _band(VC.prompt(marker=2, grow=g, thickness=t), box).sum()
        assert n == (10 + 2 * (g + t)) * (6 + 2 * (g + t)) - (10 + 2 * g) * (6 + 2 * g)
    # a 1 x 1 box, ellipse at t = 1, g = 0: DX, DY in {-2, 0, 2}; A = B = 3 holds DX^2 + DY^2 <= 9, the whole 3 x 3 block (a corner
    # is 4 + 4), A = B = 1 the centre alone
    ring = _band(VC.prompt(marker=1), [10, 10, 10, 10])
    assert ring.sum() == 8 and ring[9:12, 9:12].sum() == 8 and not ring[10, 10]
    # a 4 x 4 box: the inner ellipse (A = B = 4: DX^2 + DY^2 <= 16 over odd DX, DY in -3 .. 3) holds 12 pixels, the outer
    # (A = B = 6: <= 36 over -5 .. 5) 32: 36 without the four corners, where 25 + 25 > 36
    assert _band(VC.prompt(marker=1), [10, 10, 13, 13]).sum() == 32 - 12
    # at t = 1 the ring is closed for boxes up to about 2 : 1: every pixel of the inner ellipse's 4-neighbourhood that is not
    # inside it is on the band.  (Not for longer ones, 19 x 58 already: at 2 x 44 the inner ellipse's column reaches |DY| <= 38 where the outer
    # ellipse's next column ends at |DY| <= 30 -- such a box wants thickness >= 2.)
    for box in ([5, 9, 40, 23], [12, 20, 30, 50], [0, 0, 63, 63], [30, 30, 30, 30], [10, 10, 13, 13]):
        for g in (0, 2):
            band = _band(VC.prompt(marker=1, grow=g), box)
            x0, y0, x1, y1 = box
            y, x = np.mgrid[0:64, 0:64].astype(np.int64)
            DX, DY = 2 * x + 1 - (x0 + x1 + 1), 2 * y + 1 - (y0 + y1 + 1)
            A, B = x1 - x0 + 1 + 2 * g, y1 - y0 + 1 + 2 * g
            ins = DX * DX * B * B + DY * DY * A * A <= A * A * B * B
            nb = np.zeros_like(ins)
            nb[1:] |= ins[:-1]; nb[:-1] |= ins[1:]; nb[:, 1:] |= ins[:, :-1]; nb[:, :-1] |= ins[:, 1:]
            assert (band[nb & ~ins]).all() and not (band & ins).any(), (box, g)
    # no marker for the empty box, none outside the band's reach, and the marker crossing the border is cut at it
    assert not _band(VC.prompt(marker=1, thickness=5), [9, 4, 8, 20]).any()
    assert _band(VC.prompt(marker=2, thickness=3, grow=2), [0, 0, 9, 9]).sum() == 15 * 15 - 12 * 12


def test_gray_and_backgrounds():
    px = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], np.uint8)
    assert VC.gray(px).tolist() == [[255, 0, 77, 149, 29, (770 + 30000 + 870 + 128) >> 8]]
    H, W = 37, 53
    img, blur, norm, masks = VC.case_inputs(H, W)
    empty = np.zeros((1, H, W), bool)
    full = np.ones((1, H, W), bool)
    # a full mask sees no background at all; an empty one under `keep` is the full one
    ref = VC.views(img, None, norm, full, VC.prompt("keep"), None, 32)
    for name in ("black", "gray", "keep"):
        got = VC.views(img, None, norm, full, VC.prompt(name), None, 32)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    kept = VC.views(img, None, norm, empty, VC.prompt("keep", local_bg=1), None, 32)
    assert np.array_equal(kept[0], ref[0]) and np.array_equal(kept[1], ref[1])
    black = VC.views(img, None, norm, empty, VC.prompt("black"), None, 32)[1]
    assert np.allclose(black, ((0 - O.IMAGENET_MEAN) / O.IMAGENET_STD)[None, :, None, None], atol=1e-6)
    # a window that leaves the image: the part outside is the fill in both views, whatever the background kind
    p = VC.prompt("keep", window=1, pad_permille=4000, local_bg=1, global_fill=(255, 255, 255))
    loc, glo = VC.views(img, None, norm, full, p, np.array([[0, 0, W - 1, H - 1]], np.int32), 32)
    assert np.array_equal(loc[0, :, 0, 0], np.asarray(p["local_fill"], np.float32))
    assert np.allclose(glo[0, :, 0, 0], (1 - O.IMAGENET_MEAN) / O.IMAGENET_STD, atol=1e-6)


def test_refusals_one_per_rule():
    for why, fields, H, W, hb, hx in VC.REFUSALS:
        assert VC.refusal(VC.prompt(**fields), H, W, hb, hx) == why
    assert VC.refusal(VC.prompt("keep"), 8192, 8192, False, False) is None


# ---- hybridgl_amd.ops: the struct builder and the command line's parser (no device, no library) ----
def _fields(p):
    from hybridgl_amd import ops
    return ops.view_prompt_fields(p)


def test_presets_are_the_contracts():
    from hybridgl_amd import ops
    assert list(ops.VIEW_PROMPT_PRESETS) == list(VC.PRESETS) == ["hybridgl", "black", "gray", "keep", "red_circle", "masked_crop", "crop"]
    for name in VC.PRESETS:
        got, want = _fields(ops.view_prompt(name)), VC.prompt(name)
        assert {k: got[k] for k in want if k != "local_fill"} == {k: want[k] for k in want if k != "local_fill"}
        assert np.array_equal(np.asarray(got["local_fill"], np.float32), np.asarray(want["local_fill"], np.float32))
        assert ops.view_prompt_name(ops.view_prompt(name)) == name
        assert ops.view_prompt_is_default(ops.view_prompt(name)) == (name == "hybridgl")
    assert ops.view_prompt_is_default(None)
    rc = _fields(ops.view_prompt("red_circle"))
    assert (rc["global_bg"], rc["marker"], rc["marker_rgb"]) == (1, 1, (255, 0, 0))
    assert (_fields(ops.view_prompt("crop"))["window"], _fields(ops.view_prompt("crop"))["square"], _fields(ops.view_prompt("crop"))["local_bg"]) == (1, 1, 1)


def test_parser_accepts_presets_and_pairs():
    from hybridgl_amd import ops
    assert ops.parse_view_prompt(None) is None and ops.parse_view_prompt("") is None
    assert _fields(ops.parse_view_prompt("gray")) == _fields(ops.view_prompt("gray"))
    p = _fields(ops.parse_view_prompt("red_circle, thickness=3 ,marker_rgb=0:255:64,grow=2"))
    assert (p["marker"], p["thickness"], p["marker_rgb"], p["grow"], p["global_bg"]) == (1, 3, (0, 255, 64), 2, 1)
    p = _fields(ops.parse_view_prompt("window=box,square=on,pad_permille=250,local_bg=keep,global_bg=fill,global_fill=1:2:3"))
    assert (p["window"], p["square"], p["pad_permille"], p["local_bg"], p["global_bg"], p["global_fill"]) == (1, 1, 250, 1, 3, (1, 2, 3))
    assert ops.view_prompt_name(ops.parse_view_prompt("marker=box,thickness=4")) == "marker=2,thickness=4"
    assert _fields(ops.parse_view_prompt(ops.view_prompt_name(ops.parse_view_prompt("gray,marker=box,marker_rgb=1:2:3")))) == \
        _fields(ops.parse_view_prompt("gray,marker=box,marker_rgb=1:2:3"))


@pytest.mark.parametrize("spec,key", [
    ("sepia", "sepia"), ("gray,colour=3", "colour"), ("thickness=0", "thickness"), ("thickness=65", "thickness"), ("grow=4097", "grow"),
    ("pad_permille=-1", "pad_permille"), ("pad_permille=4001", "pad_permille"), ("window=circle", "window"), ("marker=3", "marker"),
    ("global_bg=white", "global_bg"), ("local_bg=2", "local_bg"), ("square=2", "square"), ("marker_rgb=255:0", "marker_rgb"),
    ("marker_rgb=256:0:0", "marker_rgb"), ("global_fill=a:b:c", "global_fill"), ("local_fill=0:nan:0", "local_fill"),
    ("thickness=2.5", "thickness"), ("grow", "grow"), ("grow=", "grow"), ("grow=1,grow=2", "grow")])
def test_parser_names_the_offending_key(spec, key):
    from hybridgl_amd import ops
    with pytest.raises(ValueError, match=key):
        ops.parse_view_prompt(spec)


def test_the_result_header_names_a_non_default_prompt():
    from hybridgl_amd.main import report_text
    m = dict(oIoU=1.0, mIoU=2.0, oIoU_final=3.0, mIoU_final=4.0)
    base = argparse.Namespace(fusion_mode="G2L", dataset="refcoco", split="val")
    plain = report_text(base, m)
    assert report_text(argparse.Namespace(**vars(base), view_prompt=""), m) == plain == report_text(argparse.Namespace(**vars(base), view_prompt="hybridgl"), m)
    named = report_text(argparse.Namespace(**{**vars(base), "fusion_mode": "crop"}, view_prompt="masked_crop"), m)
    assert named.split("\n")[2] == " fusion_mode=crop view_prompt=masked_crop "
    assert "view_prompt=marker=2,thickness=4" in report_text(argparse.Namespace(**vars(base), view_prompt="marker=box,thickness=4"), m)
