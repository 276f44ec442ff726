"""hgl_synthesize_views_prompt on the device against the numpy contract (tests/view_prompt_cases.py): 37 x 53 -> 32 and
97 x 130 -> 64, six masks (a seeded blob, a blob on a corner, empty, thin line, full, single pixel: boxes larger and smaller than
res).  (a) the default prompt writes hgl_synthesize_views' bits, also into out= slices; (b) every preset and a table of
single-field variations, at the tolerances of tests/test_gpu_primitives.py test_synthesize_views (2e-6 local, 5e-6 global);
(c) caller-supplied empty and out-of-image boxes; (d) the refusals."""
import numpy as np
import pytest
import torch

import view_prompt_cases as VC
from hybridgl_amd import _lib, ops

pytestmark = pytest.mark.gpu
ATOL_LOCAL, ATOL_GLOBAL = 2e-6, 5e-6


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module", params=VC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}to{s[2]}")
def world(request, cuda):
    H, W, res = request.param
    img, blur, norm, masks = VC.case_inputs(H, W)
    host = dict(img=img, blur=blur, norm=norm, masks=masks, boxes=VC.mask_boxes(masks), res=res, H=H, W=W)
    dev = dict(img=T(img, cuda), blur=T(blur, cuda), norm=T(norm, cuda), masks=T(masks, cuda))
    return host, dev


def _struct(p):
    return ops.view_prompt(**p)


def _check(world, p, boxes=None, blurred=True):
    """device against contract for prompt dict p; boxes None = the op computes them from the masks"""
    host, dev = world
    hb = boxes if boxes is not None else host["boxes"]
    want = VC.views(host["img"], host["blur"] if blurred else None, host["norm"], host["masks"], p, hb, host["res"])
    loc, glo = ops.synthesize_views_prompt(dev["img"], dev["blur"] if blurred else None, dev["norm"], dev["masks"], _struct(p),
                                           boxes=None if boxes is None else T(boxes, dev["img"].device), res=host["res"])
    el, eg = np.abs(loc.cpu().numpy() - want[0]).max(), np.abs(glo.cpu().numpy() - want[1]).max()
    print(f"{ {k: v for k, v in p.items() if v != VC.DEFAULT[k]} }: max |local| {el:.3g}, max |global| {eg:.3g}")
    np.testing.assert_allclose(loc.cpu().numpy(), want[0], rtol=0, atol=ATOL_LOCAL)
    np.testing.assert_allclose(glo.cpu().numpy(), want[1], rtol=0, atol=ATOL_GLOBAL)
    return loc, glo


def test_mask_boxes_are_the_contracts(world):
    from hybridgl_amd import sam
    host, dev = world
    assert np.array_equal(sam.mask_boxes(dev["masks"].view(torch.uint8)).cpu().numpy(), host["boxes"])


def test_default_prompt_is_the_old_kernel_bit_for_bit(world):
    host, dev = world
    res, N = host["res"], VC.N_MASKS
    old = ops.synthesize_views(dev["img"], dev["blur"], dev["norm"], dev["masks"], res)
    for p in (ops.view_prompt(), ops.view_prompt("hybridgl", pad_permille=250, square=1, thickness=7, grow=3)):
        new = ops.synthesize_views_prompt(dev["img"], dev["blur"], dev["norm"], dev["masks"], p, res=res)
        assert torch.equal(old[0].view(torch.int32), new[0].view(torch.int32))
        assert torch.equal(old[1].view(torch.int32), new[1].view(torch.int32))
    # into slices of a larger pair, as the grouped pipeline writes them; the rows around stay untouched
    loc = torch.full((N + 3, 3, res, res), 7.0, device=dev["img"].device)
    glo = torch.full_like(loc, -3.0)
    got = ops.synthesize_views_prompt(dev["img"], dev["blur"], dev["norm"], dev["masks"], ops.view_prompt(), res=res,
                                      out=(loc[2:2 + N], glo[2:2 + N]))
    assert got[0].data_ptr() == loc[2].data_ptr()
    assert torch.equal(loc[2:2 + N], old[0]) and torch.equal(glo[2:2 + N], old[1])
    assert bool((loc[:2] == 7).all()) and bool((loc[2 + N:] == 7).all()) and bool((glo[:2] == -3).all()) and bool((glo[2 + N:] == -3).all())


@pytest.mark.parametrize("name", list(VC.PRESETS))
def test_presets_against_the_contract(world, name):
    p = VC.prompt(name)
    loc, glo = _check(world, p, blurred=p["global_bg"] == 0)
    assert VC.DEFAULT == VC.prompt() and ops.view_prompt_fields(ops.view_prompt(name))["marker"] == p["marker"]
    if name == "red_circle":      # the marker is there: some pixel of the full mask's view differs from the plain `keep`
        plain = _check(world, VC.prompt("keep"), blurred=False)[1]
        assert not torch.equal(plain, glo)


@pytest.mark.parametrize("k", range(len(VC.VARIATIONS)), ids=lambda k: "-".join(f"{a}{b}" for a, b in VC.VARIATIONS[k].items() if not isinstance(b, tuple)))
def test_single_field_variations_against_the_contract(world, k):
    _check(world, VC.prompt(**VC.VARIATIONS[k]))


def test_marker_crossing_the_border(world):
    """the corner blob's box touches two edges: its grown band leaves the image and is cut there; in a padded box window the part
    of the view beyond the edge is the fill colour"""
    host, _ = world
    assert host["boxes"][1][1] == 0 and host["boxes"][1][2] == host["W"] - 1
    for marker in (1, 2):
        _check(world, VC.prompt(marker=marker, thickness=3, grow=4, global_bg=1))
        _check(world, VC.prompt(marker=marker, thickness=3, grow=4, global_bg=3, global_fill=(9, 90, 200), window=1, pad_permille=1000, square=1))


def test_caller_supplied_empty_and_out_of_image_boxes(world):
    host, _ = world
    boxes = VC.caller_boxes(host["H"], host["W"])
    for p in (VC.prompt("masked_crop"), VC.prompt("crop", pad_permille=250), VC.prompt("red_circle", thickness=3),
              VC.prompt(window=1, marker=2, thickness=2, grow=1, global_bg=2)):
        _check(world, p, boxes=boxes)
    # an empty box is the frame without a marker: rows 0 and 1 under a box window with a marker are the plain frame's
    loc, glo = _check(world, VC.prompt("keep", window=1, marker=1), boxes=boxes, blurred=False)
    plain = _check(world, VC.prompt("keep"), blurred=False)
    assert torch.equal(loc[:2], plain[0][:2]) and torch.equal(glo[:2], plain[1][:2])


def test_refusals(world):
    host, dev = world
    N, res = VC.N_MASKS, host["res"]
    args = lambda: [dev["img"], dev["blur"], dev["norm"], dev["masks"]]

    def refused(why, fn):
        with pytest.raises(_lib.HybridGLError, match=why):
            fn()
    # one message per rule of view_prompt.h, through the struct (ops.view_prompt refuses the ranges itself: set them after)
    for why, fields, H, W, hb, hx in VC.REFUSALS:
        if (H, W) != (10, 10):
            continue
        p = ops.view_prompt()
        for k, v in fields.items():
            if k == "local_fill":
                p.local_fill[:] = v
            else:
                setattr(p, k, v)
        boxes = torch.zeros((N, 4), dtype=torch.int32, device=dev["img"].device) if hx else None
        lib = _lib.load()
        import ctypes as C
        loc = torch.empty((N, 3, res, res), device=dev["img"].device)
        glo = torch.empty_like(loc)
        rc = lib.hgl_synthesize_views_prompt(dev["img"].data_ptr(), dev["blur"].data_ptr() if hb else None, dev["norm"].data_ptr(),
                                             dev["masks"].view(torch.uint8).data_ptr(), boxes.data_ptr() if boxes is not None else None,
                                             N, host["H"], host["W"], res, C.byref(p), loc.data_ptr(), glo.data_ptr(), None)
        assert rc == -1 and why in lib.hgl_last_error().decode(), (why, lib.hgl_last_error())
    refused("a blur background needs the blurred image",
            lambda: ops.synthesize_views_prompt(dev["img"], None, dev["norm"], dev["masks"], ops.view_prompt(), res=res))
    # H above 8192: refused before anything is read (the tensors are small; only the shape is large)
    lib = _lib.load()
    import ctypes as C
    one = torch.zeros(16, dtype=torch.uint8, device=dev["img"].device)
    f = torch.zeros(16, device=dev["img"].device)
    for H, W in ((8193, 1), (1, 8193)):
        rc = lib.hgl_synthesize_views_prompt(one.data_ptr(), one.data_ptr(), f.data_ptr(), one.data_ptr(), None, 1, H, W, 2,
                                             C.byref(ops.view_prompt()), f.data_ptr(), f.data_ptr(), None)
        assert rc == -1 and "image side outside 1..8192" in lib.hgl_last_error().decode()
    # null required pointers
    for hole in (0, 2, 3, 9, 10, 11):
        a = [one.data_ptr(), one.data_ptr(), f.data_ptr(), one.data_ptr(), None, 1, 2, 2, 2, C.byref(ops.view_prompt()), f.data_ptr(), f.data_ptr(), None]
        a[hole] = None
        assert lib.hgl_synthesize_views_prompt(*a) == -1 and "null argument" in lib.hgl_last_error().decode()
    # the binding's own checks
    with pytest.raises(ValueError, match="boxes"):
        ops.synthesize_views_prompt(*args(), ops.view_prompt("crop"), boxes=torch.zeros((N + 1, 4), dtype=torch.int32, device=dev["img"].device), res=res)
    with pytest.raises(TypeError, match="boxes"):
        ops.synthesize_views_prompt(*args(), ops.view_prompt("crop"), boxes=torch.zeros((N, 4), dtype=torch.int64, device=dev["img"].device), res=res)
