"""hgl_heat_paint_device on the GPU against the contract in numpy (tests/heat_cases.py), byte for byte: out, levels and status.
Sizes from one pixel to more than one share of a map, all four directions, canvases at every p % 4 with gaps that must keep
their fence, shared heat extents and shared bases, base NULL, levels NULL, huge values, NaN, inf, flat maps, a peak at weight 0,
a ramp whose weights are not finite, two calls with equal bytes, and the weight the kernel used against ops.gen_dir_mask."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops, render
from hybridgl_amd import utils as U

import heat_cases as HC

pytestmark = pytest.mark.gpu

FENCE = 0xA5
TAIL = 5      # fenced pixels behind the last canvas


def run(call, cuda, with_levels=True, misalign=0):
    """ops.heat_paint twice into fenced buffers -> (out [P,3], levels [P] or None, status [M,4]) as numpy.  misalign: bytes
    the out / levels / base buffers are shifted by from their allocation's start."""
    P = call["canvas"] + TAIL
    heat = torch.from_numpy(call["heat"]).to(cuda)
    ramp = torch.from_numpy(call["ramp"].view(np.int32).copy()).to(cuda)
    base = None
    if call["base"] is not None:
        base = torch.zeros(call["base"].size + misalign, dtype=torch.uint8, device=cuda)[misalign:]
        base.copy_(torch.from_numpy(call["base"].reshape(-1).copy()))
    got = []
    for _ in range(2):
        out = torch.full((3 * P + misalign,), FENCE, dtype=torch.uint8, device=cuda)[misalign:]
        lev = torch.full((P + misalign,), FENCE, dtype=torch.uint8, device=cuda)[misalign:] if with_levels else False
        pics, levels, status = ops.heat_paint(heat, call["maps"], ramp, base=base, out=out, levels=lev)
        assert [tuple(p.shape) for p in pics] == [(int(r[0]), int(r[1]), 3) for r in call["maps"]]
        assert (levels is None) == (not with_levels)
        got.append((out.cpu().numpy().reshape(-1, 3), lev.cpu().numpy() if with_levels else None, status.cpu().numpy()))
    assert all(a is None or np.array_equal(a, b) for a, b in zip(got[0], got[1])), "two calls differ"
    return got[0]


def check(call, cuda, with_levels=True, misalign=0):
    out, levels, status = HC.expect(call, with_levels, FENCE, TAIL)
    g_out, g_lev, g_status = run(call, cuda, with_levels, misalign)
    assert np.array_equal(g_status, status), [(m, g_status[m].tolist(), status[m].tolist()) for m in np.flatnonzero((g_status != status).any(1))[:5]]
    if with_levels:
        assert np.array_equal(g_lev, levels), np.argwhere(g_lev != levels)[:5].tolist()
    assert np.array_equal(g_out, out), np.argwhere(g_out != out)[:5].tolist()
    return status


def test_every_size_under_every_direction(cuda):
    call = HC.all_sizes_call()
    assert {int(p) % 4 for p in call["maps"][:, 5]} == {0, 1, 2, 3} and len(call["maps"]) == 32
    status = check(call, cuda)
    # (1,1) is flat; a W = 1 map has no weight under `right`; everything else paints
    codes = {(tuple(s["size"]), s["dir"]): int(c) for s, c in zip(call["specs"], status[:, 0])}
    assert all(codes[((1, 1), d)] == 1 for d in range(4)) and codes[((3, 1), 2)] == 3 and codes[((3, 1), 1)] == 0
    assert all(c == 0 for (size, d), c in codes.items() if size[1] > 3)


@pytest.mark.parametrize("size", HC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_map_alone(cuda, size):
    for d in range(4):
        check(HC.make_call(20 + d, [dict(size=size, dir=d)], gaps=[d]), cuda)


def test_64_maps_of_mixed_sizes_and_kinds(cuda):
    call = HC.mixed_call()
    maps = call["maps"]
    assert len(maps) == 64 and {int(p) % 4 for p in maps[:, 5]} == {0, 1, 2, 3}
    assert maps[1, 3] == maps[2, 3] == maps[3, 3] and len({int(d) for d in maps[1:4, 2]}) == 3      # one heat extent, three directions
    assert maps[3, 4] == maps[5, 4] == maps[6, 4]                                                    # three maps over one base
    status = check(call, cuda)
    assert {0, 1, 2} <= set(status[:, 0].tolist())
    for m in (9, 10, 11):      # the maximum sits where the weight is 0: painted all the same, the peak comes from elsewhere
        H, W, d, h = (int(v) for v in maps[m, :4])
        x = call["heat"][h:h + H * W].reshape(H, W)
        assert status[m, 0] == 0 and HC.dir_w(d, W)[np.unravel_index(x.argmax(), x.shape)[1]] == 0


def test_black_canvases_levels_off_and_unaligned_buffers(cuda):
    specs = [dict(size=s, dir=(k + 1) % 4, kind=kind) for k, (s, kind) in
             enumerate(zip(HC.SIZES[3:], ["rand", "rand", "huge", "rand", "rand"]))]
    for with_base in (False, True):
        call = HC.make_call(31, specs, with_base=with_base, gaps=[2, 1, 0, 3, 1])
        check(call, cuda, with_levels=False)
        check(call, cuda, with_levels=True)
    for misalign in (1, 2, 3):      # out, levels and base at any byte: the bytes move one by one
        check(HC.make_call(32, specs, gaps=[0, 1, 2, 3, 0]), cuda, misalign=misalign)


def test_non_finite_values_flat_maps_and_huge_ranges(cuda):
    kinds = ["nan", "inf", "flat", "range", "huge", "ties", "rand"]
    specs = [dict(size=(97, 131) if k % 2 else (5, 67), dir=k % 4, kind=kind) for k, kind in enumerate(kinds)]
    status = check(HC.make_call(33, specs, gaps=[1] * 7), cuda)
    assert status[:, 0].tolist() == [2, 2, 1, 2, 0, 0, 0] and not status[:4, 1:].any()


def test_a_ramp_with_weights_that_are_not_finite(cuda):
    call = HC.make_call(34, [dict(size=(97, 131), dir=0), dict(size=(7, 64), dir=3)], ramp=HC.broken_ramp(), gaps=[3, 2])
    _, levels, _ = HC.expect(call)
    assert {0, 7, 128, 200, 255} <= set(levels[3:3 + 97 * 131].tolist())      # the broken levels are painted
    check(call, cuda)


def test_render_heatmap_and_the_named_ramps(cuda):
    rng = np.random.default_rng(35)
    img = rng.integers(0, 256, (37, 50, 3), dtype=np.uint8)
    x = (rng.standard_normal((37, 50)) * 2).astype(np.float32)
    heat, image = torch.from_numpy(x).to(cuda), torch.from_numpy(img).to(cuda)
    for name in ("heat", "grey"):
        for d in ("none", "left", "right", "middle"):
            call = dict(heat=x.reshape(-1), maps=np.array([[37, 50, ops.DIRFLAG[d], 0, 0, 0]]), ramp=render.ramp(name), base=img.reshape(-1, 3),
                        canvas=37 * 50)
            want, _, _ = HC.expect(call, tail=0)
            assert np.array_equal(render.heatmap(image, heat, d, ramp=name).cpu().numpy(), want.reshape(37, 50, 3)), (name, d)
    # a group: two sentences over one image, one map under two directions, a second image of another size
    img2 = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    x2 = rng.standard_normal((9, 13)).astype(np.float32)
    heat2 = torch.from_numpy(x2).to(cuda)
    pics, levels, status = render.heatmap_group([image, torch.from_numpy(img2).to(cuda)], [heat, heat, heat2], ["left", "right", "middle"],
                                                image_of=[0, 0, 1], levels=True)
    assert status[:, 0].tolist() == [0, 0, 0]
    for pic, lev, (xx, d, im) in zip(pics, levels, [(x, 1, img), (x, 2, img), (x2, 3, img2)]):
        _, _, _, _, L = HC.levels_of(xx, d)
        assert np.array_equal(lev.cpu().numpy(), L) and np.array_equal(pic.cpu().numpy(), HC.blend_levels(im, L, render.ramp("heat")))
    black = render.heatmap(None, heat2, "none", ramp="grey").cpu().numpy()
    assert np.array_equal(black[..., 0], HC.levels_of(x2, 0)[4]) and np.array_equal(black[..., 0], black[..., 2])


@pytest.mark.parametrize("size", [(1, 1), (1, 2), (1, 3), (2, 5), (5, 67), (7, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_weight_the_kernel_used_is_gen_dir_mask(cuda, size):
    """a map that is 1 everywhere but one 0 normalises to itself, so the grey picture is rint(w / max w * 255) of the weight
    the device's own gen_dir_mask returns -- the mask the scoring tail multiplies with"""
    H, W = size
    for d, name in enumerate(HC.DIRS):
        x = HC.fill(np.random.default_rng(0), H, W, "onezero")      # (1,1): the one 0 alone, a flat map
        pic, lev, status = ops.heat_paint(torch.from_numpy(x).to(cuda), np.array([[H, W, d, 0, 0, 0]]), HC.grey_ramp(), levels=True)
        w = U.gen_dir_mask(name, H, W, cuda).cpu().numpy()
        assert np.array_equal(w[0], HC.dir_w(d, W))
        g = (x * w).astype(np.float32)
        if H * W == 1 or g.max() == 0:
            assert int(status[0, 0]) in (1, 3) and not lev[0].any()
            continue
        want = np.rint((g / g.max()).astype(np.float32) * np.float32(255)).astype(np.uint8)
        assert int(status[0, 0]) == 0 and np.array_equal(lev[0].cpu().numpy(), want)
        assert np.array_equal(pic[0].cpu().numpy(), np.repeat(want[..., None], 3, axis=2))


def test_refusals_leave_the_buffers_alone(cuda):
    lib = _lib.load()
    heat = torch.zeros(64, device=cuda)
    out = torch.full((3 * 64,), FENCE, dtype=torch.uint8, device=cuda)
    status = torch.full((1, 4), -7, dtype=torch.int32, device=cuda)
    ramp = torch.from_numpy(HC.grey_ramp().view(np.int32).copy()).to(cuda)
    ws = ops.workspace(4096, cuda, "rle")
    call = lambda maps, he=64, cp=64, o=None, b=None, wsb=None: lib.hgl_heat_paint_device(
        heat.data_ptr(), he, np.asarray(maps, dtype=np.int64).ctypes.data, len(maps), ramp.data_ptr(), b, out.data_ptr() if o is None else o,
        cp, None, status.data_ptr(), ws.data_ptr(), ws.numel() if wsb is None else wsb, None)
    for maps, kw, why in [([[8, 8, 4, 0, 0, 0]], {}, b"dirflag 4"), ([[8, 9, 0, 0, 0, 0]], {}, b"of heat"), ([[8, 8, 0, 0, 0, 1]], {}, b"lie outside"),
                          ([[4, 8, 0, 0, 0, 0], [4, 8, 1, 0, 0, 31]], {}, b"overlap"), ([[8, 8, 0, 0, 0, 0]], dict(b=out.data_ptr() + 8), b"out overlaps base")]:
        assert call(maps, **kw) == -1 and why in lib.hgl_last_error(), (maps, lib.hgl_last_error())
    assert call([[8, 8, 0, 0, 0, 0]], wsb=16) == -3 and b"workspace" in lib.hgl_last_error()
    torch.cuda.synchronize()
    assert bool((out == FENCE).all()) and bool((status == -7).all())
    with pytest.raises(ValueError):
        ops.heat_paint(heat, [[8, 8, 0, 0, 0, 1]], HC.grey_ramp(), out=out)
