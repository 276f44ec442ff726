"""The contract of hgl_heat_paint_device (include/hybridgl.h) in numpy float32, operation by operation, the cases the GPU test
paints, and heat_paint_plan (csrc/rle_group.h) as Python arithmetic for tests/native/heat_paint_sanitize.cpp.

The direction weight comes from torch.linspace on the CPU, composed as gen_dir_mask composes it (utils.py:135-161): left =
linspace(1, 0, W), right = linspace(0, 1, W), middle = cat(linspace(0, 1, W // 2), linspace(1, 0, W - W // 2)), else ones.
Every numpy operation below works on float32 arrays and so rounds to float32 on its own, as the contract asks."""
import numpy as np

f32 = np.float32
DIRS = ("none", "left", "right", "middle")


def dir_w(dirflag, W):
    """the column weights of gen_dir_mask(dirflag, H, W): float32 [W]"""
    import torch
    d = DIRS[dirflag] if not isinstance(dirflag, str) else dirflag
    if d == "left":
        row = torch.linspace(1, 0, W)
    elif d == "right":
        row = torch.linspace(0, 1, W)
    elif d == "middle":
        row = torch.cat([torch.linspace(0, 1, W // 2), torch.linspace(1, 0, W - W // 2)])
    else:
        row = torch.ones(W)
    assert row.dtype == torch.float32 and row.numel() == W
    return row.numpy().copy()


def ramp_rows(colours, a, b):
    """uint32 [256,3]: (0x00RRGGBB, bits of a_L, bits of b_L)"""
    c = np.asarray(colours, dtype=np.int64).reshape(256, 3)
    rows = np.empty((256, 3), dtype=np.uint32)
    rows[:, 0] = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    rows[:, 1] = np.broadcast_to(np.asarray(a, dtype=f32), (256,)).copy().view(np.uint32)
    rows[:, 2] = np.broadcast_to(np.asarray(b, dtype=f32), (256,)).copy().view(np.uint32)
    return rows


def ramp_parts(rows):
    rows = np.asarray(rows, dtype=np.uint32)
    colours = np.stack([(rows[:, 0] >> 16) & 255, (rows[:, 0] >> 8) & 255, rows[:, 0] & 255], axis=1).astype(np.uint8)
    return colours, rows[:, 1].copy().view(f32), rows[:, 2].copy().view(f32)


def grey_ramp():
    L = np.arange(256)
    return ramp_rows(np.stack([L, L, L], axis=1), 0.0, 1.0)


def random_ramp(seed=3):
    """a ramp no picture would want: random colours, weights on both sides of 0 and beyond 1"""
    rng = np.random.default_rng(seed)
    return ramp_rows(rng.integers(0, 256, (256, 3)), rng.uniform(-0.5, 1.5, 256).astype(f32), rng.uniform(-0.5, 1.5, 256).astype(f32))


def broken_ramp():
    """random_ramp with weights that are not finite at some levels: paint_blend's rule decides (a NaN sum gives 0, +inf 255)"""
    rows = random_ramp(4)
    a, b = rows[:, 1].view(f32), rows[:, 2].view(f32)
    a[0], b[7] = np.nan, np.inf
    a[128], b[128] = np.inf, -np.inf
    a[200] = -np.inf
    b[255] = np.nan
    return rows


def levels_of(x, dirflag):
    """(code, mn, mx, peak, levels uint8 [H,W] or None) of one map x: float32 [H,W]"""
    x = np.asarray(x, dtype=f32)
    H, W = x.shape
    with np.errstate(all="ignore"):
        if not np.isfinite(x).all():
            return 2, f32(0), f32(0), f32(0), None
        mn, mx = x.min(), x.max()
        rng = f32(mx - mn)
        if not np.isfinite(rng):
            return 2, f32(0), f32(0), f32(0), None
        if mx == mn:
            return 1, f32(0), f32(0), f32(0), None
        n = ((x - mn).astype(f32) / rng).astype(f32)
        g = (n * dir_w(dirflag, W)[None, :]).astype(f32)
        peak = g.max()
        if peak == 0:
            return 3, f32(0), f32(0), f32(0), None
        t = (g / peak).astype(f32)
        L = np.rint((t * f32(255)).astype(f32)).astype(np.int64)
    assert L.min() >= 0 and L.max() <= 255
    return 0, mn, mx, peak, L.astype(np.uint8)


def blend_levels(base, L, ramp):
    """base uint8 [H,W,3], L uint8 [H,W] -> uint8 [H,W,3]: paint_blend per channel with the level's colour and weights"""
    colours, a, b = ramp_parts(ramp)
    with np.errstate(all="ignore"):
        ca = (base.astype(f32) * a[L][..., None]).astype(f32)
        kb = (colours[L].astype(f32) * b[L][..., None]).astype(f32)
        r = np.rint((ca + kb).astype(f32))
        s = np.where(r >= 255, f32(255), np.where(r > 0, r, f32(0)))      # a NaN gives 0
    return s.astype(np.uint8)


def paint(heat, maps, ramp, base, out, levels, status):
    """The call on flat host arrays: heat float32 [heat_elems]; maps [M,6] rows; base uint8 [pixels,3] or None; out uint8
    [canvas_pixels,3], levels uint8 [canvas_pixels] or None and status int32 [M,4] are written in place."""
    for m, (H, W, d, h, b, p) in enumerate(np.asarray(maps).tolist()):
        n = H * W
        x = heat[h:h + n].reshape(H, W)
        src = np.zeros((H, W, 3), np.uint8) if base is None else base[b:b + n].reshape(H, W, 3)
        code, mn, mx, peak, L = levels_of(x, d)
        if code:
            out[p:p + n] = src.reshape(n, 3)
            if levels is not None:
                levels[p:p + n] = 0
            status[m] = (code, 0, 0, 0)
            continue
        out[p:p + n] = blend_levels(src, L, ramp).reshape(n, 3)
        if levels is not None:
            levels[p:p + n] = L.reshape(n)
        status[m] = np.array([0] + [int(np.asarray(v, f32).view(np.int32)) for v in (mn, mx, peak)], dtype=np.int64).astype(np.int32)


# ---- the maps ---------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (1, 3), (3, 1), (2, 5), (7, 64), (5, 67), (97, 131)]      # the last: more than one share of 4096 pixels


def fill(rng, H, W, kind, dirflag=0):
    """float32 [H,W] of one kind"""
    x = (rng.standard_normal((H, W)) * 3).astype(f32)
    if kind == "rand":
        return x
    if kind == "huge":          # negative and huge finite values whose range is still finite
        return (rng.uniform(-1.0, 1.0, (H, W)) * 1.5e38).astype(f32)
    if kind == "range":         # finite values, mx - mn is not
        x[0, 0], x[-1, -1] = f32(-3e38), f32(3e38)
        return x
    if kind == "flat":
        return np.full((H, W), 2.5, f32)
    if kind == "nan":
        x[H // 2, W // 3] = np.nan
        return x
    if kind == "inf":
        x[H - 1, W // 2] = np.inf
        return x
    if kind == "peak0":         # the map's maximum sits in a column of weight 0
        w = dir_w(dirflag, W)
        cols = np.flatnonzero(w == 0)
        assert cols.size, (dirflag, W)
        x[H // 2, cols[0]] = x.max() + f32(4)
        return x
    if kind == "onezero":       # n == x: the picture under the grey ramp is the weight itself
        x = np.ones((H, W), f32)
        x[H - 1, 0] = 0
        return x
    if kind == "ties":          # t * 255 = 127.5 at 0.5: to nearest even, 128
        return np.resize(np.array([0, 0.5, 1], f32), H * W).reshape(H, W)
    raise ValueError(kind)


def make_call(seed, specs, with_base=True, gaps=None, ramp=None):
    """specs: per map dict(size=(H, W), dir=0..3, kind=.., heat=key or None, base=key or None); maps with the same heat / base
    key share the extent.  gaps[m]: canvas pixels left out in front of canvas m.  Returns the call as host arrays."""
    rng = np.random.default_rng(seed)
    heat, base, rows = [], [], []
    ends = [0, 0, 0]
    seen = [{}, {}]
    for m, s in enumerate(specs):
        H, W = s["size"]
        n = H * W
        at = []
        for k, key in enumerate((s.get("heat"), s.get("base"))):
            if key is not None and key in seen[k]:
                at.append(seen[k][key])
                continue
            at.append(ends[k])
            if key is not None:
                seen[k][key] = ends[k]
            ends[k] += n
            if k == 0:
                heat.append(fill(rng, H, W, s.get("kind", "rand"), s["dir"]).reshape(-1))
            else:
                base.append(rng.integers(0, 256, (n, 3), dtype=np.uint8))
        ends[2] += gaps[m] if gaps else 0
        rows.append([H, W, s["dir"], at[0], at[1], ends[2]])
        ends[2] += n
    return dict(heat=np.concatenate(heat), maps=np.asarray(rows, dtype=np.int64), ramp=random_ramp() if ramp is None else ramp,
                base=np.concatenate(base) if with_base else None, canvas=ends[2], specs=specs)


def expect(call, with_levels=True, fence=0xA5, tail=0):
    """(out uint8 [canvas + tail, 3], levels uint8 [canvas + tail] or None, status int32 [M,4]) the call must leave behind in
    buffers pre-filled with `fence`"""
    P = call["canvas"] + tail
    out = np.full((P, 3), fence, np.uint8)
    levels = np.full(P, fence, np.uint8) if with_levels else None
    status = np.zeros((len(call["maps"]), 4), np.int32)
    paint(call["heat"], call["maps"], call["ramp"], call["base"], out, levels, status)
    return out, levels, status


def all_sizes_call():
    """every size of SIZES under every direction: 32 maps, the canvases at every p % 4"""
    specs = [dict(size=s, dir=d) for s in SIZES for d in range(4)]
    return make_call(11, specs, gaps=[(3 * m + 1) % 5 for m in range(len(specs))])


def mixed_call():
    """64 maps of mixed sizes and kinds; shared heat extents under different directions; three maps over one base"""
    kinds = ["rand", "huge", "flat", "nan", "inf", "range", "ties", "rand"]
    specs = []
    for m in range(64):
        size = SIZES[(m * 3) % 7] if m != 40 else SIZES[7]
        specs.append(dict(size=size, dir=m % 4, kind=kinds[(m // 4) % 8] if m != 40 else "rand"))      # the large one folds partials
    specs[1].update(size=(7, 64), dir=1, kind="rand", heat="a")
    specs[2].update(size=(7, 64), dir=2, heat="a")
    specs[3].update(size=(7, 64), dir=3, heat="a", base="i")
    specs[5].update(size=(7, 64), dir=0, kind="rand", base="i")
    specs[6].update(size=(7, 64), dir=1, kind="rand", base="i")
    specs[9].update(size=(5, 67), dir=1, kind="peak0")
    specs[10].update(size=(5, 67), dir=2, kind="peak0")
    specs[11].update(size=(2, 5), dir=3, kind="peak0")
    return make_call(12, specs, gaps=[(m * 7) % 4 for m in range(64)])


# ---- heat_paint_plan (csrc/rle_group.h) as Python arithmetic, for tests/native/heat_paint_sanitize.cpp: a case is (maps rows,
# heat_elems, canvas_pixels, base address, out address)
A = dict(base=0x7F0000000000, out=0x7F4000000000)
BLOCK_PIX, PARTS_MAX = 4096, 256


def share_of(n):
    per = (n + PARTS_MAX - 1) // PARTS_MAX
    return (per + BLOCK_PIX - 1) // BLOCK_PIX * BLOCK_PIX


def plan_case(maps, heat=None, canvas=None, base=None, out=None):
    maps = [list(r) for r in maps]
    if heat is None:
        heat = max([r[3] + r[0] * r[1] for r in maps], default=0)
    if canvas is None:
        canvas = max([r[5] + r[0] * r[1] for r in maps], default=0)
    return dict(maps=maps, heat=heat, canvas=canvas, base=A["base"] if base is None else base, out=A["out"] if out is None else out)


def plan_line_of(c):
    return " ".join(str(v) for v in [len(c["maps"]), c["heat"], c["canvas"], c["base"], c["out"]] + [v for r in c["maps"] for v in r])


def plan_want_of(c):
    """None when the plan refuses the case, else (blocks, per map (H, W, dirflag, heat0, base0, pix0, blk0))"""
    M = len(c["maps"])
    I32 = 1 << 31
    if not 1 <= M <= 64 or not 0 <= c["heat"] < (1 << 60) or not 0 <= c["canvas"] < (1 << 60):
        return None
    blocks, rows, ext, b_ext = 0, [], [], []
    for H, W, d, h, b, p in c["maps"]:
        if not (0 < H < I32 and 0 < W < I32 and H * W < I32):
            return None
        n = H * W
        if not 0 <= d <= 3 or not (0 <= h <= c["heat"] and n <= c["heat"] - h) or not 0 <= b < (1 << 60):
            return None
        if not (0 <= p <= c["canvas"] and n <= c["canvas"] - p):
            return None
        if any(not (hi <= p or p + n <= lo) for lo, hi in ext):
            return None
        ext.append((p, p + n))
        b_ext.append((b, b + n))
        rows.append((H, W, d, h, b, p, blocks))
        blocks += (n + share_of(n) - 1) // share_of(n)
    lo, hi = min(e[0] for e in b_ext), max(e[1] for e in b_ext)
    nb, no = 3 * (hi - lo), 3 * c["canvas"]
    first = c["base"] + 3 * lo
    if c["base"] and nb and no and not (first + nb <= c["out"] or c["out"] + no <= first):
        return None
    return blocks, rows


PLAN_SIZES = [(70, 37), (64, 64), (1, 1), (480, 640), (3, 65), (65, 3), (97, 131), (5, 5)]


def plan_packed(sizes, dirs=None, gaps=None):
    rows, at = [], 0
    heat = 0
    for m, (H, W) in enumerate(sizes):
        at += gaps[m] if gaps else 0
        rows.append([H, W, (dirs[m] if dirs else m % 4), heat, heat, at])
        heat += H * W
        at += H * W
    return rows, heat, at


def plan_refusals():
    """(a word of the message, the case): one per rule of the contract"""
    im, heat, total = plan_packed(PLAN_SIZES)
    edit = lambda m, col, v: [[v if (i == m and j == col) else x for j, x in enumerate(r)] for i, r in enumerate(im)]
    return [
        ("0 maps", plan_case([], 0, 0)),
        ("65 maps", plan_case([[2, 2, 0, 0, 0, 4 * m] for m in range(65)])),
        ("heat_elems -1", plan_case(im, heat=-1)),
        ("canvas_pixels -1", plan_case(im, canvas=-1)),
        ("canvas_pixels 1152921504606846976", plan_case(im, canvas=1 << 60)),
        ("bad size 0 x 64", plan_case(edit(1, 0, 0), heat, total)),
        ("bad size 64 x -3", plan_case(edit(1, 1, -3), heat, total)),
        ("bad size 46341 x 46341", plan_case([[46341, 46341, 0, 0, 0, 0]])),
        ("map 2: dirflag 4", plan_case(edit(2, 2, 4), heat, total)),
        ("map 5: dirflag -1", plan_case(edit(5, 2, -1), heat, total)),
        ("map 7: elements", plan_case(im, heat=heat - 1)),
        ("map 3: elements", plan_case(edit(3, 3, -1), heat, total)),
        ("map 4: base pixel -2", plan_case(edit(4, 4, -2), heat, total)),
        ("lie outside", plan_case(im, heat, canvas=total - 1)),
        ("lie outside", plan_case(edit(2, 5, -1), heat, total)),
        ("canvases of images 2 and 3 overlap", plan_case(edit(3, 5, im[2][5]), heat, total)),
        ("out overlaps base", plan_case(im, heat, total, out=A["base"] + 3 * heat - 1)),
        ("out overlaps base", plan_case(im, heat, total, out=A["base"] - 3 * total + 1)),
    ]
