"""Pictures of encoded masks: what the paint kernel (csrc/rle_paint.hip, ops.rle_paint) does not decide.

DEMO_STYLE     the reference demo's overlay (demo.py:212-219) in RGB terms; PURE_STYLE: the same in red
palette(n)     a fixed table of distinct colours, no RNG
overlay        entries of one image's set painted over the image, on the device
overlay_group  the same for up to 64 images of their own sizes in one call
save_png       Pillow, on the host: the one place pixels cross the bus

The overlay rule is UNPINNED, like the blur: the reference blends with cv2.addWeighted and cv2 is not installed here, so no test
compares against it.  What is pinned is the rule the kernel states (include/hybridgl.h): sat_u8(rint(f32(pixel) * a + f32(colour)
* b)) with both products and the sum rounded to fp32.  Only the a = 1 style claims to match addWeighted: pixel * 1 is exact, so
the unfused form used here and a fused multiply-add agree bit for bit, and DEMO_STYLE is such a style.

demo.py:212-219 swaps the image to BGR, turns the mask into a BGR image of 255s, zeroes its channels 2 and 1 through uint8
wrap-around ((255 - 255) * 255 = 0), adds with addWeighted(img, 1, seg, 0.7, 0) and writes BGR.  Net effect on the mask: the
image's blue channel gets + 178.5, rounded half to even and saturated; red and green stay."""
import torch

from . import ops

DEMO_STYLE = dict(fill=(0, 0, 255), a=1.0, b=0.7, outline=None)
PURE_STYLE = dict(fill=(255, 0, 0), a=1.0, b=0.7, outline=None)      # the same rule in red: the pure CLIP winner beside the final one


def palette(n):
    """n distinct (R, G, B) colours, none of them black: the bit-reversal colour cube (the PASCAL VOC label colours from label
    1 on), distinct for n <= 255 and repeating after that."""
    out = []
    for i in range(int(n)):
        c, r, g, b = i % 255 + 1, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        out.append((r, g, b))
    return out


def proposal_styles(n, a=0.5, b=0.5):
    """the style rows of `n` proposals in palette colours, filled half and half and outlined in the colour itself"""
    import numpy as np
    return np.stack([ops.rle_paint_style(fill=c, a=a, b=b, outline=c) for c in palette(n)]) if n else np.zeros((0, 4), np.uint32)


def set_from_rles(rles, device=None):
    """COCO RLE dicts ({"size": [H, W], "counts": the compressed string}) of ONE size -> (slots, table) on the device, read from
    the strings on the device (ops.rle_from_strings): one pinned buffer, one copy"""
    S = len(rles)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    buf, _, n_counts = ops.rle_strings_pack([r["counts"] for r in rles])
    sw = max(int(n_counts.max()) if S else 0, 1)
    dev = buf.to(device, non_blocking=True)
    slots, table, _ = ops.rle_from_strings(dev[8 * (S + 1):], dev[:8 * (S + 1)].view(torch.int64), S, sw)
    return slots, table


def _image_u8(image, device):
    """uint8 [H,W,3] on the device out of an array, a tensor or a path"""
    if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
        import numpy as np
        from PIL import Image
        image = np.array(Image.open(image).convert("RGB"))
    if not torch.is_tensor(image):
        from .loader import pin_upload
        image = pin_upload(image, device)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError(f"image: expected uint8 [H, W, 3], got {tuple(image.shape)} {image.dtype}")
    return image.to(device).contiguous()


def overlay_group(images, slots, table, counts, order=None, order_counts=None, style=None, labels=False, out=None):
    """Entries of an encoded set painted over up to 64 images in ONE ops.rle_paint call.  images: uint8 [H,W,3] device tensors
    (None for a black canvas needs sizes: pass (H, W) in its place); the set's counts[g] consecutive entries belong to image g.
    order / order_counts: the paint list (default every entry, in stored order); style: one row, or one per list position
    (default DEMO_STYLE).  Returns (pictures: uint8 [H,W,3] views, labels or None, status) as ops.rle_paint does."""
    sizes = [tuple(int(v) for v in (im if isinstance(im, tuple) else im.shape[:2])) for im in images]
    black = [isinstance(im, tuple) for im in images]
    if any(black) and not all(black):
        images = [torch.zeros(*s, 3, dtype=torch.uint8, device=slots.device) if k else im for im, s, k in zip(images, sizes, black)]
    if order is None:
        import numpy as np
        order = np.concatenate([np.arange(int(n), dtype=np.int32) for n in counts]) if len(counts) else np.zeros(0, np.int32)
        order_counts = [int(n) for n in counts]
    if style is None:
        style = ops.rle_paint_style(**DEMO_STYLE)
    return ops.rle_paint(slots, table, sizes, counts, order, order_counts, style, base=None if all(black) else list(images),
                         out=out, labels=labels)


def overlay(image, masks, order=None, style=None, labels=False):
    """Entries painted over ONE image: masks is a list of COCO RLE dicts or a (slots, table) pair on the device; image an uint8
    [H,W,3] array, tensor or path.  order: the entries to paint, in order (a sequence or an int32 device tensor; default all);
    style: one row or one per position (default DEMO_STYLE).  Returns the picture, uint8 [H,W,3] on the device -- with
    labels=True (picture, labels [H,W] int32, status)."""
    dev = masks[0].device if isinstance(masks, tuple) else torch.device("cuda", torch.cuda.current_device())
    image = _image_u8(image, dev)
    if not isinstance(masks, tuple):
        for r in masks:
            if tuple(r["size"]) != tuple(image.shape[:2]):
                raise ValueError(f"overlay: a mask of size {list(r['size'])} over an image of {list(image.shape[:2])}")
        masks = set_from_rles(masks, dev)
    slots, table = masks
    S = int(slots.shape[0])
    K = S if order is None else (int(order.numel()) if torch.is_tensor(order) else len(order))
    pics, labs, status = overlay_group([image], slots, table, [S], order, None if order is None else [K], style, labels)
    return (pics[0], labs[0], status) if labels else pics[0]


# ---- heat-maps: the scorer's guided map as colours (csrc/rle_paint.hip: hgl_heat_paint_device, ops.heat_paint) --------------------
HEAT_STOPS = [(0, (0, 0, 255)), (85, (0, 255, 255)), (170, (255, 255, 0)), (255, (255, 0, 0))]      # (level, colour): blue, cyan, yellow, red
HEAT_ALPHA = 0.7      # the weight of the colour at level 255; 0 at level 0: where the map is cold the image shows through
_ramps = {}


def ramp(name):
    """A named ramp of ops.heat_paint, uint32 [256,3] on the host.  "heat": piecewise linear through HEAT_STOPS, the colour's
    weight b rising from 0 at level 0 to HEAT_ALPHA at level 255 and a = 1 - b; "grey": level L is the grey (L, L, L), opaque."""
    import numpy as np
    if name not in _ramps:
        L = np.arange(256)
        if name == "heat":
            at = [s[0] for s in HEAT_STOPS]
            colours = np.stack([np.rint(np.interp(L, at, [s[1][c] for s in HEAT_STOPS])) for c in range(3)], axis=1)
            b = (HEAT_ALPHA * L / 255.0).astype(np.float32)
            _ramps[name] = ops.heat_ramp(colours, np.float32(1) - b, b)
        elif name == "grey":
            _ramps[name] = ops.heat_ramp(np.stack([L, L, L], axis=1), 0.0, 1.0)
        else:
            raise ValueError(f"ramp: {name!r} ('heat' or 'grey')")
    return _ramps[name]


_named_ramp = ramp      # the functions below take a parameter of this name

def heatmap_group(images, heats, dirflags, ramp="heat", image_of=None, levels=False, out=None):
    """Up to 64 heat-maps painted over their images in ONE ops.heat_paint call, nothing read back.  heats: float32 [H,W] device
    tensors -- the raw maps the scoring tail is given; dirflags: "none" / "left" / "right" / "middle" per map; images: uint8
    [H,W,3] device tensors, or None for black canvases; image_of[m]: the image under map m (default m: one image per map) --
    several sentences over one image share it.  ramp: a name of ramp(), or [256,3] rows of ops.heat_ramp.  The same tensor
    object given twice in heats is uploaded once and read under both directions.
    Returns (pictures: uint8 [H,W,3] views, levels: uint8 [H,W] views or None, status [M,4] int32) as ops.heat_paint does."""
    M = len(heats)
    if len(dirflags) != M or (image_of is not None and len(image_of) != M):
        raise ValueError(f"heatmap_group: {M} maps, {len(dirflags)} dirflags")
    image_of = list(range(M)) if image_of is None else [int(i) for i in image_of]
    sizes = [tuple(int(v) for v in h.shape) for h in heats]
    if images is not None:
        for m, i in enumerate(image_of):
            if not 0 <= i < len(images) or tuple(images[i].shape) != (*sizes[m], 3):
                raise ValueError(f"heatmap_group: map {m} of size {sizes[m]} over image {i}")
    shared_heat = [id(h) for h in heats]
    maps, _, _, _ = ops.heat_paint_layout(sizes, dirflags, shared_heat=shared_heat, shared_base=image_of)
    first = lambda keys: [m for m, k in enumerate(keys) if k not in keys[:m]]      # the extents in the layout's order
    flat = lambda parts: parts[0].reshape(-1) if len(parts) == 1 else torch.cat([p.reshape(-1) for p in parts])
    heat = flat([heats[m].to(torch.float32).contiguous() for m in first(shared_heat)])
    base = None if images is None else flat([images[image_of[m]].contiguous() for m in first(image_of)])
    rows = _named_ramp(ramp) if isinstance(ramp, str) else ramp
    return ops.heat_paint(heat, maps, rows, base=base, out=out, levels=levels)


def heatmap(image, heat, dirflag="none", ramp="heat"):
    """ONE heat-map over its image: uint8 [H,W,3] on the device.  image: an uint8 [H,W,3] array, tensor or path, or None for a
    black canvas; heat: float32 [H,W] on the device."""
    image = None if image is None else [_image_u8(image, heat.device)]
    return heatmap_group(image, [heat], [dirflag], ramp=ramp)[0][0]


def save_png(path, tensor):
    """uint8 [H,W,3] (device or host) -> a PNG file, through Pillow on the host"""
    from PIL import Image
    t = tensor.detach()
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"save_png: expected uint8 [H, W, 3], got {tuple(t.shape)} {t.dtype}")
    Image.fromarray(t.cpu().numpy(), "RGB").save(path, format="PNG")
