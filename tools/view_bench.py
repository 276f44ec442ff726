#!/usr/bin/env python3
"""Time the view synthesis alone at the headline shape (N = 64 proposals, 640 x 640 -> 224) on cuda:0: hgl_synthesize_views
(unchanged code: the yardstick) alternated with hgl_synthesize_views_prompt at the default prompt and then at every preset.
Device events around warmed loops of ITERS launches (default 200: ~10 ms of device work per window), ROUNDS rounds (default 9);
per variant the median and the range over the rounds, and for the old kernel the spread of its own repeats -- the noise any
difference has to clear.  Both default paths write the same 2 x N x 3 x 224 x 224 x 4 bytes (77 MB).  Prints one JSON line last.
A window holds the host's enqueue of its launches as well: where a kernel is shorter than its Python call, the window measures
the call.  For the kernels alone run it under `rocprofv3 --kernel-trace --stats` with ONLY=hybridgl (the old kernel and the
new one at the default prompt, by name) or ONLY=<preset>."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hybridgl_amd import ops, sam
from hybridgl_amd.synth import imagenet_normalize, synth_image, synth_masks

N, H, W, RES = (int(os.environ.get(k, d)) for k, d in (("N", 64), ("H", 640), ("W", 640), ("RES", 224)))
ITERS, ROUNDS = int(os.environ.get("ITERS", 200)), int(os.environ.get("ROUNDS", 9))


def main():
    assert torch.cuda.is_available(), "view_bench needs the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    img_h = synth_image(H, W, 3)
    img, norm, masks = t(img_h), t(imagenet_normalize(img_h)), t(synth_masks(N, H, W, 4))
    blur = ops.gaussian_blur_u8(img, 15)
    boxes = sam.mask_boxes(masks.view(torch.uint8))
    out = (torch.empty((N, 3, RES, RES), device=dev), torch.empty((N, 3, RES, RES), device=dev))
    variants = {"old": lambda: ops.synthesize_views(img, blur, norm, masks, RES, out=out)}
    for name in [n for n in ops.VIEW_PROMPT_PRESETS if n == "hybridgl" or os.environ.get("ONLY", n) == n]:
        p = ops.view_prompt(name)
        variants[name] = (lambda p=p: ops.synthesize_views_prompt(img, blur, norm, masks, p, boxes=boxes, res=RES, out=out))
    # the same bits at the default prompt, at the size that is timed
    a = [x.clone() for x in variants["old"]()]
    b = variants["hybridgl"]()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / ITERS * 1e3      # microseconds per launch

    for fn in variants.values():      # warm every variant: code objects, allocator
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name in variants:      # old, default, old, black, old, gray, ...: every variant beside a run of the yardstick
            if name != "old":
                times["old"].append(window(variants["old"]))
            times[name].append(window(variants[name]))
    med = lambda v: float(np.median(v))
    write_mb = 2 * N * 3 * RES * RES * 4 / 1e6
    res = {"shape": [N, H, W, RES], "iters": ITERS, "rounds": ROUNDS, "write_MB": round(write_mb, 2), "us": {}}
    for name, v in times.items():
        res["us"][name] = {"median": round(med(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "windows": len(v)}
        print(f"{name:12s} median {med(v):8.2f} us   min {min(v):8.2f}   max {max(v):8.2f}   ({len(v)} windows, {write_mb / med(v) * 1e3:7.1f} GB/s written)")
    old = np.asarray(times["old"])
    res["old_spread_us"] = round(float(old.max() - old.min()), 2)
    res["old_p10_p90_us"] = [round(float(np.percentile(old, 10)), 2), round(float(np.percentile(old, 90)), 2)]
    res["default_minus_old_us"] = round(med(times["hybridgl"]) - med(times["old"]), 2)
    print(f"old kernel's own repeats: spread {res['old_spread_us']} us (p10 {res['old_p10_p90_us'][0]}, p90 {res['old_p10_p90_us'][1]}); "
          f"new default - old = {res['default_minus_old_us']} us")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
