#!/usr/bin/env python3
"""The device RLE encoder (csrc/rle.hip) measured three ways; prints one JSON object.

  kernel     ops.rle_encode alone (HIP events, median of --reps after warm-up) for 64 proposal-shaped masks of 640 x 640 and for
             6 of the 64 selected by a device index tensor (the evaluator's case: two winners of three sentences), as TB/s of
             ONE streaming read of the selected mask bytes; beside it hgl_iou -- a pure streaming read of the project over the
             same number of bytes -- timed the same way in the same process
  generator  the record tail of SamAutomaticMaskGenerator.generate() in coco_rle mode at 64 proposals of 640 x 640, both paths
             in this process: the byte copy + host codec (the code before the device encoder) and sam.masks_to_rle (host wall
             time from the device tensor to the list of records, median of --reps)
  evaluator  (--evaluator) HybridGLPipeline.run at the benchmark's configuration (ViT-B/16, SAM ViT-H feeding CLIP, GEM
             heat-maps, 64 proposals, groups of 16) with record_predictions off and on, alternating, refs/s each

    python tools/rle_bench.py [--reps 30] [--evaluator --steps 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hybridgl_amd import ops, synth
from hybridgl_amd import sam as hsam


def device_us(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def host_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kernel_leg(masks, reps):
    N, H, W = masks.shape
    dev = masks.device
    sw = ops.rle_slot_words(H, W)
    rec = {}
    for name, sel in (("all_64", None), ("6_of_64", torch.tensor([5, 17, 17, 40, 63, 2], dtype=torch.int64, device=dev))):
        S = N if sel is None else int(sel.numel())
        flat = torch.empty(S * (4 + sw), dtype=torch.int32, device=dev)
        us = device_us(lambda: ops.rle_encode(masks, sel, sw, out=flat), reps)
        nbytes = S * H * W
        # the yardstick: hgl_iou streams two byte arrays; half of each of `nbytes` bytes in total
        a, b = masks.reshape(-1)[:nbytes // 2], masks.reshape(-1)[nbytes // 2:nbytes // 2 * 2]
        us_read = device_us(lambda: ops.iou_counts(a, b), reps)
        rec[name] = {"entries": S, "selected_mask_bytes": nbytes, "rle_encode_us": round(us, 1),
                     "TBps_of_one_read": round(nbytes / us / 1e6, 3), "hgl_iou_same_bytes_us": round(us_read, 1),
                     "hgl_iou_TBps": round(nbytes / us_read / 1e6, 3), "time_over_streaming_read": round(us / us_read, 2)}
    return rec


def generator_leg(masks, reps):
    """generate()'s record tail for the RLE modes: (device masks) -> (coco_rle segmentations, areas)"""
    def before():
        host = masks.bool().cpu().numpy()
        return [hsam.coco_encode_rle(hsam.mask_to_rle(m)) for m in host], [int(m.sum()) for m in host]

    def now():
        rles, areas = hsam._masks_to_rle(masks)
        return [hsam.coco_encode_rle(r) for r in rles], areas

    assert before() == now()
    b, n = host_ms(before, reps), host_ms(now, reps)
    return {"proposals": int(masks.shape[0]), "byte_copy_and_host_codec_ms": round(b, 2), "device_encoder_ms": round(n, 2),
            "factor": round(b / n, 2)}


def evaluator_leg(dev, steps, group=16, proposals=64, rounds=3):
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.gem import create_gem_model
    from hybridgl_amd.pipeline import HybridGLPipeline, synthetic_ref
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, sam_model_registry
    model = CLIPViTFM("ViT-B/16", seed=0, device=dev)
    gen = SamAutomaticMaskGenerator(sam_model_registry["default"](seed=0, device=dev), points_per_side=8, pred_iou_thresh=-1e30,
                                    stability_score_thresh=0.0, box_nms_thresh=2.0, crop_n_layers=0, min_mask_region_area=800)
    gem = create_gem_model("ViT-B/16", clip=model)
    refs = [synthetic_ref(j, dev, N=proposals, sam_img_size=1024, gem=True, device_blur=True)[0] for j in range(16)]
    pipes = {}
    for name, on in (("off", False), ("on", True)):
        p = HybridGLPipeline(model, mask_generator=gen, use_sam_masks=True, gem_model=gem, record_predictions=on)
        p.prepare(group=HybridGLPipeline.balanced_group(steps, group), H=640, W=640, proposals=proposals, n_sent=3)
        p.run((refs[i % 16] for i in range(2 * group)), group=group, proposal_cap=proposals, total=2 * group)
        pipes[name] = p
    torch.cuda.synchronize()
    rate = {"off": [], "on": []}
    mallocs = {}
    for _ in range(rounds):
        for name, p in pipes.items():
            m0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = p.run((refs[i % 16] for i in range(steps)), group=group, proposal_cap=proposals, total=steps)
            torch.cuda.synchronize()
            rate[name].append(n / (time.perf_counter() - t0))
            mallocs[name] = torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - m0
    n_pred = len(pipes["on"].predictions())
    runs = sum(len(r["pure"]) + len(r["final"]) for r in pipes["on"].predictions())
    off, on = statistics.median(rate["off"]), statistics.median(rate["on"])
    return {"steps": steps, "group": group, "refs_per_s_off": round(off, 2), "refs_per_s_on": round(on, 2),
            "all_rates_off": [round(v, 2) for v in rate["off"]], "all_rates_on": [round(v, 2) for v in rate["on"]],
            "cost_percent": round(100.0 * (off - on) / off, 2), "device_mallocs_last_round": mallocs,
            "sentences_recorded": n_pred, "host_bytes_of_counts": 4 * runs, "staging_buffers": len(pipes["on"]._pred_free)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--evaluator", action="store_true")
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rle_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    masks = torch.from_numpy(np.ascontiguousarray(synth.synth_masks(64, 640, 640, 2000))).to(dev).view(torch.uint8)
    out = {"kernel": kernel_leg(masks, args.reps), "generator": generator_leg(masks, args.reps)}
    if args.evaluator:
        out["evaluator"] = evaluator_leg(dev, args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
