#!/usr/bin/env python3
"""The proposal store (hybridgl_amd/proposals.py, hgl_rle_decode_group_device) measured; writes one JSON object.

  load       the load stage of a group on the device: ops.rle_decode_group for 16 images x 64 proposals of 640 x 640 (blob
             masks, packed counts) against 16 x (ops.rle_decode + sam.mask_boxes) on the same entries, in the same process,
             alternated round by round; HIP events around each, median and spread of --reps rounds
  evaluator  (--evaluator) HybridGLPipeline.run at the benchmark's configuration (ViT-B/16, SAM ViT-H feeding CLIP, GEM
             heat-maps, 64 proposals, groups of 16, image cache off) four ways, alternated: SAM as it is, SAM wrapped in a
             ProposalRecorder, StoredProposals reading the store that recorder wrote, and the same with the group's load
             stage as 16 x (rle_decode + mask_boxes); refs/s each, median and spread of --rounds.  The data are the
             benchmark's 16 seeded synthetic refs, each given an image id, NOT a REFER tree on disk as tools/evaluator_ranks.py
             walks: there is no loader thread, file decode or ground-truth rasterisation in these rates, and the stored legs
             parse their files on the loop's thread at each image's first use (the files stay staged afterwards)

    python tools/proposal_store_bench.py [--reps 30] [--evaluator --steps 64 --rounds 3] [--json profiles/proposal_store_bench.json]

A measurement path that finds no GPU fails.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hybridgl_amd import ops, synth
from hybridgl_amd import proposals as P
from hybridgl_amd import sam as hsam


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "n": len(v)}


def timed_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def load_leg(dev, reps, G=16, N=64, H=640, W=640):
    sets = []
    for g in range(G):
        masks = np.ascontiguousarray(synth.synth_masks(N, H, W, 2000 + g))
        sets.append(ops.rle_pack([hsam.mask_to_rle(m)["counts"] for m in masks], H, W, device=dev))
    sw = max(int(s.shape[1]) for s, _ in sets)
    slots = torch.zeros((G * N, sw), dtype=torch.int32, device=dev)
    for g, (s, _) in enumerate(sets):
        slots[g * N:(g + 1) * N, :s.shape[1]] = s
    table = torch.cat([t for _, t in sets]).contiguous()
    per = [(slots[g * N:(g + 1) * N].contiguous(), table[g * N:(g + 1) * N].contiguous()) for g in range(G)]
    out = torch.empty(G * N * H * W, dtype=torch.uint8, device=dev)
    sizes, counts = [(H, W)] * G, [N] * G

    def grouped():
        return ops.rle_decode_group(slots, table, sizes, counts, out=out)

    def per_image():
        res = []
        for g, (s, t) in enumerate(per):
            m, st = ops.rle_decode(s, t, H, W, out=out[g * N * H * W:(g + 1) * N * H * W])
            res.append((m, hsam.mask_boxes(m), st))
        return res

    a, b = grouped(), per_image()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y[0]) for x, y in zip(a[0], b)) and torch.equal(a[1], torch.cat([y[1] for y in b]))
    for _ in range(5):
        grouped()
        per_image()
    t = {"grouped": [], "per_image": []}
    for _ in range(reps):
        t["grouped"].append(timed_us(grouped))
        t["per_image"].append(timed_us(per_image))
    return {"images": G, "proposals": N, "size": [H, W], "output_MB": round(G * N * H * W / 1e6, 1), "slot_words": sw,
            "grouped_us": spread(t["grouped"]), "per_image_us": spread(t["per_image"]), "launches_grouped": 2, "launches_per_image": 3 * G}


class PerImageStored(P.StoredProposals):
    """the stored generator with the load stage as 16 x (rle_decode + mask_boxes): the comparison leg of the evaluator rate"""

    def _decode(self, slots, table, sizes, counts, aux):
        masks, boxes, status, e = [], [], [], 0
        for (H, W), n in zip(sizes, counts):
            m, st = ops.rle_decode(slots[e:e + n].contiguous(), table[e:e + n].contiguous(), H, W)
            masks.append(m)
            boxes.append(hsam.mask_boxes(m))
            status.append(st)
            e += n
        torch.cat(boxes, out=aux[0])
        torch.cat(status, out=aux[1])
        return masks, aux[0], aux[1]


def evaluator_leg(dev, steps, rounds, group=16, proposals=64):
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.gem import create_gem_model
    from hybridgl_amd.pipeline import HybridGLPipeline, synthetic_ref
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, sam_model_registry
    model = CLIPViTFM("ViT-B/16", seed=0, device=dev)
    gen = SamAutomaticMaskGenerator(sam_model_registry["default"](seed=0, device=dev), points_per_side=8, pred_iou_thresh=-1e30,
                                    stability_score_thresh=0.0, box_nms_thresh=2.0, crop_n_layers=0, min_mask_region_area=800)
    gem = create_gem_model("ViT-B/16", clip=model)
    refs = [dataclasses.replace(synthetic_ref(j, dev, N=proposals, sam_img_size=1024, gem=True, device_blur=True)[0], image_id=5000 + j)
            for j in range(16)]
    with tempfile.TemporaryDirectory() as tmp:
        store = os.path.join(tmp, "store")
        rec = P.ProposalRecorder(gen, store, P.generator_settings(gen, proposal_cap=proposals))
        gens = {"sam": gen, "recorder": rec, "stored": P.StoredProposals(store, dev), "stored_per_image": PerImageStored(store, dev)}
        pipes, rows = {}, {}
        for name, g in gens.items():      # the recorder's warm-up pass writes the store the two stored legs read
            p = HybridGLPipeline(model, mask_generator=g, use_sam_masks=True, gem_model=gem, image_cache=0)
            p.run((refs[i % 16] for i in range(2 * group)), group=group, proposal_cap=proposals, total=2 * group)
            if name == "recorder":
                rec.flush()
            torch.cuda.synchronize()
            rows[name] = p.partial_rows()
            pipes[name] = p
        same = all(np.array_equal(rows["sam"], r) for r in rows.values())
        rate = {k: [] for k in pipes}
        for _ in range(rounds):
            for name, p in pipes.items():
                if name == "recorder":
                    rec.forget()      # every round writes its images again
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = p.run((refs[i % 16] for i in range(steps)), group=group, proposal_cap=proposals, total=steps)
                if name == "recorder":
                    rec.flush()
                torch.cuda.synchronize()
                rate[name].append(n / (time.perf_counter() - t0))
        files = sum(os.path.getsize(os.path.join(store, f)) for f in os.listdir(store))
    return {"steps": steps, "group": group, "rows_identical_across_legs": bool(same), "store_bytes_16_images": files,
            "refs_per_s": {k: spread(v) for k, v in rate.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--evaluator", action="store_true")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "proposal_store_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("proposal_store_bench: no HIP device is visible; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "load": load_leg(dev, args.reps)}
    if args.evaluator:
        out["evaluator"] = evaluator_leg(dev, args.steps, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
