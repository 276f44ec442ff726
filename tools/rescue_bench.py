"""What on_overflow="rescue" costs when nothing overflows, and what one rescue costs.

Builds the headline pipeline the way bench.py does (ViT-B/16 + GEM + SAM ViT-H with the benchmark's open filters, 16 images
per group, 64 proposals, the same resident synthetic refs) twice over the same models, once per mode, prepares both, and
times run() over --steps refs: "raise" and "rescue" alternately, --repeat runs each; then the rescue pipeline with ONE
injected overflow (a counted split-fp16 GEMM enqueued by the loader half way through), twice -- the first rescue of a
process allocates the f32 workspaces (device mallocs, bytes the caching allocator reserves, bytes of ops.workspace arenas: all
reported per run), the second does not.  One JSON document on stdout and in --out, which holds nothing else.

    python tools/rescue_bench.py --out profiles/overflow_rescue_ab.json      (the default path against the parent commit is
    bench.py's own measurement and lies in profiles/overflow_rescue_default_path.json)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--group", type=int, default=16)
    ap.add_argument("--masks", type=int, default=64)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CLIP_GEOM
    from hybridgl_amd import ops
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.gem import create_gem_model
    from hybridgl_amd.pipeline import HybridGLPipeline, synthetic_ref
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, sam_model_registry

    assert torch.cuda.is_available(), "rescue_bench.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    geom = CLIP_GEOM["ViT-B/16"]
    model = CLIPViTFM("ViT-B/16", seed=0, device=dev)
    sam = sam_model_registry["default"](seed=0, device=dev)
    gen = SamAutomaticMaskGenerator(sam, points_per_side=8, pred_iou_thresh=-1e30, stability_score_thresh=0.0, box_nms_thresh=2.0,
                                    crop_n_layers=0, crop_n_points_downscale_factor=1, min_mask_region_area=800)
    gem_model = create_gem_model("ViT-B/16", clip=model)
    refs = [synthetic_ref(j, dev, N=args.masks, sam_img_size=1024, gem=True, device_blur=True)[0] for j in range(args.pool)]
    g_timed = HybridGLPipeline.balanced_group(args.steps, args.group)
    pipes = {}
    for mode in ("raise", "rescue"):
        pipes[mode] = HybridGLPipeline(model, fusion_mode="G2L", masking_block=geom["masking_block"], mask_generator=gen,
                                       use_sam_masks=True, gem_model=gem_model, on_overflow=mode)
        pipes[mode].prepare(group=g_timed, H=640, W=640, proposals=args.masks, n_sent=3,
                            tail=HybridGLPipeline.balanced_group(max(args.warmup, 1), args.group))

    rng = np.random.default_rng(3)
    a2 = rng.standard_normal((256, 128)).astype(np.float32)
    a2[3, 5] = 1.0e6
    a2 = torch.from_numpy(a2).to(dev)
    w = torch.from_numpy((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32)).to(dev)
    ops.gemm_f16x3(w[:64].contiguous().repeat(4, 1), w)      # (registers w and sizes the GEMM's workspace outside any timing)
    torch.cuda.synchronize()
    ops.split_overflow_count()

    def loader(k, inject_at=None):
        for i in range(k):
            if i == inject_at:
                ops.gemm_f16x3(a2, w)
            yield refs[i % len(refs)]

    def timed(mode, k, inject_at=None):
        p = pipes[mode]
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
        r0, a0, n0 = torch.cuda.memory_reserved(dev), sum(b.numel() for b in ops._ws_cache.values()), len(ops._ws_cache)
        ev = dict(p.rescue_stats, positions=list(p.rescue_stats["positions"]))
        t0 = time.perf_counter()
        n = p.run(loader(k, inject_at), group=args.group, proposal_cap=args.masks, total=k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert n == k, (n, k)
        st = p.rescue_stats
        return {"ms": round(dt * 1e3, 2), "device_mallocs": torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - m0,
                "reserved_bytes_grown": torch.cuda.memory_reserved(dev) - r0,
                "workspace_arenas_new": len(ops._ws_cache) - n0,
                "workspace_arena_bytes_grown": sum(b.numel() for b in ops._ws_cache.values()) - a0,
                "events": st["events"] - ev["events"], "groups_rerun": st["groups"] - ev["groups"], "refs_rerun": st["refs"] - ev["refs"]}

    for mode in pipes:
        timed(mode, args.warmup)
    runs = {"raise": [], "rescue": []}
    for _ in range(args.repeat):
        for mode in ("raise", "rescue"):
            runs[mode].append(timed(mode, args.steps))
    injected = [timed("rescue", args.steps, inject_at=args.steps // 2) for _ in range(2)]
    after = timed("rescue", args.steps)
    assert ops.split_overflow_count() == 0
    med = {m: statistics.median(r["ms"] for r in runs[m]) for m in runs}
    spread = {m: round(max(r["ms"] for r in runs[m]) - min(r["ms"] for r in runs[m]), 2) for m in runs}
    doc = {"what": "HybridGLPipeline.run on the headline workload, on_overflow raise vs rescue (tools/rescue_bench.py)",
           "device": torch.cuda.get_device_name(dev), "precision": ops.default_precision(), "steps": args.steps, "group": g_timed,
           "proposals": args.masks, "runs": runs, "median_ms": med, "max_minus_min_ms": spread,
           "rescue_on_nothing_overflowing": {"extra_ms": round(med["rescue"] - med["raise"], 2),
                                             "extra_percent": round(100.0 * (med["rescue"] / med["raise"] - 1.0), 2)},
           "one_injected_event": {"first_of_the_process": injected[0], "second": injected[1], "clean_run_after": after,
                                  "cost_ms_first": round(injected[0]["ms"] - med["rescue"], 2),
                                  "cost_ms_second": round(injected[1]["ms"] - med["rescue"], 2)}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
