"""A/B of the three precision modes on the ENCODER work of one headline group (not the prepare()d pipeline: no proposal
stage, text encoder, GEM or scoring tail): CLIP ViT-B/16 hybrid forward over 16 refs x 64 proposals (G2L: 1024 local + 1024
global views) and the SAM ViT-H image encoder on sixteen synthetic 1024 x 1024 images (the size a 640 x 640 image is resized
to).  Per mode: encoder images per second (timed with the per-launch HIP-event profiling on), GEMM / attention ms per ref
from those events (GEMM = the fp32, split-fp16 and few-tile classes; the skinny GEMMs count as "other" and are left out),
and the largest feature difference against f32.

    python tools/precision_ab.py [--refs 16] [--proposals 64] [--iters 3] [--out profiles/precision_ab.json]

bench.py labels every mode other than f16x3 as "f32", so this tool is the yardstick of the f16 mode."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hybridgl_amd import _lib, ops, weights  # noqa: E402

GEMM_CLASSES = (0, 3, 4, 5)   # fp32 MFMA, split-fp16 register-staged, ping-pong, few-tile launches
ATTN_CLASS = 1


def prof_ms(lib, classes):
    tot = 0.0
    for c in classes:
        n, ms, fl, by = C.c_longlong(0), C.c_double(0), C.c_double(0), C.c_double(0)
        lib.hgl_prof_read(c, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
        tot += ms.value
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=16)
    ap.add_argument("--proposals", type=int, default=64)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    from hybridgl_amd import sam as hsam
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.synth import synth_image
    from oracle.cases import views_for_case

    R, N = a.refs, a.proposals
    loc, glo, masks = views_for_case(R * N, 224, 160, 200)
    x = (torch.from_numpy(loc).to(dev), torch.from_numpy(glo).to(dev), torch.from_numpy(masks).to(dev))
    imgs = [torch.from_numpy(synth_image(1024, 1024, 10 + i)).to(dev) for i in range(R)]
    csd = weights.clip_state_dict("ViT-B/16", 0)
    ssd = weights.sam_state_dict("vit_h", 0)
    res, feats = {}, {}
    for mode in ("f32", "f16x3", "f16"):
        clip = CLIPViTFM("ViT-B/16", state_dict=csd, device=dev, precision=mode)
        sam = hsam.Sam(ssd, weights.SAM_CONFIGS["vit_h"], dev, precision=mode)
        ops.split_overflow_count()

        def step():
            y = clip(*x, masking_block=9, fusion_mode="G2L")
            e = [sam.encode(im) for im in imgs]
            return y, e

        y, e = step()     # warm-up (and the features compared)
        torch.cuda.synchronize()
        feats[mode] = (y.double().cpu(), torch.stack(e).double().cpu())
        lib.hgl_prof_enable(1)
        prof_ms(lib, GEMM_CLASSES + (ATTN_CLASS, 2))
        t0 = time.perf_counter()
        for _ in range(a.iters):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.iters
        gemm = prof_ms(lib, GEMM_CLASSES) / a.iters
        attn = prof_ms(lib, (ATTN_CLASS,)) / a.iters
        lib.hgl_prof_enable(0)
        res[mode] = {"img_per_s": R / dt, "seconds_per_group": dt, "gemm_ms_per_ref": gemm / R, "attn_ms_per_ref": attn / R,
                     "overflow": ops.split_overflow_count()}
        del clip, sam
        torch.cuda.empty_cache()
    for mode in res:
        yc, ys = feats[mode]
        rc, rs = feats["f32"]
        res[mode]["clip_max_rel_diff_vs_f32"] = float((yc - rc).abs().max() / rc.abs().max())
        res[mode]["sam_rms_rel_diff_vs_f32"] = float((ys - rs).pow(2).mean().sqrt() / rs.pow(2).mean().sqrt())
        print(json.dumps({"mode": mode, **res[mode]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"refs": R, "proposals": N, "iters": a.iters, "modes": res}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
