#!/usr/bin/env python3
"""Benchmark of the HybridGL hot path on MI355X (contract: see the task statement / DESIGN.md).

    python bench.py --gpus N --steps K --warmup W        (N>1: launched by torch.distributed.run)
    python bench.py --gpus 1 --full                      (+ every secondary measurement of the line)
    python bench.py --gpus 1 --dump-outputs DIR          (+ the last timed step's outputs as DIR/<name>.npy)

A plain run sets up, warms up, times the K steps and prints the result line.  --full adds the legs that take runs of their
own: the roofline group with per-kernel HIP events, the live rocprofv3 counter passes, the secondary configurations under
`also`, the evaluator fed from disk, the RCCL self-check and the CPU baseline.

One step = one dataset item ("ref") of BASELINE.json configs[1]: a 640x640 image with 64 mask
proposals and 3 text queries, G2L fusion, CLIP ViT-B/16 -- SAM ViT-H proposal stage, view synthesis, CLIP hybrid
encoder, text encoder (9 strings + 3 GEM prompts), the GEM heat-map stage (ViT-B/16 at 448x448) and the
per-sentence scoring tail with IoU.  All inputs are synthetic
(hybridgl_amd/synth.py), weights are seeded random (no checkpoints offline), and every input is
resident in HBM before the timed region.  Refs are sharded over ranks with no data-path
collective (weak scaling); the per-sentence metric rows are all-gathered once at the end (hybridgl_amd/dist.py).

`--gpus N` without a launcher (WORLD_SIZE unset) starts N ranks itself, before this process touches the GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

# dense fp32 matrix peak and HBM peak from /opt/skills/guides/MI355X_MICROARCH.md
PEAK_FP32_MFMA_TFLOPS = 157.3
PEAK_FP16_MFMA_TFLOPS = 2500.0   # dense; AMD's 5 PF headline includes 2:1 sparsity
PEAK_HBM_GBS = 8000.0
PEAK_HBM_TBPS = PEAK_HBM_GBS / 1000.0
TAIL_GROUP_REFS = 16     # refs per launch of the group-wide scoring tail (hgl_score_group) in the counter pass: its group of 16


# CLIP geometries: ViT-B/16 is the reference's configuration (Hybridgl_main.py:37,47); ViT-L/14 is the extension named by
# BASELINE.json (no oracle in the reference: model/backbone.py:16-21 defines neither last_layer nor heads for it;
# SURVEY.md note 2: last_layer = layers - 2, masking_block = layers - 3)
CLIP_GEOM = {
    "ViT-B/16": dict(D=768, layers=12, S=197, patch_k=768, embed=512, masking_block=9, last_layer=10, text_D=512, gem_S=785),
    "ViT-L/14": dict(D=1024, layers=24, S=257, patch_k=588, embed=768, masking_block=21, last_layer=22, text_D=768, gem_S=1025),
}


def gem_flops_per_image(S=785, D=768, layers=12, gem_blocks=6, patch_k=768, embed=512):
    """GEM ViT-B/16 at 448x448, computed ONCE per image: per block 2*S*D*12D of GEMMs + 4*S^2*D of attention;
    a GEM block adds 3 sets x 2 self-self attentions (4*S^2*D each) and one more out-projection; the MLP and the
    original attention of the last block are dead."""
    gemm = 2.0 * S * D * 12 * D
    attn = 4.0 * S * S * D
    plain = layers * (gemm + attn) - (2.0 * S * D * 8 * D + 2.0 * S * D * D + attn)
    ss = gem_blocks * (6 * attn + 2.0 * S * D * D)
    return plain + ss + 2.0 * (S - 1) * patch_k * D + 2.0 * S * D * embed


def algorithmic_flops_per_ref(N=64, n_strings=9, sam=True, gem=False, clip_name="ViT-B/16", text_S=77):
    """SURVEY.md 8d, minimal variant (dead work removed), G2L: the two streams run through the blocks below the masking
    block and the two-stream blocks (ViT-B/16: 22 N block evaluations of 2.908 GFLOP; ViT-L/14: 46 N of 6.738 GFLOP); the
    returning block runs on one stream and only as far as its CLS row needs (0.70 instead of 2.908 GFLOP per mask).  SAM ViT-H encoder 5.961 TFLOP + decoder 3.62 GFLOP
    x 64 prompts; + the GEM heat-map stage when it runs here."""
    g = CLIP_GEOM[clip_name]
    S, D = g["S"], g["D"]
    blk = 2.0 * S * D * 12 * D + 4.0 * S * S * D          # ViT-B/16: 2.908e9 (qkv .697, proj .232, mlp 1.859, attn .119)
    patch = 2.0 * (S - 1) * g["patch_k"] * D               # ViT-B/16: 0.231e9
    # full blocks: both streams below the returning block (2 * (last_layer + 1) evaluations per mask); the returning block
    # itself feeds only its CLS row to the head: ln_1 + qkv on every token, everything after on one row per sequence
    n_full = 2 * g["last_layer"] + 2
    ret = 2.0 * S * D * 3 * D + 4.0 * S * D + 2.0 * D * 9 * D
    clip = 2 * N * patch + n_full * N * blk + N * ret
    tD = g["text_D"]
    # text_S: positions the text encoder computes (77 = the full context; the pipeline computes the EOT prefix only)
    text = (12 * (2.0 * text_S * tD * 12 * tD + 4.0 * text_S * text_S * tD) + 2.0 * tD * g["embed"]) * (n_strings + (3 if gem else 0))
    gem_fl = gem_flops_per_image(g["gem_S"], D, g["layers"], 6, g["patch_k"], g["embed"]) if gem else 0.0
    return clip + text + ((5.961e12 + 64 * 3.62e9) if sam else 0.0) + gem_fl


def roofline(precision, nprof, g, x, a, traffic, whole_tflops, xg=(0, 0.0, 0.0), few=(0, 0.0, 0.0)):
    """roofline object for the kernel that dominates the step (by summed launch time)."""
    g_n, g_ms, g_fl = g
    x_n, x_ms, x_fl = x
    a_n, a_ms, a_fl = a
    xg_n, xg_ms, xg_fl = xg
    tf = lambda fl, ms: fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    members = {
        "gemm_f16x3_kernel": {"achieved": tf(x_fl, x_ms), "launches_per_step": x_n / nprof, "ms_per_step": x_ms / nprof},
        "gemm_x3p_kernel": {"achieved": tf(xg_fl, xg_ms), "launches_per_step": xg_n / nprof, "ms_per_step": xg_ms / nprof},
    }
    if max(x_ms, xg_ms) > g_ms:
        name = "gemm_f16x3_kernel (register-staged 128x128 tiling)"
        if xg_ms > x_ms:   # the LDS-DMA family dominates: report it, keep the other under other_kernels
            name = "gemm_x3p_kernel (256x256 LDS-DMA ping-pong tiling, persistent)"
            (x_n, x_ms, x_fl), (xg_n, xg_ms, xg_fl) = (xg_n, xg_ms, xg_fl), (x_n, x_ms, x_fl)
        ach = tf(x_fl, x_ms)
        main = {"bound": "mfma", "kernel": name + ": fp32 operands split in fp16 hi+lo; 3 x v_mfma_f32_16x16x32_f16 "
                "per 32-deep product step, fp32 accumulate",
                "f16x3_gemm_family": {"achieved": tf(x_fl + xg_fl, x_ms + xg_ms), "ms_per_step": (x_ms + xg_ms) / nprof,
                                      "launches_per_step": (x_n + xg_n) / nprof,
                                      "other_member": {"achieved": tf(xg_fl, xg_ms), "ms_per_step": xg_ms / nprof,
                                                       "launches_per_step": xg_n / nprof}},
                "achieved": ach, "peak": PEAK_FP16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP16_MFMA_TFLOPS,
                "note": "achieved counts ALGORITHMIC flops (2MNK); the kernel issues 3x that on the fp16 matrix cores",
                "issued_mfma_tflops": 3 * ach, "frac_issued": 3 * ach / PEAK_FP16_MFMA_TFLOPS,
                "x_fp32_matrix_peak": ach / PEAK_FP32_MFMA_TFLOPS,
                # what the bare v_mfma_f32_16x16x32_f16 stream sustains with every CU busy: 2420 TF/s on all-zero operands, 1920
                # on operands whose bits toggle (the power limit; tools/micro/mfma_rate.hip, not measured in this run)
                "frac_issued_of_sustained_mfma_rate": 3 * ach / 1920.0,
                "sustained_mfma_rate_source": "profiles/r03_mfma_rate_microbench.txt (1920 TF/s issued, random operands)",
                "launches_per_step": x_n / nprof, "avg_launch_ms": x_ms / max(x_n, 1), "ms_per_step": x_ms / nprof,
                "algorithmic_flops_per_step": x_fl / nprof}
    else:
        ach = tf(g_fl, g_ms)
        main = {"bound": "mfma", "kernel": "gemm_f32_kernel (v_mfma_f32_32x32x2_f32)", "achieved": ach,
                "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP32_MFMA_TFLOPS,
                "launches_per_step": g_n / nprof, "avg_launch_ms": g_ms / max(g_n, 1), "ms_per_step": g_ms / nprof,
                "algorithmic_flops_per_step": g_fl / nprof}
    main["traffic"] = traffic
    main["other_kernels"] = {
        "gemm_f32_kernel": {"achieved": tf(g_fl, g_ms), "launches_per_step": g_n / nprof, "ms_per_step": g_ms / nprof},
        "gemm_f16x3_kernel": members["gemm_f16x3_kernel"],
        "gemm_x3p_kernel": members["gemm_x3p_kernel"],
        "attention_kernels": {"achieved": tf(a_fl, a_ms), "launches_per_step": a_n / nprof, "ms_per_step": a_ms / nprof},
    }
    main["other_kernels"]["f16x3_gemm_few_tile_launches"] = {
        "achieved": tf(few[2], few[1]), "launches_per_step": few[0] / nprof, "ms_per_step": few[1] / nprof,
        "note": "launches of the f16x3 kernels with < 256 output tiles (GEM heat-map tower at 785 rows, text encoder at 924 "
                "rows): latency-bound when timed alone, they run on a side stream underneath the SAM / CLIP kernels"}
    main["whole_step_algorithmic_tflops"] = whole_tflops
    return main


def prof_read(lib, cls):
    n = C.c_longlong()
    ms, fl, by = C.c_double(), C.c_double(), C.c_double()
    lib.hgl_prof_read(cls, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
    return n.value, ms.value, fl.value, by.value


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_thread_calibration(cores_available):
    """torch's intra-op pool at every hardware thread is not the fastest setting on a many-core host (measured on the GPU
    box, 2 x 64 cores with SMT: 256 threads took 288 s for the ref, five times the 8-vCPU build container): the CPU leg runs
    at the BEST of {all, 1/2, 1/4, ...} threads, chosen on a probe of the dominant stage -- two blocks of the SAM ViT-H
    encoder (one windowed, one global: oracle/torch_cpu.py image_encoder on the `vit_h_d2` geometry) -- walking down while
    it gets faster.  Returns (threads, {threads: seconds per probe})."""
    import torch
    from hybridgl_amd import weights
    from oracle import torch_cpu as T
    cfg = weights.SAM_CONFIGS["vit_h_d2"]
    sst = T.to_torch(weights.sam_state_dict("vit_h_d2", 0))
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((3, 1024, 1024)).astype(np.float32))
    tried, best, best_t = {}, cores_available, None
    n = cores_available
    with torch.no_grad():
        torch.set_num_threads(max(4, n // 2))
        T.image_encoder(sst, x, cfg)               # untimed: first-touch pages, primitive caches
        while n >= 4:
            torch.set_num_threads(n)
            t = time.perf_counter()
            T.image_encoder(sst, x, cfg)
            dt = time.perf_counter() - t
            tried[str(n)] = round(dt, 3)
            if best_t is None or dt < best_t:
                best, best_t = n, dt
            elif dt > 1.25 * best_t:
                break
            n //= 2
    return best, tried


def cpu_baseline(fusion_mode, with_sam=True, with_gem=False, clip_name="ViT-B/16", host_cores=None):
    """The reference's CPU path restated in plain PyTorch (oracle/torch_cpu.py: nn.Linear / LayerNorm / softmax / matmul in
    fp32, the operators the reference runs with device = "cpu", Hybridgl_main.py:30-34), timed on the host cores: ONE ref of
    the benchmarked workload, UNSAMPLED where the work is -- the CLIP hybrid encoder on all 64 masks, the 12 text strings, all
    32 blocks of the SAM ViT-H encoder, the mask decoder on all 64 prompts.  The cheap stages (blur, view synthesis, the
    three-sentence tail, post-processing of a sample of the candidates) run through the numpy oracle.  The bench confines
    itself to 32 cores and shrinks torch's thread pool for the GPU run: both are undone for this leg (every core the process
    was started on, torch threads = that count) and restored afterwards."""
    import torch
    from hybridgl_amd import synth, weights
    from oracle import clip_oracle as O
    from oracle import cv_oracle as CV
    from oracle import sam_oracle as S
    from oracle import torch_cpu as T
    pinned = sorted(os.sched_getaffinity(0))
    threads_before = torch.get_num_threads()
    if host_cores:
        try:
            os.sched_setaffinity(0, host_cores)
        except OSError:
            pass
    cores_available = len(os.sched_getaffinity(0))
    cores, tried = cpu_thread_calibration(cores_available)
    torch.set_num_threads(cores)
    try:
        geom = CLIP_GEOM[clip_name]
        sd = weights.clip_state_dict(clip_name, 0)
        sdt = T.to_torch(sd)
        H = W = 640
        img = synth.synth_image(H, W, 1000)
        norm = synth.imagenet_normalize(img)
        masks = synth.synth_masks(64, H, W, 2000)
        boxes = synth.boxes_from_masks(masks)
        tokens = synth.synth_tokens(12 if with_gem else 9, 77, 49408, 3000)
        stages = {}
        with torch.no_grad():
            t = time.perf_counter()
            blur = CV.gaussian_blur_u8(img, 15)
            loc, glo = O.synthesize_views(img, blur, norm, masks, 224)
            stages["blur + view synthesis (numpy)"] = time.perf_counter() - t
            t = time.perf_counter()
            feats = T.clip_hybrid_forward(sdt, torch.from_numpy(loc), torch.from_numpy(glo), torch.from_numpy(masks),
                                          geom["masking_block"], fusion_mode, geom["last_layer"]).numpy()
            stages[f"CLIP {clip_name} hybrid {fusion_mode}, 64 masks"] = time.perf_counter() - t
            t = time.perf_counter()
            text = T.encode_text(sdt, tokens).numpy()
            stages[f"text encoder, {len(tokens)} strings"] = time.perf_counter() - t
            t = time.perf_counter()
            for j in range(3):
                d, r, nn = synth.PARSE_RECORDS[j]
                attn = synth.synth_heatmap(H, W, 4000 + j)
                gem = O.coherence_scores(attn, masks, d, 1.8)
                ip, ifin, _, _ = O.score_sentence(feats, 0.5 * text[3 * j:3 * j + 1] + 0.5 * text[3 * j + 1:3 * j + 2],
                                                  text[3 * j + 2:3 * j + 3], boxes, gem, 100.0, 3, 6, 0.6, r, nn != 0)
                O.compute_iou(masks[ip], masks[0]); O.compute_iou(masks[ifin], masks[0])
            stages["3-sentence tail + IoU (numpy)"] = time.perf_counter() - t
            if with_gem:
                from hybridgl_amd.gem import get_gem_img_transform
                from oracle import gem_oracle as GO
                timg = get_gem_img_transform()(img).numpy()
                # the position embedding interpolated to the 28 x 28 grid: a table, computed once per resolution, not timed
                pos = torch.from_numpy(GO.interpolate_pos_encoding(sd["visual.positional_embedding"], 448 // sd["visual.conv1.weight"].shape[2], 448 // sd["visual.conv1.weight"].shape[2]))
                t = time.perf_counter()
                feat = T.gem_vit_forward(sdt, torch.from_numpy(timg[None]), pos)
                heat = T.gem_heatmap(feat[0], torch.from_numpy(text[:3]), 448).numpy()
                GO.resize_bilinear_aa(heat, H, W)
                stages["GEM heat-maps: 1 image at 448 (torch CPU) + 3 maps (the reference re-encodes per sentence)"] = time.perf_counter() - t
            if with_sam:
                cfg = weights.SAM_CONFIGS["vit_h"]
                ssd = weights.sam_state_dict("vit_h", 0)
                sst = T.to_torch(ssd)
                x = S.preprocess(S.pil_bilinear_resize(img, 1024, 1024), 1024)
                t = time.perf_counter()
                emb = T.image_encoder(sst, torch.from_numpy(x), cfg)
                stages["SAM ViT-H encoder, 32 blocks"] = time.perf_counter() - t
                pts = S.point_grid(8) * 1024.0
                sparse = torch.from_numpy(S.embed_points(ssd, pts, 1024))
                t = time.perf_counter()
                low, iou = T.mask_decoder(sst, emb, sparse)
                stages["SAM mask decoder, 64 prompts"] = time.perf_counter() - t
                t = time.perf_counter()
                T.postprocess_and_stats(low, (1024, 1024), (640, 640))
                stages["post-processing, stability, boxes of the 192 candidates"] = time.perf_counter() - t
        t_ref = sum(stages.values())
    finally:
        torch.set_num_threads(threads_before)
        try:
            os.sched_setaffinity(0, pinned)
        except OSError:
            pass
    return {"value": 1.0 / t_ref, "unit": "images/s", "cores": cores, "kind": "port", "cpu_model": cpu_model_name(),
            "torch_threads": cores, "cores_available": cores_available, "threads_tried_s_per_probe": tried,
            "seconds_per_ref": t_ref,
            "stages_s": {k: round(v, 3) for k, v in stages.items()},
            "reference_torch_cpu": {"value": 0.014, "unit": "images/s", "cores": 8,
                                    "note": "the reference's own torch CPU path (imported, seeded weights) measured in the build "
                                            "container on 8 vCPU, BASELINE.md section 2 / SURVEY.md section 6: ~73 s per ref; the reference "
                                            "cannot travel to the GPU box, so this number is quoted, not re-measured there"},
            "sample": "ONE ref of the benchmarked workload through oracle/torch_cpu.py (plain PyTorch fp32 on the CPU, pinned to the numpy "
                      "oracle by tests/test_torch_cpu_baseline.py): CLIP hybrid on all 64 masks, all text strings, all 32 SAM encoder "
                      "blocks, the decoder on all 64 prompts and the post-processing of all 192 candidates, nothing sampled or "
                      "extrapolated; the GEM tower likewise (oracle/torch_cpu.py gem_vit_forward); blur, views, tail and the final resize of the heat-maps through the numpy oracle"}


PMC_PASS = {"groups": 2, "refs_per_group": 16}      # what the counter pass ran (set by live_pmc_table): launches per ref derive from it


def live_pmc_table(timeout_s=150.0, refs=16, groups=1):
    """Per-kernel HBM bytes and launch times of the headline's loop, measured NOW: two child processes `rocprofv3 --pmc
    FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, counters only, as MI355X_MICROARCH.md prescribes) over
    tools/group_profile.py (one serial group of `refs` refs after a warm-up group, same models and shapes), corrected as that
    guide says (KB units x1024, FETCH_SIZE x2 on gfx950).  Returns ({kernel: {launches, fetch_bytes, write_bytes, us}}, note)
    with per-launch averages (us from the kernel trace of the FETCH_SIZE pass: a profiled pass, a few per cent slow), or
    (None, why not)."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from profile_summary import short
    out = tempfile.mkdtemp(prefix="hgl_pmc_")
    try:
        sums, dur = {}, collections.defaultdict(lambda: [0, 0.0])
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(out, ctr)
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run([exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--",
                                sys.executable, os.path.join(ROOT, "tools", "group_profile.py"), str(groups), str(refs)],
                               cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} exited {r.returncode}"
            acc = collections.defaultdict(lambda: [0, 0.0])
            for path in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if row["Counter_Name"] == ctr:
                        k = short(row["Kernel_Name"])
                        acc[k][0] += 1
                        acc[k][1] += float(row["Counter_Value"])
            sums[ctr] = acc
            if ctr == "FETCH_SIZE":
                for path in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        k = short(row["Kernel_Name"])
                        dur[k][0] += 1
                        dur[k][1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        table = {}
        PMC_PASS["groups"], PMC_PASS["refs_per_group"] = groups + 1, refs      # group_profile.py runs a warm-up group first
        for k, (n, v) in sums["FETCH_SIZE"].items():
            nw, vw = sums["WRITE_SIZE"].get(k, [0, 0.0])
            table[k] = {"launches": n, "fetch_bytes": 2.0 * 1024.0 * v / max(n, 1), "write_bytes": 1024.0 * vw / max(nw, 1),
                        "us": dur[k][1] / max(dur[k][0], 1)}
        return table, ("measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate child processes) over "
                       f"tools/group_profile.py {groups} {refs} (a warm-up group + {groups} serial group(s) of {refs} refs: launches / "
                       f"{(groups + 1) * refs} = launches per ref), FETCH x2 x1024 and WRITE x1024 bytes per launch")
    except Exception as e:
        return None, repr(e)[:200]
    finally:
        shutil.rmtree(out, ignore_errors=True)


def live_pmc_traffic(table, note, prefix):
    """HBM bytes per launch of the kernels whose name starts with `prefix`, launch-weighted over the template instantiations."""
    if table is None:
        return None, note
    ks = [k for k in table if k.startswith(prefix)]
    n = sum(table[k]["launches"] for k in ks)
    if n == 0:
        return None, f"no launch of {prefix} in the counter pass"
    fetch = sum(table[k]["launches"] * table[k]["fetch_bytes"] for k in ks) / n
    write = sum(table[k]["launches"] * table[k]["write_bytes"] for k in ks) / n
    return fetch + write, (f"{note}; {n} launches of {prefix}...> (fetch {fetch / 1e9:.3f} GB + write {write / 1e9:.3f} GB per launch)")


# The HBM-bound kernels north_star names (per-mask pooling / reductions, post-processing, view synthesis, clean-up): ALGORITHMIC
# bytes per launch at the benchmarked shape (N = 64 proposals, 640 x 640, S = 3 sentences, 192 candidates of
# 256 x 256 low-res logits; `g` = refs per launch for the group-wide tail), stated per kernel in DESIGN.md section 5.
def hbm_kernel_specs(N=64, H=640, W=640, S=3, K=192, g=1):
    px = H * W
    return {
        "grp_masked_pool_kernel": (g * (N * px + S * 4 * px), f"the group's {g} refs in one launch: N*H*W mask bytes + S heat-maps of 4*H*W "
                                                             "each (K10: 31.1 MB per ref)"),
        "grp_minmax_kernel": (g * S * 4 * px, "S heat-maps per ref read once"),
        "grp_iou_kernel": (g * S * 2 * 2 * px, "two winners x (mask + target) bytes per sentence (K12)"),
        "ref_masked_pool_kernel": (N * px + S * 4 * px, "N*H*W mask bytes + S heat-maps of 4*H*W (K10: 31.1 MB per ref)"),
        "ref_minmax_kernel": (S * 4 * px, "S heat-maps read once"),
        "ref_iou_kernel": (S * 2 * 2 * px, "two winners x (mask + target) bytes per sentence (K12)"),
        "sam_postprocess_sep_kernel": (K * 256 * 256 * 4 + K * px // 8, "read K*256^2*4 B of low-res logits, write K*H*W mask BITS (K18 "
                                                                       "minimal: 50.3 + 9.8 MB; the kernel writes bytes: 78.6 MB)"),
        "synth_views_kernel": (2 * N * 3 * 224 * 224 * 4 + 2 * px * 3 + N * px // 8, "write both views (77 MB) + sharp / blurred image + mask bits (K9)"),
        # the clean-up (round 6): the first pass packs the working bits (one eighth of the mask bytes), every later pass scans
        # bit rows; run links / areas live in int planes touched at run starts only (data-dependent: not in the algorithmic figure)
        "ccl_rows_kernel": (N * px + N * px // 8, "mask bytes read once, working bits written"),
        "ccl_strip_kernel": (N * px // 8, "bit plane read (strips of 16 rows linked in LDS; run links written at run starts)"),
        "ccl_merge_kernel": (N * px // 8 // 8, "bit rows of the row pairs BETWEEN strips (an eighth of the rows, read as pairs)"),
        "ccl_count_kernel": (N * px // 8, "bit plane read once"),
        "ccl_stats_kernel": (N * px // 8, "bit plane read once"),
        "ccl_apply_kernel": (N * px // 8 + N * px, "bit plane read + cleaned mask bytes written (+ the per-row box words)"),
        "blur_q8_tile_kernel": (3 * px + 3 * px, "u8 image read, u8 image written (both passes in LDS; the tile halos -- 3.9x the image -- are re-reads inside an XCD's L2)"),
        "mask_resize_kernel": (N * 14 * 14 * 4 * 2, "4 taps per output of the 14 x 14 CLS keep maps (never the 26 MB of masks)"),
        # LayerNorm between the fp32 residual stream and the split GEMM operands: 8 B per element (fp32 row in, fp16 hi + lo row
        # out) is the floor of such a pass, and launches differ in rows -- the measured bytes ARE the algorithmic bytes here
        "layernorm_split_kernel<3>": (None, "= measured: 4 B in + 4 B out per element, CLIP / GEM width 768 (one wave per row, row in registers)"),
        "layernorm_split_kernel<5>": (None, "= measured: 4 B in + 4 B out per element, SAM width 1280"),
    }


def hbm_kernel_table(table, refs_in_pass=None, tail_group=1):
    """roofline.hbm_kernels: per kernel launches per ref, us per launch (profiled pass), measured bytes per launch (PMC),
    algorithmic bytes per launch, TB/s on both, fraction of the 8 TB/s HBM3E peak on the algorithmic bytes."""
    if table is None:
        return None
    out = {}
    if refs_in_pass is None:
        refs_in_pass = PMC_PASS["groups"] * PMC_PASS["refs_per_group"]
    specs = hbm_kernel_specs(g=tail_group)
    for k, (alg, what) in specs.items():
        ks = [t for t in table if t == k or t.startswith(k + "<")]
        n = sum(table[t]["launches"] for t in ks)
        if n == 0:
            continue
        us = sum(table[t]["launches"] * table[t]["us"] for t in ks) / n
        meas = sum(table[t]["launches"] * (table[t]["fetch_bytes"] + table[t]["write_bytes"]) for t in ks) / n
        if alg is None:
            alg = meas
        out[k] = {"launches_per_ref": n / float(refs_in_pass), "us_per_launch": us, "measured_bytes_per_launch": meas,
                  "algorithmic_bytes_per_launch": alg, "algorithmic_bytes": what,
                  "TBps_measured": meas / us / 1e6 if us > 0 else None, "TBps_algorithmic": alg / us / 1e6 if us > 0 else None,
                  "frac_of_hbm_peak": alg / us / 1e6 / PEAK_HBM_TBPS if us > 0 else None,
                  "ms_per_ref": n / float(refs_in_pass) * us / 1e3}
    if out:
        out["_sum_ms_per_ref"] = sum(v["ms_per_ref"] for v in out.values() if isinstance(v, dict))
        out["_note"] = ("bound: hbm; peak 8 TB/s (MI355X_MICROARCH.md; 6.3 TB/s is what a streaming copy reaches).  us_per_launch comes from "
                        "the kernel trace of the FETCH_SIZE pass (profiled: a few per cent slow).  Kernels of a few tens of "
                        "microseconds on a few tens of MB are launch- / latency-bound, not bandwidth-bound: the fraction says how "
                        "far, the measured bytes say whether bytes are wasted")
    return out


def evaluator_from_disk(args, model, gen, gem_model, dev, group, n_images=208, keep_root=None, host_cores=None):
    """`python -m hybridgl_amd.main --real` on a synthetic REFER tree written to local disk (hybridgl_amd.synth.write_refer_tree:
    COCO-sized JPEGs of 8 sizes, 2-3 refs per image, 3 sentences per ref, polygon ground truth, parse records, a BPE merges
    file): JPEG decode, BPE, ground-truth rasterisation and pinned uploads on 4 loader threads (hybridgl_amd.loader.Prefetcher),
    the two dataset transforms on the device, the product's run() loop with its per-image cache.  Same models as the
    headline (filters open, first 64 proposals).  Timings of the SAME refs: from disk on the cores this process is pinned to
    (at most 32: a rank's share of an 8-GPU job on a 256-core host); the same items resident in HBM (what the headline's
    loop sees); from disk on 8 cores and roaming over all host cores (`host_cores`: the affinity before pinning)."""
    import shutil
    import tempfile
    from hybridgl_amd import dist as D, main as drv, synth
    from hybridgl_amd.pipeline import HybridGLPipeline
    root = keep_root or tempfile.mkdtemp(prefix="hgl_refer_")
    try:
        t0 = time.perf_counter()
        info = synth.write_refer_tree(root, n_images=n_images)
        t_write = time.perf_counter() - t0
        a = drv.default_argument_parser().parse_args([
            "--real", "--refer_data_root", root, "--dataset", "refcoco", "--split", "val", "--bpe_vocab", os.path.join(root, "bpe.txt.gz"),
            "--parse_json", os.path.join(root, "parse.json"), "--proposal_cap", str(args.masks), "--group", str(group),
            "--fusion_mode", args.fusion, "--clip_model", args.clip, "--heatmap", args.heatmap])
        a.masking_block = CLIP_GEOM[args.clip]["masking_block"]

        def leg(**over):
            b = argparse.Namespace(**{**vars(a), **over})
            m, st = drv.evaluate(b, model, gen, gem_model, dev)
            return m, {"value": st["refs"] / st["seconds"], "unit": "images/s", "refs": st["refs"], "seconds": st["seconds"],
                       "ms_per_ref": st["seconds"] / max(st["refs"], 1) * 1e3,
                       "distinct_images_per_s": st["images_decoded"] / st["seconds"] if st["images_decoded"] else None,
                       "loader_wait_ms_per_group": st["loader_wait_s"] / max(st["groups"] or 1, 1) * 1e3,
                       "loader_wait_frac": st["loader_wait_s"] / st["seconds"],
                       "loader_cpu_ms_per_ref": st["loader_make_s"] / max(st["refs"], 1) * 1e3,
                       "images_decoded": st["images_decoded"], "image_cache_hits": st["image_cache_hits"], "groups": st["groups"],
                       "skipped": st["skipped"], "workers": st["workers"]}
        leg(max_refs=4 * group)                               # warm: page cache, allocator, coefficient tables, BPE cache
        m_disk, disk = leg()
        # the same items resident in HBM before the clock starts (what bench.py's headline loop is fed)
        rr = drv.RealRefs(a, dev, "unc", 77)
        resident = [rr.load(i) for i in rr.jobs()]
        torch.cuda.synchronize()
        pipe = HybridGLPipeline(model, fusion_mode=args.fusion, masking_block=a.masking_block, mask_generator=gen, use_sam_masks=True,
                                gem_model=gem_model)
        t1 = time.perf_counter()
        n = pipe.run(iter(resident), group=group, proposal_cap=args.masks)
        torch.cuda.synchronize()
        t_res = time.perf_counter() - t1
        m_res = pipe.metrics()
        del resident, pipe
        torch.cuda.empty_cache()
        # other core budgets for the same feed: this thread (and the loader threads it starts) confined to 8 cores (a quarter
        # of what a rank of an 8-GPU job owns on this host), and roaming over every core of the host (no pinning)
        now_cores = sorted(os.sched_getaffinity(0))
        variants = {}
        old_threads = torch.get_num_threads()
        for name, share in (("eight_cores", now_cores[:8]), ("all_host_cores_unpinned", list(host_cores or now_cores))):
            if not share or share == now_cores:
                continue
            try:
                os.sched_setaffinity(0, share)
                D.size_host_threads(share, a.workers)
                _, v = leg()
                v["host_cores"] = len(share)
                variants[name] = v
            except OSError as e:
                variants[name] = {"error": repr(e)}
            finally:
                os.sched_setaffinity(0, now_cores)
                torch.set_num_threads(old_threads)
        out = dict(disk)
        out.update({
            "config": f"synthetic REFER tree on local disk: {info['images']} JPEGs (8 COCO sizes up to 640x640), {info['refs']} refs "
                      f"(2-3 per image, ~10 % of them ~20 images late), {info['sentences']} sentences; python -m hybridgl_amd.main "
                      f"--real --group {group} --workers {a.workers} --proposal_cap {args.masks} (evaluate()), filters open; the refs of an "
                      "image share its proposals / hybrid / GEM features (the product's image cache), so a ref costs less "
                      "than a headline step, whose refs are all different images",
            "host_cores": len(now_cores),
            "host_cores_note": "the cores this process is confined to (hybridgl_amd.dist.pin_rank_to_cores: at most 32 per rank, = the "
                               "share of a rank of an 8-GPU job on a 256-core host)",
            "tree_write_s": t_write,
            "resident_same_items": {"value": n / t_res, "unit": "images/s", "seconds": t_res,
                                    "note": "the same RefBatches already in HBM, same run() call, same image cache"},
            "disk_over_resident": (disk["value"] / (n / t_res)) if n else None,
            "other_core_budgets": variants,
            "metrics_equal_resident": m_disk == m_res,
            "metrics": m_disk,
        })
        # the same evaluator as EIGHT ranks sharing this GPU (tools/evaluator_ranks.py: python -m hybridgl_amd.main --real x 8, gloo,
        # 32 cores each): a separate tool run (8 model sets, ~45 s), REPLAYED here from the tracked file of the last evidence pass
        import glob as _glob
        tags = sorted({os.path.basename(f).split("_evaluator_8ranks_gloo.json")[0]
                       for f in _glob.glob(os.path.join(ROOT, "profiles", "r*_evaluator_8ranks_gloo.json"))}, reverse=True)
        for tag in tags:      # the newest evidence pass that has both files (tags sort by round, then by letter)
            p8 = os.path.join(ROOT, "profiles", f"{tag}_evaluator_8ranks_gloo.json")
            p1 = os.path.join(ROOT, "profiles", f"{tag}_evaluator_1rank.json")
            if os.path.exists(p8) and os.path.exists(p1):
                try:
                    j8, j1 = json.load(open(p8)), json.load(open(p1))
                    out["eight_ranks_one_gpu"] = {
                        "value": j8["value"], "unit": j8["unit"], "host_cores_per_rank": j8["host_cores_per_rank"],
                        "one_rank_same_tree": j1["value"], "images": j8["tree"]["images"], "refs": j8["tree"]["refs"],
                        "rank0_loader_wait_s": j8["rank0"]["loader_wait_s"], "seconds_job": j8["seconds_job"],
                        "source": f"profiles/{tag}_evaluator_8ranks_gloo.json / _1rank.json -- replayed, not measured in this run"}
                except Exception:
                    pass
                break
        return out
    finally:
        if keep_root is None:
            shutil.rmtree(root, ignore_errors=True)


def dump_outputs(out_dir, last_step, n_sent, rows, winners):
    """--dump-outputs: the arrays the caller of the timed loop receives for its LAST ref -- (hybrid, text, last-sentence
    tensors) as HybridGLPipeline.step() returns them and run(collect=True) keeps them, plus that ref's `n_sent` rows of
    partial_rows() / winning_indices() -- as out_dir/<name>.npy, float32 (features, scores) or float64 (indices, counts).
    Two outputs are NaN by definition in places, as in the reference: the coherence score of an empty proposal (0 / 0) and
    the negative-noun logits of a sentence without other nouns.  Every file holds finite values only, so those two are
    written with 0 in place of a NaN, and <name>_finite.npy (1 / 0 per entry) says which entries the path defined."""
    hybrid, text, last = last_step
    out = {"hybrid_features": hybrid, "text_features": text,
           "sentence_winning_indices": winners[len(winners) - n_sent:],
           "sentence_iou_counts": rows[len(rows) - n_sent:, 2:6]}
    if last is not None:
        idx, score_clip, score_neg, coherence = last
        out.update(last_sentence_indices=idx, last_sentence_score_clip=score_clip, last_sentence_score_neg=score_neg,
                   last_sentence_coherence=coherence)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        a = a.astype(np.float32 if a.dtype.kind == "f" and a.itemsize <= 4 else np.float64)
        if name in ("last_sentence_score_neg", "last_sentence_coherence"):
            finite = np.isfinite(a)
            np.save(os.path.join(out_dir, name + "_finite.npy"), finite.astype(np.float32))
            a = np.where(finite, a, np.zeros_like(a))
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128,
                    help="timed steps (refs); the default is a whole number of groups of --sam-batch images (8 groups: the "
                         "fill and the drain of the two-stream loop, which are inside the timed region, weigh 1 / 8 each)")
    ap.add_argument("--warmup", type=int, default=32, help="untimed steps (refs); the default is two full groups")
    ap.add_argument("--fusion", default="G2L", choices=["G2L", "L2G", "G2L&L2G"])
    ap.add_argument("--clip", default="ViT-B/16", choices=list(CLIP_GEOM),
                    help="CLIP geometry: ViT-B/16 = the reference's configuration; ViT-L/14 = the extension BASELINE.json names")
    ap.add_argument("--masks", type=int, default=64)
    ap.add_argument("--pool", type=int, default=16, help="distinct synthetic refs resident per rank (a group of 16 = 16 different images)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run the SAM stage and the CLIP stage of the loop back to back on one stream (HybridGLPipeline.run(serial=True)) "
                         "instead of the SAM stage of group g+1 beside the CLIP stage of group g on two streams")
    ap.add_argument("--heatmap", default="device", choices=["device", "given"],
                    help="device: the GEM heat-map stage (ViT-B/16 at 448x448 with self-self attention, 3 prompts) runs "
                         "inside the step; given: seeded heat-maps are inputs (the stage is then outside the timed work)")
    ap.add_argument("--blur", default="device", choices=["device", "given"],
                    help="device: cv2.GaussianBlur's fixed-point filter runs inside the step; given: the blurred image is an input")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to exercise the N > 1 path on a box "
                         "with fewer GPUs than ranks)")
    ap.add_argument("--sam-batch", type=int, default=16, choices=[1, 2, 4, 8, 12, 16, 24, 32],
                    help="images per group of the evaluation loop (HybridGLPipeline.run): ONE SAM encoder pass over the images of "
                         "group g+1 (token rows stacked, weights read once) beside ONE text-encoder batch + ONE hybrid forward "
                         "over the proposals of group g; same work and same results per ref (1: ref by ref, HybridGLPipeline.step)")
    ap.add_argument("--proposals-from", default="sam", choices=["sam", "seeded"],
                    help="sam (default): the CLIP stage scores SAM's OWN masks -- the first --masks survivors of the first NMS of "
                         "every image go through the small-region clean-up and the second NMS into view synthesis and the hybrid "
                         "forward, their counts are read back (two device->host copies per group); seeded: rounds 1-2's workload -- "
                         "the SAM proposal kernels run and their output is discarded, the clean-up + CLIP stages take the items' "
                         "seeded proposal-shaped masks (no count read-back)")
    ap.add_argument("--scope", default="B", choices=["A", "B"],
                    help="A: proposals given (CLIP + scoring only); B: + SAM ViT-H proposal stage (full path)")
    ap.add_argument("--no-balance", action="store_true", help="full groups of --sam-batch and a remainder instead of equally full groups (A/B)")
    ap.add_argument("--no-prepare", action="store_true", help="skip HybridGLPipeline.prepare before the warm-up (A/B of the first-use cost)")
    ap.add_argument("--no-also", action="store_true",
                    help="skip the short secondary timings (seeded masks, L2G, G2L&L2G, strict fp32, ViT-L/14, PhraseCut) that are "
                         "attached under the `also` key at N = 1")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="N = 1: do not measure roofline.traffic in this run (two rocprofv3 --pmc child processes, ~1 min); replay "
                         "profiles/pmc_traffic.json instead")
    ap.add_argument("--no-rccl-check", action="store_true",
                    help="N = 1: skip the RCCL self-check (nccl backend in a world of one, the timed steps' metric rows through it)")
    ap.add_argument("--no-disk", action="store_true", help="skip also['evaluator_from_disk'] (the evaluator fed from a REFER tree on disk)")
    ap.add_argument("--timeout", type=float, default=3600.0, help="--gpus N without a launcher: seconds before the ranks are killed")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the measurements that take runs of their own: the roofline leg (one "
                         "serial group with HIP events around every launch), and at N = 1 the live counter passes, the `also` "
                         "legs, the evaluator from disk, the RCCL self-check and the CPU baseline (each --no-* option above "
                         "drops one of them); without it the line carries the headline and the timed region only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step (the last ref) computed as DIR/<name>.npy (float32 / float64): its "
                         "hybrid and text features, the last sentence's scores, every sentence's winning indices and IoU "
                         "counts (rank 0; the timed run keeps each ref's outputs, HybridGLPipeline.run(collect=True)); entries "
                         "the path leaves NaN are written as 0 and flagged in <name>_finite.npy")
    args = ap.parse_args()

    from hybridgl_amd import dist as D
    rank, local_rank, world = D.env_rank()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # No launcher: start the N ranks here.  Nothing above has touched the GPU (importing torch and counting devices
        # does not create a context); the children are fresh interpreters, rank 0 prints the one JSON line.
        ngpu = D.visible_gpu_count()
        argv = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
        if ngpu < args.gpus and args.backend == "nccl":
            # RCCL cannot put two ranks on one device; gloo can (exercises the N > 1 path on a box with fewer GPUs)
            print(f"bench.py: {args.gpus} ranks on {ngpu} visible GPU(s): ranks share devices, metric exchange over gloo",
                  file=sys.stderr)
            argv += ["--backend", "gloo"]
        sys.exit(D.spawn_local_ranks(args.gpus, argv, timeout=args.timeout))
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world}; reporting n_gpus={world}", file=sys.stderr)
    # The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a version banner at communicator
    # creation): from here on fd 1 is stderr for everything in this process, and the line goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU path exists)"
    ngpu = torch.cuda.device_count()
    local_dev = local_rank % ngpu      # identity on a node with one GPU per rank
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    host_cores_at_start = sorted(os.sched_getaffinity(0))
    cores = D.pin_rank_to_cores(local_rank, local_world)    # each rank's launch thread on its own share of the host cores
    D.size_host_threads(cores, 4)
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    dist = None
    if world > 1:
        dist = D.init_process_group(args.backend, dev)

    from hybridgl_amd import _lib, ops
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.pipeline import HybridGLPipeline, synthetic_ref

    lib = _lib.load()
    geom = CLIP_GEOM[args.clip]
    model = CLIPViTFM(args.clip, seed=0, device=dev)
    gen = sam = None
    dependent = args.scope == "B" and args.proposals_from == "sam"

    def make_gen(sam_model):
        from hybridgl_amd.sam import SamAutomaticMaskGenerator
        # Hybridgl_main.py:67-73 (8x8 grid, no crops, min_mask_region_area=800).  With random weights the reference
        # thresholds (0.7 / 0.7 / NMS 0.7) would keep an arbitrary number of proposals, so the benchmark opens the three
        # filters ("AMG filters forced to keep a fixed 64", SURVEY.md 8d scope B): every candidate reaches the first NMS,
        # the first --masks of its order go on.
        return SamAutomaticMaskGenerator(sam_model, points_per_side=8, pred_iou_thresh=-1e30, stability_score_thresh=0.0,
                                         box_nms_thresh=2.0, crop_n_layers=0, crop_n_points_downscale_factor=1,
                                         min_mask_region_area=800)
    if args.scope == "B":
        from hybridgl_amd.sam import sam_model_registry
        sam = sam_model_registry["default"](seed=0, device=dev)
        gen = make_gen(sam)
    use_gem = args.heatmap == "device"
    gem_model = None
    if use_gem:
        # Hybridgl_main.py:36-38: the same OpenAI ViT-B/16 checkpoint as the CLIP stage -> shared device weights
        from hybridgl_amd.gem import create_gem_model
        gem_model = create_gem_model(args.clip, clip=model)

    def make_pipe(m=model, g=gen, gm=gem_model, fusion=args.fusion, mb=geom["masking_block"], dep=dependent):
        return HybridGLPipeline(m, fusion_mode=fusion, masking_block=mb, mask_generator=g, use_sam_masks=dep,
                                fixed_proposals=args.masks if (dep and args.sam_batch == 1) else None,
                                cleanup_given_masks=g is not None and not dep, gem_model=gm)
    pipe = make_pipe()
    # rank r owns refs i = r (mod world) of the shuffle=False order
    refs = [synthetic_ref(D.owned_index(j, rank, world), dev, N=args.masks, sam_img_size=1024 if gen else 0, gem=use_gem,
                          device_blur=args.blur == "device")[0]
            for j in range(args.pool)]

    def barrier():
        if world > 1:
            dist.barrier()

    nbatch = args.sam_batch

    def do_steps(k, p=None, cap=args.masks, pool=None, group=None, collect=False):
        """k steps = k refs completed, start to finish (proposal stage + CLIP/scoring stage of each), through the PRODUCT's
        loop: HybridGLPipeline.run over a loader that yields k resident refs (hybridgl_amd.main runs the same call over a
        Prefetcher).  collect=True: returns the last ref's (hybrid, text, last-sentence tensors), as step() returns them."""
        p = p or pipe
        pool = pool or refs
        if nbatch == 1:
            out = None
            for i in range(k):
                out = p.step(pool[i % len(pool)])
            return out if collect else None
        n = p.run((pool[i % len(pool)] for i in range(k)), group=group or nbatch, proposal_cap=cap if p.use_sam_masks else None,
                  serial=args.no_overlap, total=None if args.no_balance else k, collect=collect)
        assert n == k, f"{k - n} refs were skipped (no proposals)"
        if collect:
            last = p.collected[-1] if p.collected else None
            p.collected = None
            return last

    prepared = None
    if nbatch >= 2 and not args.no_prepare:
        # the product's own set-up call (HybridGLPipeline.prepare: workspaces, allocator blocks and kernel instantiations
        # of the group sizes the loop will meet), part of building the pipeline like loading the weights: the length of the
        # warm-up then decides nothing
        t_p = time.perf_counter()
        g_timed = nbatch if args.no_balance else HybridGLPipeline.balanced_group(args.steps, nbatch)
        pipe.prepare(group=g_timed, H=640, W=640, proposals=args.masks, n_sent=3,
                     tail=HybridGLPipeline.balanced_group(max(args.warmup, 1), nbatch), serial=args.no_overlap)
        prepared = {"group": g_timed, "seconds": time.perf_counter() - t_p}
    do_steps(args.warmup)
    torch.cuda.synchronize()
    # the metric rows of the report are those of the timed steps only
    pipe.cum.zero_(); pipe.iu_log.clear(); pipe.iu_owner.clear(); pipe.idx_log.clear()
    ops.split_overflow_count(reset=True)
    barrier()
    torch.cuda.synchronize()
    # diagnostics of the timed region that cost nothing inside it: the allocator's device-malloc counter before / after, a
    # host-side stamp per group boundary (HybridGLPipeline.group_marks) and the host time at which the last launch was enqueued
    mallocs0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
    pipe.group_marks = []
    pipe.stage_marks = []
    ev0 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    t0 = time.perf_counter()
    last_step = do_steps(args.steps, collect=args.dump_outputs is not None)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    timed_region = {"seconds": dt, "host_enqueue_seconds": t_enq,
                    "group_start_ms": [round((g - t0) * 1e3, 2) for g in pipe.group_marks],
                    "device_mallocs": torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - mallocs0,
                    "reserved_GiB": round(torch.cuda.memory_reserved(dev) / 2**30, 2),
                    # (stage, group, device ms, host ms): the proposal stage of group g+1 should lie beside the CLIP stage of group g
                    "stages": pipe.stage_timeline(ev0, t0)}
    pipe.group_marks = pipe.stage_marks = None
    rows = pipe.partial_rows()
    # fp16 range guard of the f16x3 mode (ops.check_split_overflow): GPU threads that met |x| > 65504 in the timed steps
    overflow = ops.split_overflow_count(reset=True)
    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, last_step, len(refs[(args.steps - 1) % len(refs)].sentences), rows, pipe.winning_indices())
    del last_step

    # ---- roofline leg: one group of the same loop with every stage on ONE stream, HIP events around every launch
    if args.full:
        lib.hgl_prof_enable(1)
        nprof = max(nbatch, 2)
        keep_rows = (pipe.cum.clone(), list(pipe.iu_log), list(pipe.iu_owner), list(pipe.idx_log))
        if nbatch == 1:
            for i in range(nprof):
                pipe.step(refs[i % len(refs)])
        else:
            pipe.run((refs[i % len(refs)] for i in range(nprof)), group=nbatch, proposal_cap=args.masks if pipe.use_sam_masks else None,
                     serial=True)
        torch.cuda.synchronize()
        lib.hgl_prof_enable(0)
        pipe.cum.copy_(keep_rows[0]); pipe.iu_log[:] = keep_rows[1]; pipe.iu_owner[:] = keep_rows[2]; pipe.idx_log[:] = keep_rows[3]
        g_n, g_ms, g_fl, g_by = prof_read(lib, 0)
        a_n, a_ms, a_fl, a_by = prof_read(lib, 1)
        x_n, x_ms, x_fl, x_by = prof_read(lib, 3)
        xg_n, xg_ms, xg_fl, xg_by = prof_read(lib, 4)
        fw_n, fw_ms, fw_fl, fw_by = prof_read(lib, 5)
    precision = "f16x3" if lib.hgl_get_precision() == 1 else "f32"

    dt = D.max_over_ranks(dt, dist, dev)
    # the only exchange of the path: one all-gather of the per-sentence metric rows (RCCL over xGMI; hybridgl_amd/dist.py)
    m = D.gather_metrics(rows, dist, dev)
    overflow = int(D.max_over_ranks(float(overflow), dist, dev))

    # ---- short secondary timings in the same process (N = 1 only)
    also = None
    if args.full and world == 1 and not args.no_also and args.scope == "B" and args.fusion == "G2L" and args.clip == "ViT-B/16" and nbatch >= 2 \
            and dependent:
        also = {}

        def timed(p2, n_steps=3 * nbatch, **kw):     # three groups: the middle one runs with both neighbours beside it
            do_steps(n_steps, p2, **kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            do_steps(n_steps, p2, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / n_steps

        def entry(t, n_steps, config, fl=None):
            return {"ms_per_step": t * 1e3, "value": 1.0 / t, "unit": "images/s", "steps": n_steps, "config": config,
                    "whole_step_algorithmic_tflops": None if fl is None else fl / t / 1e12}
        text_S = max(r.token_len or 77 for r in refs)
        t = timed(make_pipe(dep=False))
        also["seeded_masks"] = entry(t, 3 * nbatch, "rounds 1-2's headline workload (--proposals-from seeded): the SAM proposal kernels run, their "
                                     "masks are discarded, clean-up + CLIP take the 64 seeded masks; no count read-back")
        t = timed(make_pipe(fusion="L2G"))
        also["L2G"] = entry(t, 3 * nbatch, "the headline workload with fusion_mode L2G (BASELINE configs[2] per GPU)")
        t = timed(make_pipe(fusion="G2L&L2G"))
        also["G2L&L2G"] = entry(t, 3 * nbatch, "the headline workload with fusion_mode G2L&L2G (BASELINE configs[3] per GPU)")
        # CLIP / GEM weights fp16-valued, as the OpenAI archives the reference loads hold them (clip/model.py:509 is commented
        # out: fp32 tensors with fp16 values): W_lo == 0, the GEMMs on them issue two of the three products (same results) and
        # multiply by zeros less often under the power limit.  The headline keeps genuine fp32 random weights.
        import numpy as _np
        from hybridgl_amd import weights as _w
        sd16 = {k: (_np.asarray(v).astype(_np.float16).astype(_np.float32) if _np.asarray(v).dtype.kind == "f" else v)
                for k, v in _w.clip_state_dict(args.clip, 0).items()}
        model_h = CLIPViTFM(args.clip, state_dict=sd16, device=dev)
        gem_h = None
        if use_gem:
            from hybridgl_amd.gem import create_gem_model
            gem_h = create_gem_model(args.clip, clip=model_h)
        t = timed(make_pipe(m=model_h, gm=gem_h))
        also["clip_weights_fp16_valued"] = entry(t, 3 * nbatch, "the headline workload with CLIP / GEM weights rounded through fp16 (the "
                                                 "values an OpenAI CLIP archive holds); SAM's weights stay genuine fp32")
        del model_h, gem_h, sd16
        torch.cuda.empty_cache()
        # strict fp32: every product an exact fp32 MFMA (v_mfma_f32_32x32x2_f32), own model objects
        model_f = CLIPViTFM(args.clip, seed=0, device=dev, precision="f32")
        from hybridgl_amd.sam import sam_model_registry
        sam_f = sam_model_registry["default"](seed=0, device=dev, precision="f32")
        gem_f = None
        if use_gem:
            from hybridgl_amd.gem import create_gem_model
            gem_f = create_gem_model(args.clip, clip=model_f)
        t = timed(make_pipe(m=model_f, g=make_gen(sam_f), gm=gem_f), n_steps=2 * nbatch)
        also["f32"] = entry(t, 2 * nbatch, "the headline workload with HYBRIDGL_PRECISION=f32 semantics (exact fp32 MFMA products in every "
                                  "GEMM and attention; roofline denominator 157.3 TFLOP/s)",
                            algorithmic_flops_per_ref(args.masks, sam=True, gem=use_gem, clip_name=args.clip, text_S=text_S))
        del model_f, sam_f, gem_f
        torch.cuda.empty_cache()
        gl = CLIP_GEOM["ViT-L/14"]
        model_l = CLIPViTFM("ViT-L/14", seed=0, device=dev)
        gem_l = None
        if use_gem:
            from hybridgl_amd.gem import create_gem_model
            gem_l = create_gem_model("ViT-L/14", clip=model_l)
        t = timed(make_pipe(m=model_l, gm=gem_l, mb=gl["masking_block"]), n_steps=2 * nbatch)
        also["ViT-L/14"] = entry(t, 2 * nbatch, "the headline workload with the CLIP / GEM ViT-L/14 geometry north_star names (masking_block 21)",
                                 algorithmic_flops_per_ref(args.masks, sam=True, gem=use_gem, clip_name="ViT-L/14", text_S=text_S))
        del model_l, gem_l
        torch.cuda.empty_cache()
        # PhraseCut-shaped items (BASELINE configs[4] per GPU; Hybridgl_main_PhraseCut.py:56-62): 64x64 points + one crop
        # layer (5 encoder passes, 128 decoder batches, per-crop + cross-crop NMS over 12288 + 4 x 3072 candidates), 8 phrases
        # per image scored against one hybrid forward; at most 256 proposals per image go on (random weights: noise masks)
        from hybridgl_amd.sam import SamAutomaticMaskGenerator
        PC_PPB = 1024      # prompts per decoder launch (a memory knob: the candidates do not depend on it; 512 in rounds 4-5)
        gen_pc = SamAutomaticMaskGenerator(sam, points_per_side=64, points_per_batch=PC_PPB, pred_iou_thresh=-1e30, stability_score_thresh=0.0,
                                           crop_n_layers=1, crop_n_points_downscale_factor=2, min_mask_region_area=100)
        pc_refs = [synthetic_ref(100 + j, dev, N=args.masks, H=480, W=640, n_sent=8, sam_img_size=1024, gem=use_gem,
                                 device_blur=True)[0] for j in range(2)]
        # three groups of two images: the crop-layer proposal stage of group g+1 (three count read-backs per group) runs beside
        # the CLIP stage of group g, fill and drain inside the timed region
        t = timed(make_pipe(g=gen_pc, fusion="G2L&L2G"), n_steps=6, cap=256, pool=pc_refs, group=2)
        also["PhraseCut"] = entry(t, 6, "PhraseCut-shaped item, run() in groups of 2 images: 480x640 image, heavy AMG (64x64 points, 1 crop layer, downscale 2, min "
                                        f"area 100, thresholds open, {PC_PPB} prompts per decoder launch: points_per_batch is a memory knob), <= 256 of SAM's masks into CLIP G2L&L2G, 8 phrases x (sentence + noun "
                                        "phrase + 1 other noun) + 8 GEM prompts")
        also["PhraseCut"]["unit"] = "images/s (8 phrases each)"
        # algorithmic work of one PhraseCut-shaped image: 5 encoder passes (image + 4 crops), 4096 + 4 x 1024 prompts
        # through the decoder, CLIP G2L&L2G (28 block evaluations per mask, minimal variant) on the <= 256 masks that go on,
        # 24 + 8 strings, one GEM tower pass
        g_ = CLIP_GEOM[args.clip]
        blk_ = 2.0 * g_["S"] * g_["D"] * 12 * g_["D"] + 4.0 * g_["S"] * g_["S"] * g_["D"]
        pc_fl = (5 * 5.961e12 + 8192 * 3.62e9 + 256 * (28 * blk_ + 2 * 2.0 * (g_["S"] - 1) * g_["patch_k"] * g_["D"])
                 + 32 * 12 * (2.0 * text_S * g_["text_D"] * 12 * g_["text_D"]) + (gem_flops_per_image(g_["gem_S"], g_["D"], g_["layers"], 6, g_["patch_k"], g_["embed"]) if use_gem else 0.0))
        also["PhraseCut"]["whole_step_algorithmic_tflops"] = pc_fl / t / 1e12
        also["PhraseCut"]["algorithmic_flops_per_image"] = pc_fl
        # the stage that carries this configuration: the mask decoder on 8192 prompts per image.  Timed alone here (PC_PPB prompts
        # per call, HIP events); its HBM bytes per prompt come from the committed counter pass (529 prompts per call)
        emb_ = torch.randn(4096, 256, device=dev)
        p01_ = torch.rand(PC_PPB, 2, device=dev)
        for _ in range(2):
            sam.decode_points(emb_, p01_)
        e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0_.record()
        for _ in range(4):
            sam.decode_points(emb_, p01_)
        e1_.record()
        torch.cuda.synchronize()
        dec_ms = e0_.elapsed_time(e1_) / 4
        dec = {"bound": "hbm / valu (see DESIGN.md section 5.4: dec_tail_kernel is bound by element-wise arithmetic, dec_i2t_kernel, the q "
                        "projection and the token -> image attention on the raw token planes by the bytes of the per-prompt image tokens)",
               "prompts_per_launch": PC_PPB, "ms_per_64_prompts": dec_ms * 64 / PC_PPB, "algorithmic_gflop_per_prompt": 3.62,
               "achieved": PC_PPB * 3.62e9 / (dec_ms * 1e-3) / 1e12, "unit": "TFLOP/s",
               "frac_of_fp16_mfma_peak": PC_PPB * 3.62e9 / (dec_ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS,
               "ms_per_image_at_8192_prompts": dec_ms * 8192 / PC_PPB}
        # HBM bytes per prompt: the newest tracked counter pass (profiles/r*_decoder_traffic.json, tools/decoder_traffic.py)
        import glob as _glob
        dpaths = sorted(_glob.glob(os.path.join(ROOT, "profiles", "r*_decoder_traffic.json")), reverse=True)
        if not dpaths:
            dec["bytes_source"] = "no profiles/r*_decoder_traffic.json in this checkout: bytes per prompt not reported"
        else:
            try:
                dj = json.load(open(dpaths[0]))
                dec["bytes_per_prompt"] = dj["bytes_per_prompt"]
                dec["TBps"] = dj["bytes_per_prompt"] * PC_PPB / (dec_ms * 1e-3) / 1e12
                dec["frac_of_hbm_peak"] = dec["TBps"] / PEAK_HBM_TBPS
                dec["bytes_source"] = (f"profiles/{os.path.basename(dpaths[0])} (" + dj.get("source", "") + "), replayed -- not measured in this run")
            except Exception as e:
                dec["bytes_source"] = f"profiles/{os.path.basename(dpaths[0])} unreadable: {e!r}"
        # the same call with the generator's IoU gate (hgl_sam_decode_points_gated) at the MEDIAN of the prompts' best
        # prediction: what a real pred_iou_thresh (0.86 in Hybridgl_main_PhraseCut.py:56-62) does to the decoder when about half
        # the prompts fail it -- random weights need the open filters of the leg above, so the threshold is placed, not given
        try:
            _, iou_ = sam.decode_points(emb_, p01_)
            thr_ = float(iou_.max(dim=1).values.median())
            for _ in range(2):
                sam.decode_points(emb_, p01_, iou_gate=thr_)
            e0_.record()
            for _ in range(4):
                sam.decode_points(emb_, p01_, iou_gate=thr_)
            e1_.record()
            torch.cuda.synchronize()
            gms = e0_.elapsed_time(e1_) / 4
            dec["iou_gate_at_median"] = {"ms_per_64_prompts": gms * 64 / PC_PPB, "ms_per_image_at_8192_prompts": gms * 8192 / PC_PPB,
                                         "prompts_skipping_the_upscaling": float((~(iou_ > thr_).any(dim=1)).float().mean()),
                                         "note": "candidates identical with the gate on and off (tests/test_gpu_sam.py::"
                                                 "test_decoder_iou_gate_leaves_the_candidates_unchanged)"}
        except Exception as e:
            dec["iou_gate_at_median"] = {"error": repr(e)[:200]}
        also["PhraseCut"]["decoder"] = dec
        del emb_, p01_
        del gen_pc, pc_refs
        torch.cuda.empty_cache()

    # ---- the evaluator's real feed: a REFER tree on disk through hybridgl_amd.main.evaluate (loader threads -> run())
    if also is not None and not args.no_disk:
        try:
            also["evaluator_from_disk"] = evaluator_from_disk(args, model, gen, gem_model, dev, nbatch, host_cores=host_cores_at_start)
        except Exception as e:      # the headline must not die with a secondary leg
            import traceback
            also["evaluator_from_disk"] = {"error": repr(e)[:400], "traceback": traceback.format_exc()[-1500:]}

    # ---- RCCL once on a 1-GPU box: the nccl branch of hybridgl_amd/dist.py in a world of one (device tensors through the
    # same two all-gathers + all-reduce the multi-GPU job uses); no process group is alive here at N = 1
    rccl = None
    if args.full and world == 1 and not args.no_rccl_check:
        try:
            rccl = D.rccl_selfcheck(dev, rows)
        except Exception as e:
            rccl = {"error": repr(e)}

    if rank == 0:
        total_refs = args.steps * world
        traffic, traffic_src = None, None
        pmc_table = None
        for cand in ("r03_pmc_traffic.json", "pmc_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", cand)
            if os.path.exists(tpath):
                break
        live = None
        if args.full and world == 1 and not args.no_live_pmc:
            if precision == "f16x3":
                live_prefix = "gemm_x3p_kernel<" if xg_ms > x_ms else "gemm_f16x3_kernel<"
            else:
                live_prefix = "gemm_f32_kernel<"
            torch.cuda.empty_cache()      # the child processes build their own models on this GPU
            pmc_table, pmc_note = live_pmc_table()
            live = live_pmc_traffic(pmc_table, pmc_note, live_prefix)
        if live is not None and live[0] is not None:
            traffic, traffic_src = live
        elif args.full and os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                # launch-weighted mean over the template instantiations of the dominant kernel
                if precision == "f16x3":
                    prefix = "gemm_x3p_kernel<" if xg_ms > x_ms else "gemm_f16x3_kernel<"
                else:
                    prefix = "gemm_f32_kernel<"
                num = den = 0.0
                for k, v in tj.items():
                    if k.startswith(prefix) and isinstance(v, dict):
                        n_l = max(float(v.get("launches_fetch_pass", 0)), 1.0)
                        num += n_l * float(v.get("hbm_bytes_per_launch", 0.0))
                        den += n_l
                traffic = num / den if den > 0 else None
                traffic_src = (f"profiles/{os.path.basename(tpath)}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this "
                               "command on an earlier box (tools/profile_round.sh), replayed here -- not measured in this run"
                               + (f" (live counter pass unavailable: {live[1]})" if live is not None else ""))
            except Exception:
                traffic = None
        workload = (f"RefCOCO-shaped ref (BASELINE configs[1]): 640x640 image, 3 queries x (sentence+noun phrase+1 other noun); "
                    + (("SAM ViT-H proposal stage (Pillow-exact resize to 1024 on the device, encoder, 8x8 point grid = 64 prompts x 3 "
                        "masks, fused post-processing of the 192 candidates, NMS; filters open) whose OWN masks feed the rest: the "
                        f"first {args.masks} survivors of every image -> connected-component clean-up (min area 800) + second NMS -> "
                        "counts read back (two device->host copies per group) -> " if dependent else
                        "SAM ViT-H proposal stage (encoder, 64 prompts x 3 masks, fused post-processing, NMS) whose noise masks "
                        "(random weights) are discarded; connected-component clean-up (min area 800) + second NMS run on the 64 "
                        "seeded proposal-shaped masks + ") if args.scope == "B" else "proposals given (scope A) + ")
                    + ("15x15 Gaussian blur (cv2 fixed-point) + " if args.blur == "device" else "")
                    + f"view synthesis + CLIP {args.clip} hybrid {args.fusion} (masking_block {geom['masking_block']}) on "
                    f"{args.masks} proposals + text encoder ({12 if use_gem else 9} strings) + "
                    + (f"GEM heat-map stage ({args.clip} at 448x448, self-self attention in the last 6 blocks, once "
                       "per image; 3 prompts -> 3 maps, antialiased resize to the image) + " if use_gem else "heat-maps given + ")
                    + "scoring tail + IoU"
                    + (f"; timed through HybridGLPipeline.run (the evaluator's loop, hybridgl_amd/main.py) in groups of at most {nbatch} "
                       f"images, equally full ({args.steps} refs = {-(-args.steps // HybridGLPipeline.balanced_group(args.steps, nbatch))} x "
                       f"{HybridGLPipeline.balanced_group(args.steps, nbatch)}): one SAM encoder pass over the images of group g+1 beside one text-encoder batch, one GEM tower "
                       "pass and one hybrid forward over the proposals of group g; pipeline fill and drain are inside the timed "
                       "region" if nbatch >= 2 else "; ref by ref (HybridGLPipeline.step)"))
        rec = {
            "metric": "images/sec (whole node)",
            "value": total_refs / dt,
            "unit": "images/s",
            "n_gpus": min(world, ngpu) if world > 1 else 1,
            "world_size_seen": dist.get_world_size() if dist is not None else 1,
            "backend": (args.backend + (" (RCCL)" if args.backend == "nccl" else "")) if world > 1 else None,
            "ranks_per_gpu": max(1, -(-world // max(ngpu, 1))),
            "host_cores_per_rank": len(cores) if cores else None,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if precision == "f32" else "f32 via fp16x3 split MFMA (fp32 accumulate)",
            "data": ("synthetic (seeded images/tokens; seeded random weights; proposals = SAM's own masks)" if dependent else
                     "synthetic (seeded images/masks/tokens; seeded random weights)"),
            "config": {
                "workload": workload,
                "scope": args.scope,
                "proposals_from": args.proposals_from if args.scope == "B" else "given",
                "heatmap": args.heatmap,
                "stage_overlap": bool(gen is not None and not args.no_overlap and nbatch >= 2),
                "sam_images_per_encoder_pass": HybridGLPipeline.balanced_group(args.steps, nbatch) if nbatch >= 2 else 1,
                "refs_per_clip_forward": HybridGLPipeline.balanced_group(args.steps, nbatch) if nbatch >= 2 else 1,
                "group_max": nbatch,
                "prepared": prepared,
                "host_syncs_per_group": (2 if dependent else 0) if nbatch >= 2 else None,
                "clip": args.clip,
                "fusion_mode": args.fusion, "proposals": args.masks, "image": "640x640", "queries": 3,
                "parallelism": f"image-parallel x{world}",
            },
            "precision": precision,
            "split_overflow_count": overflow,
            "metrics": m,
            "timed_region": timed_region,
        }
        if args.full:
            rec["roofline"] = roofline(precision, nprof, (g_n, g_ms, g_fl), (x_n, x_ms, x_fl), (a_n, a_ms, a_fl), traffic,
                                       algorithmic_flops_per_ref(args.masks, sam=args.scope == "B", gem=use_gem, clip_name=args.clip,
                                                                 text_S=max(r.token_len or 77 for r in refs)) / (dt / args.steps) / 1e12,
                                       xg=(xg_n, xg_ms, xg_fl), few=(fw_n, fw_ms, fw_fl))
            rec["roofline"]["traffic_source"] = traffic_src
            if pmc_table is not None:
                rec["roofline"]["hbm_kernels"] = hbm_kernel_table(pmc_table, tail_group=TAIL_GROUP_REFS)
        if also is not None:
            rec["also"] = also
        if rccl is not None:
            rec["rccl_selfcheck"] = rccl
        if args.full and world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(args.fusion, with_sam=args.scope == "B", with_gem=use_gem, clip_name=args.clip,
                                               host_cores=host_cores_at_start)
        os.write(real_stdout, (json.dumps(rec) + "\n").encode())
    if world > 1:
        dist.destroy_process_group()
    if overflow:
        raise SystemExit(f"bench.py: {overflow} GPU threads met activations beyond the fp16 range in f16x3 mode: the numbers above "
                         "are void; rerun with HYBRIDGL_PRECISION=f32")


if __name__ == "__main__":
    main()
