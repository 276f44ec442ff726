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

  decode     (--decode, instead of the legs above) the way back: ops.rle_decode for 64 and for 6 blob masks of 640 x 640 and
             ops.rle_iou for 64 pairs (HIP events, median of --reps after warm-up), the decoder's time against ONE streaming
             write of the S*H*W output bytes (a fill of the same buffer, timed the same way), and the host wall time of the
             path it replaces: sam.rle_to_mask per mask plus the upload, both sides ending in a synchronise; writes
             profiles/rle_decode_bench.json as well

  match      (--match, instead of the legs above) every mask of one set against every mask of another: ops.rle_match for
             64 x 64 masks of 640 x 640 (a RefCOCO image) and for 512 x 512 (a heavy-AMG image), against what a caller had to
             do before the entry existed: replicate both sets into the Sa*Sb-long pair list and run ops.rle_iou over it, in
             chunks within its S*H*W < 2^31 limit (HIP events, median of --reps after warm-up; the pair list's time with and
             without the replication); writes profiles/rle_match_bench.json as well

  polygons   (--polygons, instead of the legs above) ground truth from polygons: ONE ops.rle_from_polygons call for 64 entries of
             480 x 640 -- the golden 40-gon scaled and shifted per entry, plus a small triangle -- as host wall time (pack, copy,
             kernel, synchronise) and as the kernel alone (HIP events), against the path it replaces: refer_io.gt_mask_from_polygons
             per entry + loader.pin_upload + ops.rle_encode, wall time to the synchronise; and the wall time of
             `python -m hybridgl_amd.main --proposal_ceiling` with and without --device_targets on a synthetic on-disk REFER
             tree (hybridgl_amd.synth.write_refer_tree, as tools/evaluator_ranks.py) with a seeded proposal store; writes
             profiles/rle_polygons_bench.json as well

  merge      (--merge, instead of the legs above) new masks out of encoded masks: ONE ops.rle_merge call against the pixel path
             built from the existing entries (ops.rle_decode -> torch sum and compare -> ops.rle_encode), both from packed runs
             to the encoder's slots, HIP events: the majority of 3 runs x 2 masks x 128 sentences of 640 x 640, and the union of
             64 proposals per image for 16 images of 640 x 640; equality of the two paths is checked before any timing; writes
             profiles/rle_merge_bench.json as well

  nms        (--nms, instead of the legs above) a proposal set thinned by mask overlap: ONE ops.rle_nms call for 16 images of
             640 x 640 with 64 and with 256 proposals each (IoU, thr 0.7, scored), as the kernels alone (HIP events) and as host
             wall time to the kept lists on the host, against what the product offered before the entry existed: the
             ops.rle_match matrix of the set against itself read back and walked in numpy (wall time, and its device part
             alone); equality of the two paths is checked before any timing; writes profiles/rle_nms_bench.json as well

  select     (--select, instead of the legs above) the kept entries of that set compacted on the device: ONE ops.rle_select call
             on the workload of --nms, driven by the NMS result with two side columns, (a) as the kernels alone (HIP events
             behind a 256 MB copy that keeps the device busy while the host enqueues: two launches of a few microseconds are
             otherwise timed at the host's pace) against a plain device-to-device copy of the set's bytes timed the same way, and (b) as wall time from the uploaded set to compacted
             slots ready for the decode (ops.rle_nms + ops.rle_select) against what there was before the entry: ops.rle_nms,
             the kept lists read back, the kept rows re-packed with numpy and uploaded; equality of the two paths is checked
             before any timing; writes profiles/rle_select_bench.json as well

  clean      (--clean, instead of the legs above) a stored set re-tuned to another min_mask_region_area: ONE
             ops.rle_remove_small_regions call (mode both, area 100) for 64 entries of 640 x 640 -- blobs with a handful of small
             islands and holes each, packed runs as a store holds them -- against the pixel path built from the existing entries
             (ops.rle_decode_group -> sam.remove_small_regions holes -> sam.remove_small_regions_boxes islands -> ops.rle_encode),
             outputs pre-allocated on both sides, HIP events, three alternating rounds; the workspace bytes of either path;
             equality of the two paths is checked before any timing; writes profiles/rle_clean_bench.json as well

--strings    COCO's compressed strings on the device (ops.rle_to_strings / ops.rle_from_strings) against the host codec one record
             at a time, on the benchmark's 64 seeded masks of 640 x 640: (a) wall time from the encoded set on the device to
             finished Python strings, (b) from Python strings to slots / table on the device, (c) the kernels alone under HIP
             events, (d) minimum, median and maximum string length per mask; medians of --reps repetitions, the two paths
             alternated; equality of the two paths is checked before any timing; writes profiles/rle_strings_bench.json as well

--paint      pictures of encoded masks (ops.rle_paint) for 64 images of 480 x 640 with 64 stored proposals each: one winner per image
             in the demo's style, then every proposal of every image in palette style with outlines, largest first; (a) the
             kernels alone under HIP events (the list already on the device), (b) the wall time of the call itself and of the call
             to finished pictures, against the path it replaces: sam.rles_to_masks of the listed entries, the masks to the host,
             the blend in numpy, the pictures uploaded (all 64 images for the winners, 2 images for the proposals, per image);
             medians of --reps repetitions; equality of the two paths is checked before any timing; writes
             profiles/rle_paint_bench.json as well

    python tools/rle_bench.py [--reps 30] [--evaluator --steps 64]
    python tools/rle_bench.py --paint [--reps 30]
    python tools/rle_bench.py --strings [--reps 30]
    python tools/rle_bench.py --decode [--reps 30]
    python tools/rle_bench.py --match [--reps 30]
    python tools/rle_bench.py --polygons [--reps 30] [--cli_images 100]
    python tools/rle_bench.py --merge [--reps 30]
    python tools/rle_bench.py --nms [--reps 30]
    python tools/rle_bench.py --select [--reps 20]
    python tools/rle_bench.py --clean [--reps 30]
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

from hybridgl_amd import _lib, ops, synth
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
        flat = torch.empty(ops.rle_block_words("set", S, sw), dtype=torch.int32, device=dev)
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


def decode_leg(masks, reps):
    """masks: [64,H,W] uint8 blobs on the device.  The inputs of the decoder are the runs as a saved set holds them: packed
    counts (ops.rle_pack), form 0."""
    N, H, W = masks.shape
    dev = masks.device
    rles = hsam.masks_to_rle(masks)
    host = masks.cpu().numpy()
    rec = {"H": H, "W": W, "counts_per_mask_max": max(len(r["counts"]) for r in rles)}
    for name, S in (("64_masks", 64), ("6_masks", 6)):
        part = rles[:S]
        slots, table = ops.rle_pack([r["counts"] for r in part], H, W, device=dev)
        out = torch.empty(S * H * W, dtype=torch.uint8, device=dev)
        got, status = ops.rle_decode(slots, table, H, W, out=out)
        assert np.array_equal(got.cpu().numpy(), host[:S]) and not status[:, 0].any()
        us = device_us(lambda: ops.rle_decode(slots, table, H, W, out=out), reps)
        us_fill = device_us(lambda: out.fill_(1), reps)      # the yardstick: one streaming write of the output bytes
        nbytes = S * H * W

        def host_path():
            up = [torch.from_numpy(hsam.rle_to_mask(r)).to(dev) for r in part]
            torch.cuda.synchronize()
            return up

        def device_path():
            m = hsam.rles_to_masks(part, device=dev)      # pack + copy + decode + the status read-back (a synchronise)
            torch.cuda.synchronize()
            return m

        h, d = host_ms(host_path, max(3, reps // 3)), host_ms(device_path, max(3, reps // 3))
        rec[name] = {"entries": S, "output_bytes": nbytes, "slot_words": int(slots.shape[1]), "input_bytes": int(slots.numel() * 4),
                     "rle_decode_us": round(us, 1), "TBps_of_one_write": round(nbytes / us / 1e6, 3), "fill_same_bytes_us": round(us_fill, 1),
                     "fill_TBps": round(nbytes / us_fill / 1e6, 3), "time_over_streaming_write": round(us / us_fill, 2),
                     "host_decode_and_upload_ms": round(h, 2), "rles_to_masks_ms": round(d, 2), "host_over_device_wall": round(h / d, 2),
                     "host_over_decode_kernels": round(h * 1e3 / us, 1)}
    a_s, a_t = ops.rle_pack([r["counts"] for r in rles], H, W, device=dev)
    b_s, b_t = ops.rle_pack([r["counts"] for r in rles[1:] + rles[:1]], H, W, device=dev)
    iu = ops.rle_iou(a_s, a_t, b_s, b_t, H, W).cpu().numpy()
    hb = np.roll(host, -1, axis=0)
    assert iu.tolist() == [[int((x & y).sum()), int((x | y).sum())] for x, y in zip(host, hb)]
    us = device_us(lambda: ops.rle_iou(a_s, a_t, b_s, b_t, H, W), reps)
    da, db = masks, torch.roll(masks, -1, 0).contiguous()
    us_bytes = device_us(lambda: [ops.iou_counts(da[i], db[i]) for i in range(N)], reps)
    rec["iou_64_pairs"] = {"entries": N, "rle_iou_us": round(us, 1), "hgl_iou_on_bytes_64_launches_us": round(us_bytes, 1),
                           "mask_bytes_never_formed": 2 * N * H * W}
    return rec


def blobs(n, H, W, seed):
    """seeded unions of ellipses, as the tests' blobs"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, ry, rx = rng.random() * H, rng.random() * W, (0.05 + 0.3 * rng.random()) * H, (0.05 + 0.3 * rng.random()) * W
            out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
    return out


def match_leg(dev, reps, H=640, W=640):
    """both sets are runs as a store holds them: packed counts (ops.rle_pack), form 0"""
    rec = {"H": H, "W": W}
    limit = ((1 << 31) - 1) // (H * W)      # entries per ops.rle_iou call
    for name, n in (("64x64", 64), ("512x512", 512)):
        sets = []
        for seed in (11, 12):
            runs = []
            for at in range(0, n, 64):      # 64 masks at a time through the device encoder
                m = torch.from_numpy(blobs(min(64, n - at), H, W, 1000 * seed + at)).to(dev)
                runs += [r["counts"] for r in hsam.masks_to_rle(m)]
            sets.append(ops.rle_pack(runs, H, W, device=dev))
        (sa, ta), (sb, tb) = sets
        inter, ma, mb = ops.rle_match(sa, ta, sb, tb, [(H, W)], [n], [n])
        us = device_us(lambda: ops.rle_match(sa, ta, sb, tb, [(H, W)], [n], [n]), reps)
        us_nomatrix = device_us(lambda: ops.rle_match(sa, ta, sb, tb, [(H, W)], [n], [n], matrix=False), reps)
        rows = max(1, min(n, limit // n))      # rows of the matrix per pair-list chunk
        ib = torch.arange(n, device=dev).repeat(rows)

        def pair_list(keep=None, held=None):
            """held: a dict that keeps the replicated chunks from call to call (the rle_iou calls alone); None: replicate anew"""
            for a0 in range(0, n, rows):
                k = min(rows, n - a0)
                part = None if held is None else held.get(a0)
                if part is None:
                    ia = torch.arange(a0, a0 + k, device=dev).repeat_interleave(n)
                    part = (sa[ia].contiguous(), ta[ia].contiguous(), sb[ib[:k * n]].contiguous(), tb[ib[:k * n]].contiguous())
                    if held is not None:
                        held[a0] = part
                iu = ops.rle_iou(*part, H, W)
                if keep is not None:
                    keep.append(iu[:, 0].reshape(k, n))

        got = []
        pair_list(got)
        assert torch.equal(torch.cat(got).to(torch.int32), inter[0]), "the pair list and the entry disagree"
        r2 = max(3, reps // 5)
        us_pairs = device_us(lambda: pair_list(), r2, warm=2)
        held = {}
        us_pairs_kernels = device_us(lambda: pair_list(held=held), r2, warm=2)
        rec[name] = {"masks_a": n, "masks_b": n, "pairs": n * n, "slot_words": [int(sa.shape[1]), int(sb.shape[1])],
                     "rle_match_us": round(us, 1), "rle_match_no_matrix_us": round(us_nomatrix, 1),
                     "pair_list_chunks": (n + rows - 1) // rows, "pair_list_us": round(us_pairs, 1),
                     "pair_list_rle_iou_only_us": round(us_pairs_kernels, 1), "pair_list_over_match": round(us_pairs / us, 1),
                     "rle_iou_only_over_match": round(us_pairs_kernels / us, 1)}
    return rec


def device_spread(fn, reps, warm=5):
    """median, fastest and slowest of `reps` HIP-event timings in microseconds, after `warm` calls"""
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
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def merge_leg(dev, reps, H=640, W=640):
    """sources are runs as saved predictions and stores hold them: packed counts (ops.rle_pack), form 0"""
    reps = max(reps, 20)
    base = torch.from_numpy(blobs(64, H, W, 4100)).to(dev)
    runs = [r["counts"] for r in hsam.masks_to_rle(base)]
    sw = ops.rle_slot_words(H, W)
    rec = {"H": H, "W": W, "reps": reps, "merged_plane": "materialised once in the workspace"}
    shapes = {
        # 128 sentences x (pure, final), three runs each: output e votes sources 3e .. 3e+2 (neighbouring blobs: runs that mostly agree)
        "majority_3_runs_2_masks_128_sentences": (256, 3, "majority", lambda e, i: (e + 7 * i) % 64),
        # 16 images, the union of each one's 64 proposals
        "union_64_proposals_16_images": (16, 64, "union", lambda e, i: (5 * e + i) % 64),
    }
    for name, (S, k, rule, pick) in shapes.items():
        slots, table = ops.rle_pack([runs[pick(e, i)] for e in range(S) for i in range(k)], H, W, device=dev)
        members = torch.arange(S * k, dtype=torch.int32, device=dev)
        offsets = torch.arange(0, S * k + 1, k, dtype=torch.int32, device=dev)
        lo, hi = ops.rle_merge_rule(rule, k)
        bounds = torch.tensor([[lo, hi]] * S, dtype=torch.int32, device=dev)
        out_m = torch.empty(ops.rle_block_words("status", S, sw), dtype=torch.int32, device=dev)
        out_p = torch.empty(ops.rle_block_words("set", S, sw), dtype=torch.int32, device=dev)
        pix = torch.empty(S * k * H * W, dtype=torch.uint8, device=dev)

        def entry():
            return ops.rle_merge(slots, table, [(H, W)], [S * k], members, offsets, bounds, [S], slot_words=sw, out=out_m)

        def pixels():
            dec, _ = ops.rle_decode(slots, table, H, W, out=pix)
            count = dec.view(S, k, H, W).sum(dim=1, dtype=torch.int32)
            return ops.rle_encode(((count >= lo) & (count <= hi)).to(torch.uint8), slot_words=sw, out=out_p)

        ms, mt, st = entry()
        ps, pt = pixels()
        n = int(pt[:, 0].max())
        assert int(st[:, 0].abs().sum()) == 0 and torch.equal(mt, pt) and int(pt[:, 1].abs().sum()) == 0 and torch.equal(ms[:, :n], ps[:, :n]), \
            "the entry and the pixel path disagree"
        a, b = device_spread(entry, reps), device_spread(pixels, reps)
        rec[name] = {"sources": S * k, "outputs": S, "members_per_output": k, "rule": rule, "source_slot_words": int(slots.shape[1]),
                     "counts_per_output_max": n, "rle_merge": a, "decode_vote_encode": b,
                     "pixel_path_over_entry": round(b["median_us"] / a["median_us"], 2)}
    return rec


def nms_leg(dev, reps, H=640, W=640, G=16, thr=0.7):
    """the lists are runs as a store holds them: packed counts (ops.rle_pack), form 0; image g holds the same 256 seeded blobs
    in an order and with scores of its own"""
    rec = {"H": H, "W": W, "images": G, "thr": thr, "metric": "iou", "reps": reps}
    base = []
    for at in range(0, 256, 64):
        base += [r["counts"] for r in hsam.masks_to_rle(torch.from_numpy(blobs(64, H, W, 7000 + at)).to(dev))]
    rng = np.random.default_rng(5)
    for n in (64, 256):
        picks = [rng.permutation(256)[:n] for _ in range(G)]
        slots, table = ops.rle_pack([base[int(i)] for p in picks for i in p], H, W, device=dev)
        scores_h = rng.random(G * n).astype(np.float32)
        scores = torch.from_numpy(scores_h).to(dev)
        sizes, counts = [(H, W)] * G, [n] * G

        def entry():
            return ops.rle_nms(slots, table, sizes, counts, scores, thr, "iou")

        def entry_host():
            out_idx, out_n, _ = entry()
            out_idx, out_n = out_idx.cpu().numpy(), out_n.cpu().numpy()
            return [out_idx[g * n:g * n + int(out_n[g])].tolist() for g in range(G)]

        def matrix():
            return ops.rle_match(slots, table, slots, table, sizes, counts, counts)

        def matrix_walk():
            inter, ma, _ = matrix()
            area = ma[:, 1].cpu().numpy().astype(np.int64)
            kept = []
            for g in range(G):
                I = inter[g].cpu().numpy().astype(np.int64)
                a = area[g * n:(g + 1) * n]
                order = np.lexsort((np.arange(n), -scores_h[g * n:(g + 1) * n].astype(np.float64)))
                I, a = I[order][:, order], a[order]
                U = a[:, None] + a[None, :] - I
                over = (I > 0) & (I.astype(np.float64) / np.maximum(U, 1).astype(np.float64) > thr)
                gone = np.zeros(n, bool)
                mine = []
                for i in range(n):
                    if not gone[i]:
                        mine.append(int(order[i]))
                        gone[i + 1:] |= over[i, i + 1:]
                kept.append(mine)
            return kept

        a, b = entry_host(), matrix_walk()
        assert a == b, "the entry and the matrix walk disagree"
        rec[f"{n}_proposals"] = {"entries": G * n, "kept": sum(len(k) for k in a), "slot_words": int(slots.shape[1]),
                                 "rle_nms": device_spread(entry, reps), "rle_nms_to_host_ms": round(host_ms(entry_host, reps), 3),
                                 "rle_match_matrix": device_spread(matrix, reps),
                                 "matrix_read_back_and_numpy_walk_ms": round(host_ms(matrix_walk, max(3, reps // 3)), 3)}
        r = rec[f"{n}_proposals"]
        r["host_path_over_entry"] = round(r["matrix_read_back_and_numpy_walk_ms"] / r["rle_nms_to_host_ms"], 2)
    return rec


def device_spread_behind(fn, reps, head, warm=5):
    """device_spread for a call of a few microseconds: `head` -- device work of some hundred microseconds -- is enqueued in front
    of the first event, so the host has enqueued fn and the second event before the device reaches the first, and the interval
    holds the kernels of fn back to back, not the host's pace of launching them"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        head()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def select_leg(dev, reps, H=640, W=640, G=16, thr=0.7):
    """the workload of nms_leg; the NMS result of the set is computed once and held on the device for (a)"""
    rec = {"H": H, "W": W, "images": G, "thr": thr, "metric": "iou", "reps": reps}
    base = []
    for at in range(0, 256, 64):
        base += [r["counts"] for r in hsam.masks_to_rle(torch.from_numpy(blobs(64, H, W, 7000 + at)).to(dev))]
    rng = np.random.default_rng(5)
    ballast = torch.empty((2, 1 << 28), dtype=torch.uint8, device=dev)      # a 256 MB copy: the device's work while the host enqueues

    def head():
        ballast[1].copy_(ballast[0])

    for n in (64, 256):
        picks = [rng.permutation(256)[:n] for _ in range(G)]
        slots, table = ops.rle_pack([base[int(i)] for p in picks for i in p], H, W, device=dev)
        S, sw = int(slots.shape[0]), int(slots.shape[1])
        scores = torch.from_numpy(rng.random(G * n).astype(np.float32)).to(dev)
        cols = torch.stack([scores, 1 - scores]).contiguous()
        sizes, counts = [(H, W)] * G, [n] * G
        slots_h, table_h = slots.cpu().numpy(), table.cpu().numpy()      # the host's copy: it packed the set
        result = ops.rle_nms(slots, table, sizes, counts, scores, thr, "iou")[2]
        out = torch.empty(ops.rle_block_words("select", S, sw, C=2), dtype=torch.int32, device=dev)
        back = torch.empty(ops.rle_block_words("back", S, G=G), dtype=torch.int32, device=dev)

        def select():
            return ops.rle_select(slots, table, sizes, counts, nms_result=result, cols=cols, out=out, back=back)

        whole = torch.cat([table.reshape(-1), slots.reshape(-1)])      # the set's bytes, table and slots
        twin = torch.empty_like(whole)

        def copy():
            twin.copy_(whole)

        def entry_path():
            """uploaded set -> compacted slots ready for the decode, all on the device"""
            res = ops.rle_nms(slots, table, sizes, counts, scores, thr, "iou")[2]
            o = ops.rle_select(slots, table, sizes, counts, nms_result=res, cols=cols, out=out, back=back)
            torch.cuda.synchronize()
            return o

        def host_path():
            """what there was before the entry: the kept lists read back, the kept rows re-packed with numpy, uploaded"""
            out_idx, out_n, _ = ops.rle_nms(slots, table, sizes, counts, scores, thr, "iou")
            out_idx, out_n = out_idx.cpu().numpy(), out_n.cpu().numpy()
            rows = np.concatenate([g * n + np.sort(out_idx[g * n:g * n + int(out_n[g])]) for g in range(G)])
            flat = torch.from_numpy(np.concatenate([table_h[rows].reshape(-1), slots_h[rows].reshape(-1)])).pin_memory()
            d = flat.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return rows, ops.rle_split(d, len(rows), sw), [int(v) for v in out_n]

        cs, ct, cc, src, k = (x.cpu().numpy() for x in entry_path())
        rows, (hs, ht), kept = host_path()
        hs, ht = hs.cpu().numpy(), ht.cpu().numpy()
        assert k.tolist() == kept, "the entry and the host path keep different counts"
        at = 0
        for g in range(G):      # the survivors' rows, and the words their rows define, are those of the host's gather
            e, kg = g * n, kept[g]
            assert np.array_equal(src[e:e + kg] + e, rows[at:at + kg]) and np.array_equal(ct[e:e + kg], ht[at:at + kg])
            for p in range(kg):
                w = int(ct[e + p, 0])
                assert np.array_equal(cs[e + p, :w], hs[at + p, :w])
            assert (src[e + kg:e + n] == -1).all() and (ct[e + kg:e + n] == (1, 0, 0, 0)).all() and (cs[e + kg:e + n, 0] == H * W).all()
            at += kg
        moved = int(ct[src >= 0][:, 0].sum()) + 4 * int((src >= 0).sum())
        r = {"entries": S, "kept": int(k.sum()), "slot_words": sw, "set_bytes": int(whole.numel()) * 4, "words_moved": moved,
             "rle_select": device_spread_behind(select, reps, head), "device_copy_of_the_set": device_spread_behind(copy, reps, head),
             "rle_select_at_the_hosts_pace": device_spread(select, reps),
             "nms_select_to_ready_ms": round(host_ms(entry_path, reps), 3),
             "nms_read_back_numpy_repack_upload_ms": round(host_ms(host_path, reps), 3)}
        r["select_over_copy"] = round(r["rle_select"]["median_us"] / r["device_copy_of_the_set"]["median_us"], 2)
        r["host_path_over_entry"] = round(r["nms_read_back_numpy_repack_upload_ms"] / r["nms_select_to_ready_ms"], 2)
        rec[f"{n}_proposals"] = r
    return rec


def clean_leg(dev, reps, H=640, W=640, S=64, area=100):
    """ops.rle_remove_small_regions (mode both) against the pixel path -- rle_decode_group -> remove_small_regions holes ->
    remove_small_regions_boxes islands -> rle_encode -- on S entries as a store holds them: packed counts (ops.rle_pack), form 0,
    blobs with a handful of small islands and holes each.  Outputs pre-allocated on both sides; the workspace of either path in
    bytes: what the entry's query states, and for the pixel path the three [S,H,W] byte arrays, the union-find planes of the
    clean-up and the planes of the decoder and the encoder."""
    from hybridgl_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(31)
    m = blobs(S, H, W, 29)
    for i in range(S):      # speckle: 12 islands and 12 holes of 1 .. 40 pixels
        for _ in range(24):
            y, x, h, w = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
            m[i, y:y + h, x:x + w] ^= 1
    rles = [hsam.mask_to_rle(k)["counts"] for k in m]
    slots, table = ops.rle_pack(rles, H, W, device=dev)
    sw = int(slots.shape[1])
    cap = sw // 2 + W + 1
    osw = ops.rle_slot_words(H, W)
    sizes, counts = [(H, W)], [S]
    out = torch.empty(ops.rle_block_words("clean", S, osw), dtype=torch.int32, device=dev)
    run_new = lambda: ops.rle_remove_small_regions(slots, table, sizes, counts, area, "both", seg_cap=cap, slot_words=osw, out=out)
    pix = torch.empty(S * H * W, dtype=torch.uint8, device=dev)
    aux = torch.empty((2, S, 4), dtype=torch.int32, device=dev)
    m1, m2 = torch.empty((S, H, W), dtype=torch.uint8, device=dev), torch.empty((S, H, W), dtype=torch.uint8, device=dev)
    c1, c2 = torch.empty(S, dtype=torch.uint8, device=dev), torch.empty(S, dtype=torch.uint8, device=dev)
    nb = torch.empty((S, 4), dtype=torch.int32, device=dev)
    enc = torch.empty(ops.rle_block_words("set", S, osw), dtype=torch.int32, device=dev)

    def run_pixels():
        masks, _, _ = ops.rle_decode_group(slots, table, sizes, counts, out=pix, aux=aux)
        hsam.remove_small_regions(masks[0], area, "holes", out=(m1, c1))
        hsam.remove_small_regions_boxes(m1, area, "islands", out=(m2, c2, nb))
        return ops.rle_encode(m2, slot_words=osw, out=enc)

    s_new, t_new, b_new, r_new = run_new()
    s_pix, t_pix = run_pixels()
    torch.cuda.synchronize()
    assert torch.equal(t_new, t_pix) and torch.equal(b_new, nb) and torch.equal(r_new[:, 2], (c1 | (c2 << 1)).to(torch.int32))
    n_counts = t_new[:, 0].cpu().numpy()
    for i in range(S):
        assert torch.equal(s_new[i, :n_counts[i]], s_pix[i, :n_counts[i]])
    images = ops.rle_clean_layout(sizes, counts)
    ws_new = int(lib.hgl_rle_clean_workspace_bytes(images.ctypes.data, 1, S, sw, cap))
    ws_pix = (3 * S * H * W + int(lib.hgl_remove_small_regions_workspace_bytes(S, H, W)) + int(lib.hgl_rle_decode_group_workspace_bytes(S, sw))
              + int(lib.hgl_rle_encode_workspace_bytes(S, H, W)))
    rounds = [(device_spread(run_new, reps), device_spread(run_pixels, reps)) for _ in range(3)]      # alternating: the spread between rounds shows
    new, old = rounds[1]      # the middle round stands; all three are reported
    return {"S": S, "H": H, "W": W, "area_thresh": area, "slot_words": sw, "seg_cap": cap, "changed": int((r_new[:, 2] != 0).sum()),
            "rle_clean": new, "pixel_path": old, "ratio_pixel_over_clean": round(old["median_us"] / new["median_us"], 2),
            "workspace_bytes_rle_clean": ws_new, "workspace_bytes_pixel_path": ws_pix,
            "workspace_ratio_pixel_over_clean": round(ws_pix / ws_new, 2),
            "rounds_median_us": [[r[0]["median_us"], r[1]["median_us"]] for r in rounds]}


def alternated_ms(fa, fb, reps, warm=3):
    """the median wall times (ms) of two paths run in turn, each from a quiet device"""
    for _ in range(warm):
        fa(), fb()
    out = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for v in out]


def strings_leg(dev, reps, S=64, H=640, W=640):
    """the two ends of an encoded set's life, host path against device path (see --strings at the top)"""
    masks = torch.from_numpy(np.ascontiguousarray(synth.synth_masks(S, H, W, 2000))).to(dev).view(torch.uint8)
    sw = ops.rle_slot_words(H, W)
    flat = torch.empty(ops.rle_block_words("set", S, sw), dtype=torch.int32, device=dev)
    slots, table = ops.rle_encode(masks, None, sw, out=flat)

    def out_host():      # what ProposalRecorder and generate() do today: the whole set over the bus, a Python list per mask, ctypes per mask
        s, t = ops.rle_split(flat.cpu().numpy(), S, sw)
        return [hsam.coco_encode_rle({"size": [H, W], "counts": hsam.rle_from_slot(s[i], int(t[i, 0]), int(t[i, 1]), H, W)})["counts"]
                for i in range(S)]

    def out_device():
        return [b.decode("ascii") for b in hsam.strings_from_device(slots, table, H, W)]

    strings = out_host()
    assert out_device() == strings
    lengths = [len(x) for x in strings]
    n_counts = table[:, 0].cpu().numpy()

    def in_host():       # what StoredProposals._load + rle_pack do today
        return ops.rle_pack([hsam.rle_counts_from_string(x) for x in strings], H, W, device=dev)

    def in_device():
        buf, _, n = ops.rle_strings_pack(strings)
        d = buf.to(dev, non_blocking=True)
        return ops.rle_from_strings(d[8 * (S + 1):], d[:8 * (S + 1)].view(torch.int64), S, max(int(n.max()), 1))[:2]

    (hs, ht), (ds, dt) = in_host(), in_device()
    torch.cuda.synchronize()
    assert torch.equal(ht, dt) and hs.shape == ds.shape
    for i in range(S):
        assert torch.equal(hs[i, :n_counts[i]], ds[i, :n_counts[i]])
    out_t = alternated_ms(out_host, out_device, reps)
    in_t = alternated_ms(in_host, in_device, reps)
    cap = ops.RLE_STRING_CAP_PER_ENTRY * S
    sbuf = torch.empty(ops.rle_strings_bytes(S, cap), dtype=torch.uint8, device=dev)
    data, offsets, _ = ops.rle_to_strings(slots, table, cap, out=sbuf)
    back = torch.empty(ops.rle_block_words("set", S, int(ds.shape[1])), dtype=torch.int32, device=dev)
    total = int(offsets[S])
    k_out = device_spread(lambda: ops.rle_to_strings(slots, table, cap, out=sbuf), reps)
    k_in = device_spread(lambda: ops.rle_from_strings(data[:total], offsets, S, int(ds.shape[1]), out=back), reps)
    return {"S": S, "H": H, "W": W, "slot_words": sw, "counts_per_mask": {"min": int(n_counts.min()), "median": float(np.median(n_counts)),
                                                                         "max": int(n_counts.max())},
            "string_bytes_per_mask": {"min": min(lengths), "median": float(statistics.median(lengths)), "max": max(lengths)},
            "string_bytes_total": total, "default_cap_bytes": cap, "bytes_per_count": round(total / float(n_counts.sum()), 3),
            "bus_bytes_host_path_out": 4 * ops.rle_block_words("set", S, sw), "bus_bytes_device_path_out": ops.rle_strings_bytes(S, 0) + total,
            "to_python_strings_host_path": out_t[0], "to_python_strings_device_path": out_t[1],
            "ratio_out_host_over_device": round(out_t[0]["median_ms"] / out_t[1]["median_ms"], 2),
            "from_python_strings_host_path": in_t[0], "from_python_strings_device_path": in_t[1],
            "ratio_in_host_over_device": round(in_t[0]["median_ms"] / in_t[1]["median_ms"], 2),
            "kernels_rle_to_strings": k_out, "kernel_rle_from_strings": k_in}


def paint_leg(dev, reps, G=64, H=480, W=640, N=64, host_images=2):
    """pictures of encoded masks, device path against host path (see --paint at the top)"""
    from hybridgl_amd import render
    SW = 4096
    f32 = np.float32
    shapes = blobs(N, H, W, 7)
    slots1, table1 = ops.rle_encode(torch.from_numpy(shapes).to(dev), None, SW)      # three ellipses: at most 6 W + 1 counts
    assert int(table1[:, 1].max()) == 0
    slots, table = slots1.repeat(G, 1), table1.repeat(G, 1)                              # every image owns N entries
    sizes, counts = [(H, W)] * G, [N] * G
    base = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (G * H * W * 3,), dtype=np.uint8)).to(dev)
    out = torch.empty_like(base)
    area = table1[:, 2].cpu().numpy()
    legs = {"winner": (np.array([(5 * g) % N for g in range(G)], np.int32), [1] * G, ops.rle_paint_style(**render.DEMO_STYLE)[None].repeat(G, 0)),
            "all_proposals": (np.tile(np.argsort(-area, kind="stable").astype(np.int32), G), [N] * G, np.tile(render.proposal_styles(N), (G, 1)))}
    host_counts = hsam.counts_from_set(*ops.rle_split(torch.cat([table1.reshape(-1), slots1.reshape(-1)]).cpu().numpy(), N, SW), H, W)

    def edge(m):
        p = np.zeros((H + 2, W + 2), bool)
        p[1:-1, 1:-1] = m
        return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])

    def host_path(order, order_counts, style, images):
        """what a caller had before the entry: the listed masks to pixels (sam.rles_to_masks), to the host, the blend in numpy,
        the pictures uploaded"""
        k, pics = 0, []
        for g in range(images):
            ks = range(k, k + order_counts[g])
            k += order_counts[g]
            m = hsam.rles_to_masks([{"size": [H, W], "counts": host_counts[int(order[t])]} for t in ks], dev).cpu().numpy().astype(bool)
            img = base[g * H * W * 3:(g + 1) * H * W * 3].view(H, W, 3).cpu().numpy().copy()
            for t, mask in zip(ks, m):
                w0, a, b, w3 = int(style[t, 0]), style[t, 1:2].view(f32)[0], style[t, 2:3].view(f32)[0], int(style[t, 3])
                if w0 & ops.PAINT_FILL:
                    col = np.array([(w0 >> 16) & 255, (w0 >> 8) & 255, w0 & 255], f32)
                    img[mask] = np.clip(np.rint(img[mask].astype(f32) * a + col * b), 0, 255).astype(np.uint8)
                if w0 & ops.PAINT_OUTLINE:
                    img[edge(mask)] = [(w3 >> 16) & 255, (w3 >> 8) & 255, w3 & 255]
            pics.append(torch.from_numpy(img).to(dev))
        torch.cuda.synchronize()
        return pics

    rec = {"G": G, "H": H, "W": W, "proposals_per_image": N, "slot_words": SW, "reps": reps}
    for name, (order, oc, style) in legs.items():
        d_order, d_style = torch.from_numpy(order).to(dev), torch.from_numpy(style.view(np.int32).copy()).to(dev)
        call = lambda: ops.rle_paint(slots, table, sizes, counts, order, oc, style, base=base, out=out)
        pics = call()[0]
        want = host_path(order, oc, style, host_images)
        torch.cuda.synchronize()
        assert all(torch.equal(p, w) for p, w in zip(pics, want)), name      # the two paths paint the same bytes
        kernels = device_spread(lambda: ops.rle_paint(slots, table, sizes, counts, d_order, oc, d_style, base=base, out=out), reps)
        wall = host_ms(call, reps)                                                        # the call itself: asynchronous
        done = host_ms(lambda: (call(), torch.cuda.synchronize()), reps)                  # ... to finished pictures on the device
        n_host = host_images if name == "all_proposals" else G
        t_host = host_ms(lambda: host_path(order, oc, style, n_host), min(reps, 5), warm=1)
        K = int(sum(oc))
        rows = ops.rle_paint_layout(sizes, counts, oc)[0]      # kept alive across the call: the library reads it through the pointer
        need = _lib.load().hgl_rle_paint_workspace_bytes(rows.ctypes.data, G, G * N, SW, K, G * H * W)
        rec[name] = {"list_positions": K, "kernels": kernels, "call_ms": round(wall, 4), "call_and_sync_ms": round(done, 4),
                     "host_path_images": n_host, "host_path_ms": round(t_host, 3), "host_path_ms_per_image": round(t_host / n_host, 3),
                     "device_ms_per_image": round(done / G, 4), "workspace_bytes": int(need),
                     "canvas_bytes_read_plus_written": 2 * 3 * G * H * W,
                     "canvas_GBps_at_kernel_median": round(2 * 3 * G * H * W / (kernels["median_us"] * 1e-6) / 1e9, 1)}
    return rec


def heat_leg(dev, reps, M=16, H=480, W=640, inner=20):
    """ops.heat_paint of M maps of H x W over their images (three launches) against the same steps as torch device ops: amin /
    amax per map, the normalisation and the direction weight, the peak, the levels, the ramp gathered per pixel and the blend.
    Device events around `inner` calls in a row, the two sides alternated window by window; median and range over reps windows.
    The torch side is compared with the call first: the shares of equal levels and equal picture bytes are reported."""
    from hybridgl_amd import render
    from hybridgl_amd import utils as U
    rng = np.random.default_rng(5)
    heat = torch.from_numpy(rng.standard_normal((M, H, W)).astype(np.float32)).to(dev)
    base = torch.from_numpy(rng.integers(0, 256, (M, H, W, 3), dtype=np.uint8)).to(dev)
    dirs = [("none", "left", "right", "middle")[m % 4] for m in range(M)]
    maps, _, _, total = ops.heat_paint_layout([(H, W)] * M, dirs)
    rows = render.ramp("heat")
    ramp = torch.from_numpy(rows.view(np.int32).copy()).to(dev)
    out = torch.empty(3 * total, dtype=torch.uint8, device=dev)
    lev = torch.empty(total, dtype=torch.uint8, device=dev)
    call = lambda: ops.heat_paint(heat, maps, ramp, base=base.view(-1), out=out, levels=lev)
    w = torch.stack([U.gen_dir_mask(d, 1, W, dev)[0] for d in dirs])[:, None, :]      # [M,1,W]
    colours = torch.from_numpy(np.stack([(rows[:, 0] >> 16) & 255, (rows[:, 0] >> 8) & 255, rows[:, 0] & 255], 1).astype(np.float32)).to(dev)
    a_l, b_l = (torch.from_numpy(rows[:, c].copy().view(np.float32)).to(dev) for c in (1, 2))

    def steps():
        mn, mx = heat.amin((1, 2), keepdim=True), heat.amax((1, 2), keepdim=True)
        g = (heat - mn) / (mx - mn) * w
        L = torch.round(g / g.amax((1, 2), keepdim=True) * 255.0).long()
        pic = torch.round(base.float() * a_l[L][..., None] + colours[L] * b_l[L][..., None]).clamp_(0, 255).to(torch.uint8)
        return pic, L

    pics, levels, status = call()
    pic_t, L_t = steps()
    torch.cuda.synchronize()
    assert not status[:, 0].any()
    # the same steps, not the same contract: torch's own division and a fused multiply-add in its blend may move a last bit
    same_l = float((torch.stack(levels).long() == L_t).float().mean())
    same = float((torch.stack(pics) == pic_t).float().mean())

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / inner

    for _ in range(3):
        window(call), window(steps)
    t_call, t_steps = [], []
    for _ in range(reps):
        t_call.append(window(call))
        t_steps.append(window(steps))
    px = M * H * W
    byt = px * (4 * 3 + 3 + 3 + 1)      # the map read three times, the base read, the picture and the levels written
    stat = lambda t: {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
    return {"maps": M, "size": [H, W], "inner_calls_per_window": inner, "heat_paint": stat(t_call), "torch_steps": stat(t_steps),
            "speedup_median": round(statistics.median(t_steps) / statistics.median(t_call), 2),
            "algorithmic_bytes": byt, "heat_paint_GBps": round(byt / statistics.median(t_call) / 1e3, 1),
            "levels_equal_share": same_l, "pictures_equal_share": same,
            "note": "device events around windows of calls issued back to back, so the host's enqueue cost counts where it exceeds the kernels'"}


def polygons_leg(dev, reps, cli_images):
    import shutil
    import subprocess
    import tempfile
    from hybridgl_amd import _lib, proposals as P, refer_io
    from hybridgl_amd.loader import pin_upload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = np.load(os.path.join(root, "tests", "golden", "gtmask.npz"))
    i = next(i for i in range(int(gold["n_cases"][0])) if tuple(gold[f"c{i}_size"]) == (480, 640))
    H, W = 480, 640
    xy, npts = gold[f"c{i}_xy"], gold[f"c{i}_npts"]
    gon, tri = xy[:2 * npts[0]].reshape(-1, 2), xy[2 * npts[0]:].reshape(-1, 2)
    rng = np.random.default_rng(1)
    entries = []
    for _ in range(64):
        s, d = rng.uniform(0.5, 1.0), rng.uniform(-60, 60, 2)
        entries.append([((gon - (320, 240)) * s + (320, 240) + d).ravel().tolist(), (tri + rng.uniform(-5, 5, 2)).ravel().tolist()])
    sizes, counts = [(H, W)], [64]

    def device_path():
        ops.rle_from_polygons(entries, sizes, counts, device=dev)
        torch.cuda.synchronize()

    def host_path():
        gt = torch.stack([pin_upload((refer_io.gt_mask_from_polygons(e, H, W)[0] == 1).astype(np.uint8), dev) for e in entries])
        ops.rle_encode(gt)
        torch.cuda.synchronize()

    # the two paths agree, bit for bit
    slots, table, status = ops.rle_from_polygons(entries, sizes, counts, device=dev)
    gt = torch.stack([pin_upload((refer_io.gt_mask_from_polygons(e, H, W)[0] == 1).astype(np.uint8), dev) for e in entries])
    es, et = ops.rle_encode(gt)
    n = int(table[:, 0].max())
    assert torch.equal(table, et) and torch.equal(slots[:, :n], es[:, :n]) and int(status[:, 0].abs().sum()) == 0
    # the kernel alone: the ABI on buffers already on the device
    lib = _lib.load()
    polys = [np.asarray(p, np.float64) for e in entries for p in e]
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    xy_d = d(np.concatenate(polys), np.float64)
    po_d = d(np.concatenate([[0], np.cumsum([len(p) // 2 for p in polys])]), np.int32)
    ep_d = d(np.arange(0, 2 * 64 + 1, 2), np.int32)
    images = np.asarray([[H, W, 0]], dtype=np.int64)
    sw = ops.rle_slot_words(H, W)
    out = torch.empty(ops.rle_block_words("status", 64, sw), dtype=torch.int32, device=dev)
    t_p, s_p, st_p = (p.data_ptr() for p in ops.rle_block("status", out, 64, sw))
    ws =ops.workspace(lib.hgl_rle_from_polygons_workspace_bytes(images.ctypes.data, 1, 64, len(polys)), dev, "rle")

    def kernel():
        rc = lib.hgl_rle_from_polygons_device(xy_d.data_ptr(), po_d.data_ptr(), len(polys), ep_d.data_ptr(), 64, images.ctypes.data, 1, 0,
                                              s_p, sw, t_p, st_p, ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    rec = {"entries": 64, "size": [H, W], "vertices_per_entry": int(npts.sum()), "counts_per_entry_max": n,
           "device_path_wall_ms": host_ms(device_path, reps), "device_kernel_us": device_us(kernel, reps),
           "host_path_wall_ms": host_ms(host_path, reps)}
    rec["wall_ratio_host_over_device"] = rec["host_path_wall_ms"] / rec["device_path_wall_ms"]
    # the CLI leg: --proposal_ceiling on an on-disk tree, with and without --device_targets (fresh child processes)
    tree = tempfile.mkdtemp(prefix="hgl_refer_")
    try:
        info = synth.write_refer_tree(tree, n_images=cli_images)
        ds = refer_io.ReferDataset(tree, "refcoco", "unc", "val")
        store = P.ProposalStore(os.path.join(tree, "store"))
        for img in ds.refer.data["images"]:
            h, w = img["height"], img["width"]
            masks = np.zeros((8, h, w), bool)
            for k in range(8):
                y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
                masks[k, y0:y0 + int(rng.integers(20, h // 2)), x0:x0 + int(rng.integers(20, w // 2))] = True
            store.write(img["id"], P.build_records(h, w, [hsam.mask_to_rle(m)["counts"] for m in masks], [int(m.sum()) for m in masks],
                                                   np.zeros((8, 4), np.int64), np.ones(8), np.ones(8), np.zeros((8, 2)),
                                                   np.asarray([[0, 0, w, h]] * 8)))
        store.write_meta({})
        argv = [sys.executable, "-m", "hybridgl_amd.main", "--real", "--refer_data_root", tree, "--dataset", "refcoco", "--split", "val",
                "--bpe_vocab", os.path.join(tree, "bpe.txt.gz"), "--parse_json", os.path.join(tree, "parse.json"), "--heatmap", "given",
                "--proposals_dir", store.directory, "--result_dir", os.path.join(tree, "log")]
        env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cli = {"tree": info, "proposals_per_image": 8}
        for name, more in (("host_targets", []), ("device_targets", ["--device_targets"]), ("host_targets_again", []),
                           ("device_targets_again", ["--device_targets"])):
            path = os.path.join(tree, name + ".json")
            t0 = time.perf_counter()
            r = subprocess.run(argv + ["--proposal_ceiling", path] + more, env=env, capture_output=True, text=True, timeout=900)
            cli[name + "_wall_s"] = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            cli[name] = json.load(open(path))
        assert cli["host_targets"] == cli["device_targets"]
        rec["cli_proposal_ceiling"] = cli
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--polygons", action="store_true",
                    help="measure rle_from_polygons against the host codec + upload + encode; writes profiles/rle_polygons_bench.json")
    ap.add_argument("--cli_images", type=int, default=100, help="--polygons: images of the on-disk tree of the CLI leg")
    ap.add_argument("--match", action="store_true", help="measure rle_match against the pair list; writes profiles/rle_match_bench.json")
    ap.add_argument("--merge", action="store_true",
                    help="measure rle_merge against decode -> vote -> encode; writes profiles/rle_merge_bench.json")
    ap.add_argument("--nms", action="store_true",
                    help="measure rle_nms against the rle_match matrix walked in numpy; writes profiles/rle_nms_bench.json")
    ap.add_argument("--select", action="store_true",
                    help="measure rle_select against a device copy and the host re-pack; writes profiles/rle_select_bench.json")
    ap.add_argument("--clean", action="store_true",
                    help="measure rle_remove_small_regions against decode -> clean -> encode; writes profiles/rle_clean_bench.json")
    ap.add_argument("--strings", action="store_true",
                    help="measure the device string codec against the host codec per record; writes profiles/rle_strings_bench.json")
    ap.add_argument("--paint", action="store_true",
                    help="measure rle_paint against decode -> host blend -> upload; writes profiles/rle_paint_bench.json")
    ap.add_argument("--heat", action="store_true",
                    help="measure heat_paint against the same steps as torch device ops; writes profiles/rle_heat_bench.json")
    ap.add_argument("--decode", action="store_true", help="measure the decoder and rle_iou; writes profiles/rle_decode_bench.json")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--evaluator", action="store_true")
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rle_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    if args.polygons:
        out = {"polygons": polygons_leg(dev, args.reps, args.cli_images), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_polygons_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.heat:
        out = {"heat": heat_leg(dev, args.reps), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_heat_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.paint:
        out = {"paint": paint_leg(dev, args.reps), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_paint_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.strings:
        out = {"strings": strings_leg(dev, args.reps), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_strings_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.clean:
        out = {"clean": clean_leg(dev, args.reps), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_clean_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.nms:
        out = {"nms": nms_leg(dev, args.reps), "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_nms_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.select:
        out = {"select": select_leg(dev, args.reps), "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_select_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.merge:
        out = {"merge": merge_leg(dev, args.reps), "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_merge_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.match:
        out = {"match": match_leg(dev, args.reps), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_match_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.decode:
        rng = np.random.default_rng(7)
        yy, xx = np.mgrid[0:640, 0:640]
        blob = np.zeros((64, 640, 640), np.uint8)
        for i in range(64):      # seeded unions of ellipses, as the tests' blobs
            for _ in range(int(rng.integers(1, 4))):
                cy, cx, ry, rx = rng.random() * 640, rng.random() * 640, (0.05 + 0.3 * rng.random()) * 640, (0.05 + 0.3 * rng.random()) * 640
                blob[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
        out = {"decode": decode_leg(torch.from_numpy(blob).to(dev), args.reps), "reps": args.reps,
               "device": torch.cuda.get_device_name(0)}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_decode_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    masks = torch.from_numpy(np.ascontiguousarray(synth.synth_masks(64, 640, 640, 2000))).to(dev).view(torch.uint8)
    out = {"kernel": kernel_leg(masks, args.reps), "generator": generator_leg(masks, args.reps)}
    if args.evaluator:
        out["evaluator"] = evaluator_leg(dev, args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
