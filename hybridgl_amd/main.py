"""Evaluation driver with the reference's command line and report format (Hybridgl_main.py:23-261,
flags of utils.py:397-471) for the pieces this package owns.

`--synthetic N` evaluates N seeded RefCOCO-shaped refs (hybridgl_amd/synth.py) through the full device pipeline
and prints/appends the reference's two result lines.

`--real` walks the REFER annotations under --refer_data_root (hybridgl_amd/refer_io.py: refs(<splitBy>).p,
instances.json, COCO images; ground truth from the native polygon/RLE codec) with real checkpoints
(HYBRIDGL_CLIP_CHECKPOINT / HYBRIDGL_SAM_CHECKPOINT / HYBRIDGL_BPE_VOCAB).  The two external models of the
spaCy parse of the reference stays an input (--parse_json: {sent_id: {"noun_phrase", "other_nouns", "dirflag",
"relaflag"}}, default = whole sentence, no relation words).  The GEM heat-map of the noun phrase is computed on the
device (hybridgl_amd/gem.py, Hybridgl_main.py:200-201) unless --heatmap_dir/<sent_id>.npy supplies it; the blurred
background is OpenCV's fixed-point GaussianBlur restated on the device (Hybridgl_main.py:99).

    python -m hybridgl_amd.main --dataset refcocog --split val --fusion_mode G2L --synthetic 8
    python -m hybridgl_amd.main --dataset refcoco --split testA --real --refer_data_root ./refer/data
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m hybridgl_amd.main --real ...
    python -m hybridgl_amd.main --synthetic 8 --save_masks out      # ... and later, with no model or checkpoint:
    python -m hybridgl_amd.main --synthetic 8 --score_masks out     # the same report from the saved masks and the ground truth
    python -m hybridgl_amd.main --synthetic 8 --ensemble_masks a b c --ensemble_out voted   # saved runs voted into one, scored, saved
    python -m hybridgl_amd.main --real ... --save_proposals props   # SAM's proposals kept per image (hybridgl_amd/proposals.py) ...
    python -m hybridgl_amd.main --real ... --proposals_dir props --fusion_mode L2G     # ... and evaluated from, with no SAM

Under a launcher (WORLD_SIZE > 1) rank r evaluates the items i = r (mod R) of the loader's order and the metric rows
are gathered once at the end (hybridgl_amd/dist.py); rank 0 writes the report.
"""
import argparse
import os

import torch


def default_argument_parser():
    """the live flags of utils.py:397-471"""
    p = argparse.ArgumentParser(description="HybridGL evaluation (MI355X-native hot path)")
    p.add_argument("--dataset", default="refcoco", choices=["refcoco", "refcoco+", "refcocog", "phrasecut"],
                   help="phrasecut = the Hybridgl_main_PhraseCut.py path: one item per IMAGE with all its phrases, heavy AMG")
    p.add_argument("--phrasecut_root", default="./PhraseCutDataset/data/VGPhraseCut_v0",
                   help="image_data_split.json, refer_<split>.json, images/ (data/dataset_phrasecut.py:40)")
    p.add_argument("--unseen_mode", action="store_true", help="PhraseCut: skip phrases of COCO categories (dataset_phrasecut.py:63)")
    p.add_argument("--seen_mode", action="store_true", help="PhraseCut: only phrases of COCO categories (:65)")
    p.add_argument("--split", default=None,
                   help="default: val (Hybridgl_main.py), test for --dataset phrasecut (Hybridgl_main_PhraseCut.py:42)")
    p.add_argument("--fusion_mode", default="G2L", choices=["G2L", "L2G", "G2L&L2G", "crop"],
                   help="crop: the ViT on the local views alone (model/backbone.py:126); meant for --view_prompt crop / masked_crop")
    p.add_argument("--view_prompt", default="", metavar="SPEC_OR_PRESET",
                   help="what CLIP is shown for a proposal (ops.parse_view_prompt): hybridgl (default), black, gray, keep, red_circle, "
                        "masked_crop, crop, or key=value,... over a preset, e.g. red_circle,thickness=3,marker_rgb=0:255:0; a box "
                        "window (masked_crop, crop) needs --fusion_mode crop")
    p.add_argument("--refer_data_root", default="./refer/data")
    p.add_argument("--synthetic", type=int, default=4, help="number of seeded synthetic refs to evaluate")
    p.add_argument("--proposals", type=int, default=64)
    p.add_argument("--sam", action="store_true", help="also run the SAM ViT-H proposal stage on every ref")
    p.add_argument("--result_dir", default="./result_log")
    p.add_argument("--real", action="store_true", help="evaluate the REFER refs under --refer_data_root")
    p.add_argument("--parse_json", default="", help="pre-computed parse records keyed by sent_id")
    p.add_argument("--heatmap_dir", default="", help="pre-computed heat-maps <sent_id>.npy ([H,W] or any size, fp32)")
    p.add_argument("--heatmap", default="device", choices=["device", "given"],
                   help="device: GEM heat-maps computed here; given: --heatmap_dir files (real) / seeded maps (synthetic)")
    p.add_argument("--max_refs", type=int, default=0, help="stop after this many refs (0 = all)")
    p.add_argument("--clip_model", default="ViT-B/16")
    p.add_argument("--sam_model", default="default")
    p.add_argument("--bpe_vocab", default="", help="bpe_simple_vocab_16e6.txt.gz (or HYBRIDGL_BPE_VOCAB)")
    # proposal thresholds: Hybridgl_main.py:67-73 (8 / 0.7 / 0.7 / 800, no crops); --dataset phrasecut:
    # Hybridgl_main_PhraseCut.py:56-62 (64 / 0.86 / 0.92 / 100, one crop layer with 32 x 32 points per crop)
    p.add_argument("--points_per_side", type=int, default=None)
    p.add_argument("--pred_iou_thresh", type=float, default=None)
    p.add_argument("--stability_score_thresh", type=float, default=None)
    p.add_argument("--min_mask_region_area", type=int, default=None)
    p.add_argument("--crop_n_layers", type=int, default=None)
    p.add_argument("--crop_n_points_downscale_factor", type=int, default=None)
    p.add_argument("--points_per_batch", type=int, default=None,
                   help="prompts per decoder launch (a memory knob: 64 in the reference; default 64, PhraseCut 512)")
    p.add_argument("--box_nms_thresh", type=float, default=0.7, help="SamAutomaticMaskGenerator's default (Hybridgl_main.py:67-73 does not set it)")
    p.add_argument("--group", type=int, default=None,
                   help="images taken at a time by the two-stream loop (HybridGLPipeline.run); 1 = ref by ref on one stream; "
                        "default 16 (PhraseCut: 4 -- a heavy-AMG image holds ~5 GB of candidate masks until its counts are read)")
    p.add_argument("--workers", type=int, default=4, help="loader threads (Hybridgl_main.py:45 num_workers)")
    p.add_argument("--prepare", action="store_true",
                   help="size every workspace and touch every kernel of a full group before the loop starts (HybridGLPipeline.prepare)")
    p.add_argument("--proposal_cap", type=int, default=0,
                   help="keep at most this many proposals of the first NMS order per image (0 = all; the benchmark's fixed 64)")
    p.add_argument("--host_transforms", action="store_true",
                   help="ToTensor/Normalize and the GEM transform on the loader threads' CPU (numpy / PIL) as the reference's "
                        "DataLoader workers do, instead of bit-identical device kernels (hybridgl_amd/transforms.py)")
    p.add_argument("--precision", default=None, choices=["f16x3", "f32", "f16"],
                   help="arithmetic of the encoders (default: HYBRIDGL_PRECISION, else f16x3); f16 = fp16 GEMM operands with fp32 "
                        "accumulation, opt-in and not fp32-class")
    p.add_argument("--on_overflow", default="raise", choices=["raise", "rescue"],
                   help="an activation beyond the fp16 range in f16x3 / f16 mode: raise = stop at the offending group (rerun with "
                        "--precision f32); rescue = run the groups that were in flight again in f32 and go on (grouped loop only)")
    p.add_argument("--stats_json", default="", help="rank 0 writes {stats, metrics} of the run here (throughput, loader wait)")
    p.add_argument("--k_clamp", default="auto", choices=["auto", "persistent", "per_ref"],
                   help="the k1 / k2 clamp of Hybridgl_main.py:178-181: persistent = the reference's quirk (once an image yields "
                        "fewer than 3 / 6 proposals the clamp stays for every later item OF THE PROCESS: depends on the number of "
                        "ranks); per_ref = that item only (order- and sharding-independent); auto = persistent on one rank, "
                        "per_ref under sharding")
    p.add_argument("--save_masks", default="", metavar="DIR",
                   help="every rank writes DIR/masks.rank{rank}.jsonl: one line per sentence with its two winning masks as COCO "
                        "RLE strings and its IoU counts (INTEGRATION.md); the files of all ranks together are the job's predictions")
    p.add_argument("--score_masks", default="", metavar="DIR",
                   help="score the predictions a run saved with --save_masks DIR against the dataset's ground truth, without any "
                        "model or checkpoint (the dataset flags as in that run); exits non-zero when a stored count differs")
    p.add_argument("--render_masks", default="", metavar="DIR",
                   help="paint the predictions a run saved with --save_masks DIR over the dataset's images, on the device, without "
                        "any model (the dataset flags as in that run): one PNG per sentence under --render_out")
    p.add_argument("--render_out", default="", metavar="OUT", help="--render_masks: the directory of the {index:06d}_{sentence}.png files")
    p.add_argument("--render_which", default="final", choices=["final", "pure", "both"],
                   help="--render_masks: the winner with spatial guidance (the demo's blue), the pure CLIP winner, or pure (red) then final")
    p.add_argument("--render_limit", type=int, default=0, metavar="N", help="--render_masks: stop after N pictures (0 = all)")
    p.add_argument("--ensemble_masks", nargs="+", default=[], metavar="DIR",
                   help="vote two or more runs saved with --save_masks into one prediction, mask by mask on the device "
                        "(predictions.ensemble: ops.rle_merge on the strings' runs), score it against the dataset's ground truth "
                        "and write it to --ensemble_out; no model is built, no checkpoint read (the dataset flags as in those runs)")
    p.add_argument("--ensemble_rule", default="majority", metavar="RULE",
                   help="with --ensemble_masks: majority, union, intersect, at_least:T or exactly:T over the (weighted) votes")
    p.add_argument("--ensemble_weights", nargs="+", type=int, default=None, metavar="W",
                   help="with --ensemble_masks: one non-negative integer per directory; a run of weight 2 votes twice")
    p.add_argument("--ensemble_out", default="", metavar="OUT",
                   help="with --ensemble_masks: the directory that receives the voted masks.rank0.jsonl (readable by --score_masks)")
    p.add_argument("--save_proposals", default="", metavar="DIR",
                   help="with --real: keep the mask generator's proposals beside the run, DIR/<image_id>.json in the format of "
                        "SAM's scripts/amg.py --convert-to-rle plus DIR/meta.json (INTEGRATION.md); the run itself is unchanged")
    p.add_argument("--proposals_dir", default="", metavar="DIR",
                   help="with --real: take every image's proposals from a store --save_proposals (or SAM's amg.py) wrote instead of "
                        "running SAM: no SAM model is built, no checkpoint read; an image the store lacks is an error")
    p.add_argument("--mask_nms_thresh", type=float, default=None, metavar="T",
                   help="with --proposals_dir: thin every image's stored list by mask overlap as it loads, on the device -- an entry "
                        "falls when a kept entry before it in the walk has ratio > T with it; what `python -m hybridgl_amd.proposals "
                        "thin` would write to a second store, without the store; --proposal_cap then caps the survivors")
    p.add_argument("--mask_nms_metric", default="iou", choices=["containment", "iou"],
                   help="with --mask_nms_thresh: the ratio, I / union or I / the smaller area")
    p.add_argument("--mask_nms_score", default="predicted_iou", choices=["predicted_iou", "stability_score", "area", "stored"],
                   help="with --mask_nms_thresh: the record field the walk is ordered by, descending (stored: the stored order)")
    p.add_argument("--rle_strings", default="host", choices=["host", "device"],
                   help="with --save_proposals / --proposals_dir: where the COCO strings of the store are written and read -- on the "
                        "host, one record at a time, or on the device (ops.rle_to_strings / ops.rle_from_strings); files and rows "
                        "are identical either way")
    p.add_argument("--proposal_ceiling", default="", metavar="OUT",
                   help="with --proposals_dir: write the proposal ceiling of the store -- per sentence the stored proposal of the "
                        "largest IoU against the ground truth, {oIoU, mIoU, cum, n_sentences} as the sweep reports it -- here and "
                        "exit; no SAM, CLIP or GEM model is built (the dataset flags and --proposal_cap as in the run)")
    p.add_argument("--device_targets", action="store_true",
                   help="with --score_masks or --proposal_ceiling on --real REFER data: take every target's size and polygons from "
                        "the annotations alone and rasterise them on the device, straight into run lengths "
                        "(ops.rle_from_polygons); no image file is opened, nothing is rasterised on the host; same rows and metrics")
    p.add_argument("--sweep", default="", metavar="SPEC",
                   help="score every ref under a grid of the tail's hyper-parameters in the same pass, e.g. "
                        "'r=0.3,0.5,0.7;alpha=0:1:0.1;k1=3;k2=6': an axis is a value list or lo:hi:step (hi included), an axis "
                        "left out keeps the run's value; the grid is the product, r slowest and k2 fastest (at most 256 "
                        "configurations, 32 distinct r).  The run's own result is unchanged; see --sweep_json")
    p.add_argument("--sweep_json", default="", metavar="OUT",
                   help="with --sweep: rank 0 writes the configurations, their oIoU / mIoU (pure and with guidance), the proposal "
                        "ceiling and the best configuration by final oIoU here (INTEGRATION.md)")
    return p


def sweep_report(configs, sm):
    """what --sweep_json holds, from HybridGLPipeline.sweep_metrics()"""
    keys = ("r", "alpha", "k1", "k2", "oIoU", "mIoU", "oIoU_final", "mIoU_final", "n_sentences")
    best = sm["best"]
    return {"configs": [dict(zip(("r", "alpha", "k1", "k2"), t)) for t in configs],
            "metrics": [{k: m[k] for k in keys} for m in sm["configs"]],
            "ceiling": sm["ceiling"],
            "best": None if best is None else dict({k: sm["configs"][best][k] for k in keys}, index=best)}


OTHER_NOUN_PREFIX = "a photo of "   # Hybridgl_main.py:160: clip.tokenize('a photo of ' + other_noun)


def sentence_strings(raw, rec):
    """The strings the reference tokenises for one sentence (Hybridgl_main.py:146-161), in the row order of
    pipeline.Sentence: [sentence, noun phrase, 'a photo of ' + other noun ...].  `rec` is the sentence's parse record
    ({"noun_phrase", "other_nouns": bare phrases as extract_nouns returns them, ...}); missing -> whole sentence, no nouns."""
    others = list(rec.get("other_nouns", []))
    return [raw, rec.get("noun_phrase", raw)] + [OTHER_NOUN_PREFIX + o for o in others]


class _Slot:
    """one image of RealRefs' look-aside: filled by the loader thread that met the image first, awaited by the others"""
    __slots__ = ("done", "value", "error")

    def __init__(self):
        import threading
        self.done, self.value, self.error = threading.Event(), None, None


class RealRefs:
    """The dataset side of the loop (Hybridgl_main.py:40-45,79-146): `jobs(rank, world)` = the dataset positions of this
    rank in the loader's order, `load(i)` = one RefBatch.  `load` is what hybridgl_amd.loader.Prefetcher runs on its
    background threads, each with its own copy stream current:

        host    JPEG decode (PIL), BPE, ground-truth rasterisation (native codec), pinned uploads of the uint8 image,
                the tokens and the target
        device  image['image'] = ToTensor + Normalize and image['tensor_img'] = the GEM transform (bicubic resize to
                448 x 448 + Normalize), bit-identical to the host transforms (hybridgl_amd/transforms.py) -- 24 of the
                28 ms of host work an item costs the reference's workers; `device_transforms=False` restores the host
                versions (numpy / PIL)

    The dataset yields one item per REF and re-decodes the image for each (data/dataset_refer_bert.py:103-110); here
    the decoded image and its two device tensors are shared by the refs of an image that the loader meets within its
    look-ahead (`image_lru` images)."""

    def __init__(self, args, dev, splitBy, context_length, device_transforms=True, image_lru=48):
        import collections
        import json
        import threading
        from .refer_io import ReferDataset
        from .tokenizer import SimpleTokenizer
        from .gem import get_gem_img_transform
        self.args, self.dev, self.context_length = args, dev, context_length
        self.ds = ReferDataset(args.refer_data_root, args.dataset, splitBy, args.split)
        self.tk = SimpleTokenizer(args.bpe_vocab or None)
        self._tk_lock = threading.Lock()        # the BPE cache is a plain dict shared by the loader threads
        self.preprocess = get_gem_img_transform()                                       # Hybridgl_main.py:39
        self.parse = json.load(open(args.parse_json)) if args.parse_json else {}
        self.n = len(self.ds) if args.max_refs <= 0 else min(len(self.ds), args.max_refs)
        self.device_transforms = device_transforms
        self.image_lru = int(image_lru)
        self._imgs = collections.OrderedDict()
        self._lock = threading.Lock()
        self.decoded = 0        # images decoded / uploaded (<= items loaded)
        self.proposals = None   # a proposals.StoredProposals: its files are read and packed here, on the loader threads

    def jobs(self, rank=0, world=1):
        from .dist import shard_by_groups
        image_ids = [self.ds.image_id(i) for i in range(self.n)]
        return shard_by_groups(image_ids, rank, world)   # refs of one image stay on one rank (per-image cache)

    def _image(self, i):
        """(sam_img u8 [H,W,3], image_norm f32 [3,H,W], tensor_img f32 [3,448,448] | None) of item i on the device, valid
        on the calling thread's current stream."""
        iid = self.ds.image_id(i)
        with self._lock:
            slot = self._imgs.get(iid) if self.image_lru > 0 else None
            owner = slot is None
            if owner:
                slot = _Slot()
                if self.image_lru > 0:
                    self._imgs[iid] = slot
                    while len(self._imgs) > self.image_lru:
                        self._imgs.popitem(last=False)
            elif self.image_lru > 0:
                self._imgs.move_to_end(iid)
        if not owner:
            slot.done.wait()
            if slot.error is not None:
                raise slot.error
            ev, val = slot.value
            torch.cuda.current_stream().wait_event(ev)     # the uploads ran on another loader thread's stream
            return val
        try:
            from . import synth, transforms as T
            from .loader import pin_upload
            img = self.ds.image(i)
            sam_img = pin_upload(img, self.dev)
            want_gem = self.args.heatmap == "device"
            if self.device_transforms:
                norm = T.to_tensor_normalize(sam_img)
                timg = T.gem_img_transform(sam_img) if want_gem else None
            else:
                norm = pin_upload(synth.imagenet_normalize(img), self.dev)
                timg = pin_upload(self.preprocess(img), self.dev) if want_gem else None
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with self._lock:
                self.decoded += 1
            slot.value = (ev, (sam_img, norm, timg))
            return slot.value[1]
        except BaseException as e:
            slot.error = e
            with self._lock:
                self._imgs.pop(iid, None)
            raise
        finally:
            slot.done.set()

    def load(self, i):
        import numpy as np
        from .gem import GEMWrapper, resize_antialias
        from .loader import pin_upload
        from .pipeline import RefBatch, Sentence
        from .tokenizer import tokenize
        args, dev = self.args, self.dev
        sam_img, image_norm, tensor_img = self._image(i)
        H, W = sam_img.shape[:2]
        rid = self.ds.ref_ids[i]
        ref = self.ds.refer.Refs[rid]
        if self.proposals is not None:
            self.proposals.prefetch(int(ref["image_id"]), (H, W))
        annot, sentences = self.ds.target(i), self.ds.sentence_raws[i]
        strings, sents = [], []
        t = lambda a: pin_upload(a, dev)
        for sent_id, raw in zip(ref["sent_ids"], sentences):
            rec = self.parse.get(str(sent_id), {})
            # Hybridgl_main.py:131-141 tokenises the lower-cased sentence re-joined from spaCy's tokens; the record carries it
            raw = rec.get("sentence_for_spacy", raw)
            row = len(strings)
            others = list(rec.get("other_nouns", []))   # extract_nouns' phrases, bare (utils.py:82-98)
            strings += sentence_strings(raw, rec)
            attn = None
            if args.heatmap_dir and os.path.exists(os.path.join(args.heatmap_dir, f"{sent_id}.npy")):
                a = t(np.load(os.path.join(args.heatmap_dir, f"{sent_id}.npy")).astype(np.float32))
                if tuple(a.shape) != (H, W):     # Hybridgl_main.py:201: T.Resize((h, w), antialias=True)
                    a = resize_antialias(a[None], (H, W))[0]
                attn = a
            gem_row = None
            if attn is None and args.heatmap == "device":
                gem_row = len(strings)                                         # Hybridgl_main.py:200 gem_model(tensor_img, [noun_phrase])
                strings += GEMWrapper.prompts([rec.get("noun_phrase", raw)])
            elif attn is None:
                attn = torch.ones((H, W), dtype=torch.float32, device=dev)     # uniform: no spatial guidance
            sents.append(Sentence(row, row + 1, list(range(row + 2, row + 2 + len(others))), rec.get("dirflag", "none"),
                                  rec.get("relaflag", "none"), len(others), attn, gem_row=gem_row))
        with self._tk_lock:
            tokens = tokenize(strings, context_length=self.context_length, tokenizer=self.tk)   # raises on over-long text, as clip.tokenize
        placeholder = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
        return RefBatch(sam_img, None, image_norm, placeholder,
                        torch.zeros((1, 4), dtype=torch.int64, device=dev), t(tokens), t(annot), sents, None,
                        int(ref["image_id"]), tensor_img=tensor_img,
                        token_len=int(tokens.argmax(axis=1).max()) + 1, index=i)


def real_refs(args, dev, splitBy, context_length, rank=0, world=1):
    """RefBatch per dataset item of this rank, in the loader's order, prepared on the calling thread (no prefetching)."""
    rr = RealRefs(args, dev, splitBy, context_length)
    for i in rr.jobs(rank, world):
        yield rr.load(i)


AMG_DEFAULTS = {   # Hybridgl_main.py:67-73 / Hybridgl_main_PhraseCut.py:56-62
    "refer": dict(points_per_side=8, pred_iou_thresh=0.7, stability_score_thresh=0.7, min_mask_region_area=800, crop_n_layers=0,
                  crop_n_points_downscale_factor=1, points_per_batch=64, group=16),
    "phrasecut": dict(points_per_side=64, pred_iou_thresh=0.86, stability_score_thresh=0.92, min_mask_region_area=100,
                      crop_n_layers=1, crop_n_points_downscale_factor=2, points_per_batch=1024, group=4),
}


def resolve_defaults(args, loop=True):
    """fill the flags left at None with the configuration of the reference script that --dataset selects; loop=False: for a
    branch that runs no evaluation loop (the loop's own flag combinations are not checked)"""
    for k, v in AMG_DEFAULTS["phrasecut" if args.dataset == "phrasecut" else "refer"].items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    if getattr(args, "split", None) is None:
        # Hybridgl_main_PhraseCut.py:42 evaluates PhraseCutDataset(split='test'); the REFER scripts their val split
        args.split = "test" if args.dataset == "phrasecut" else "val"
    if loop and getattr(args, "group", None) is not None and args.group <= 1 and getattr(args, "proposal_cap", 0):
        # the ref-by-ref path (HybridGLPipeline.step) keeps every proposal: silently ignoring the cap would give other results
        # than the grouped loop whenever the cap binds
        raise SystemExit("--proposal_cap applies to the grouped loop only: use --group >= 2 with it (or drop the cap)")
    return args


class RealPhraseCut:
    """The dataset side of Hybridgl_main_PhraseCut.py:40-43,67-119: one item per IMAGE (hybridgl_amd/phrasecut_io.py), all its
    phrases scored against one proposal set and one hybrid forward, a ground truth per phrase.  `load(i)` -> RefBatch whose
    sentences carry their own targets (None for an image whose phrases are all filtered out: the loop skips it)."""

    def __init__(self, args, dev, context_length):
        import json
        import threading
        from .phrasecut_io import PhraseCutDataset
        from .tokenizer import SimpleTokenizer
        self.args, self.dev, self.context_length = args, dev, context_length
        self.ds = PhraseCutDataset(args.phrasecut_root, args.split, unseen_mode=args.unseen_mode, seen_mode=args.seen_mode)
        self.tk = SimpleTokenizer(args.bpe_vocab or None)
        self._tk_lock = threading.Lock()
        self.parse = json.load(open(args.parse_json)) if args.parse_json else {}
        self.n = len(self.ds) if args.max_refs <= 0 else min(len(self.ds), args.max_refs)
        self.decoded = 0
        self.proposals = None   # as RealRefs.proposals

    def jobs(self, rank=0, world=1):
        from .dist import shard_indices
        return shard_indices(self.n, rank, world)

    def load(self, i):
        from . import transforms as T
        from .gem import GEMWrapper
        from .loader import pin_upload
        from .pipeline import RefBatch, Sentence
        from .tokenizer import tokenize
        item = self.ds[i]
        if item is None:
            return None
        dev = self.dev
        H, W = item["height"], item["width"]
        if self.proposals is not None:
            self.proposals.prefetch(int(item["image_id"]), (H, W))
        sam_img = pin_upload(item["sam_img"], dev)
        file_img = sam_img if item["file_img"] is None else pin_upload(item["file_img"], dev)
        image_norm = T.phrasecut_image_norm(file_img, H, W)             # dataset_phrasecut.py:49-51 + Hybridgl_main_PhraseCut.py:69-70
        want_gem = self.args.heatmap == "device"
        tensor_img = T.gem_img_transform(file_img) if want_gem else None    # :44-45 preprocessor(image): the file's own pixels
        self.decoded += 1
        strings, sents = [], []
        for j, phrase in enumerate(item["phrases"]):
            rec = self.parse.get(phrase, self.parse.get(phrase.lower(), {}))
            sentence = rec.get("sentence_for_spacy", phrase.lower())          # Hybridgl_main_PhraseCut.py:118-129
            row = len(strings)
            others = list(rec.get("other_nouns", []))
            strings += sentence_strings(sentence, rec)
            gem_row, attn = None, None
            if want_gem:
                gem_row = len(strings)
                strings += GEMWrapper.prompts([rec.get("noun_phrase", sentence)])      # :200
            else:
                attn = torch.ones((H, W), dtype=torch.float32, device=dev)
            gt = pin_upload(self.ds.gt_mask(item, j).astype("uint8"), dev)
            sents.append(Sentence(row, row + 1, list(range(row + 2, row + 2 + len(others))), rec.get("dirflag", "none"),
                                  rec.get("relaflag", "none"), len(others), attn, gt, gem_row=gem_row))
        with self._tk_lock:
            tokens = tokenize(strings, context_length=self.context_length, tokenizer=self.tk)
        placeholder = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
        return RefBatch(sam_img, None, image_norm, placeholder, torch.zeros((1, 4), dtype=torch.int64, device=dev),
                        pin_upload(tokens, dev), sents[0].target, sents, None, int(item["image_id"]), tensor_img=tensor_img,
                        token_len=int(tokens.argmax(axis=1).max()) + 1, index=i)


def split_by(dataset):
    return "umd" if dataset == "refcocog" else "unc"          # Hybridgl_main.py:26-29


def check_mask_nms_flags(args):
    """--mask_nms_thresh thins a store as it loads: it needs the store, a number, and a run (the ceiling reads the files itself)"""
    thr = getattr(args, "mask_nms_thresh", None)
    if thr is None:
        return
    if not getattr(args, "proposals_dir", ""):
        raise SystemExit("--mask_nms_thresh thins the proposals of a store as they load: it needs --proposals_dir (the generator's "
                         "own proposals are thinned by writing a store and reading it back)")
    if thr != thr:
        raise SystemExit("--mask_nms_thresh is NaN")
    if getattr(args, "proposal_ceiling", ""):
        raise SystemExit("--mask_nms_thresh and --proposal_ceiling exclude each other: the ceiling reads the store's files as they "
                         "are; write the thinner store with `python -m hybridgl_amd.proposals thin` and ask for its ceiling")


def check_proposal_flags(args):
    check_mask_nms_flags(args)
    save, read = getattr(args, "save_proposals", ""), getattr(args, "proposals_dir", "")
    if save and read:
        raise SystemExit("--save_proposals and --proposals_dir exclude each other: a run either writes a store or reads one")
    if (save or read) and not args.real:
        raise SystemExit("--save_proposals / --proposals_dir need --real: a store is keyed by the dataset's image ids")
    if save and getattr(args, "on_overflow", "raise") == "rescue":
        raise SystemExit("--save_proposals and --on_overflow rescue exclude each other: the store would keep the proposals of a pass "
                         "that a rescue rolls back and runs again in f32; write the store with --on_overflow raise")
    if read and getattr(args, "prepare", False):
        raise SystemExit("--prepare rehearses the loop on synthetic images, which a proposal store does not hold: drop one of "
                         "--prepare and --proposals_dir")


def build_models(args, dev):
    """(CLIPViTFM, SamAutomaticMaskGenerator | None, GEM model | None) as Hybridgl_main.py:36-38,47-48,66-74 builds them"""
    from .backbone import CLIPViTFM
    resolve_defaults(args)
    if getattr(args, "precision", None) is None:
        from . import ops
        args.precision = ops.default_precision()
    model = CLIPViTFM(model_name=args.clip_model, device=dev, precision=args.precision).eval()
    gen = None
    check_proposal_flags(args)
    if getattr(args, "proposals_dir", ""):      # the store stands in for the generator: no SAM model, no checkpoint
        from .proposals import StoredProposals
        gen = StoredProposals(args.proposals_dir, dev, mask_nms_thresh=getattr(args, "mask_nms_thresh", None),
                              mask_nms_metric=getattr(args, "mask_nms_metric", "iou"),
                              mask_nms_score=getattr(args, "mask_nms_score", "predicted_iou"),
                              strings=getattr(args, "rle_strings", "host"))
    elif args.sam or args.real:
        from .sam import SamAutomaticMaskGenerator, sam_model_registry
        sam = sam_model_registry[args.sam_model](device=dev, precision=args.precision)
        # Hybridgl_main.py:67-73
        gen = SamAutomaticMaskGenerator(sam, points_per_side=args.points_per_side, points_per_batch=args.points_per_batch,
                                        pred_iou_thresh=args.pred_iou_thresh, stability_score_thresh=args.stability_score_thresh,
                                        box_nms_thresh=args.box_nms_thresh, crop_n_layers=args.crop_n_layers,
                                        crop_n_points_downscale_factor=args.crop_n_points_downscale_factor,
                                        min_mask_region_area=args.min_mask_region_area)
    gem_model = None
    if args.heatmap == "device":
        from .gem import create_gem_model
        gem_model = create_gem_model(args.clip_model, clip=model)          # Hybridgl_main.py:36-38 (same checkpoint: shared weights)
    return model, gen, gem_model


def dataset_items(args, dev, rank=0, world=1, sam_img_size=0, gem=False):
    """(dataset object | None, this rank's job list, item maker i -> RefBatch | None) of the run that `args` describes:
    PhraseCut, REFER or the seeded synthetic refs.  What evaluate() loops over and what --score_masks takes the ground truth from."""
    from . import dist as D
    if args.real and args.dataset == "phrasecut":
        from .weights import CLIP_CONFIGS
        rr = RealPhraseCut(args, dev, CLIP_CONFIGS[args.clip_model]["context_length"])
        return rr, rr.jobs(rank, world), rr.load
    if args.real:
        from .weights import CLIP_CONFIGS
        rr = RealRefs(args, dev, split_by(args.dataset), CLIP_CONFIGS[args.clip_model]["context_length"],
                      device_transforms=not getattr(args, "host_transforms", False))
        return rr, rr.jobs(rank, world), rr.load
    from .pipeline import synthetic_ref
    make = lambda i: synthetic_ref(i, dev, N=args.proposals, sam_img_size=sam_img_size, gem=gem, device_blur=True)[0]
    return None, D.shard_indices(args.synthetic, rank, world), make


def report_text(args, m, precision=None, rescued=None):
    """the result lines of Hybridgl_main.py:233-248 / Hybridgl_main_PhraseCut.py:224-238; rescued: HybridGLPipeline.rescue_stats,
    a line of its own when a rescue happened"""
    pc = args.dataset == "phrasecut"
    from . import ops
    prompt = ops.parse_view_prompt(getattr(args, "view_prompt", "") or None)
    return (f"\n\n fusion_mode={args.fusion_mode} " + ("" if ops.view_prompt_is_default(prompt) else f"view_prompt={ops.view_prompt_name(prompt)} ")
            + (f"\nDataset: PhraseCut / {args.split}" if pc else f"\nDataset: {args.dataset} / {args.split} / {split_by(args.dataset)}") +
            f"\nOverall IoU / mean IoU"
            f"\npure hybridgl: {m['oIoU']:.2f} / {m['mIoU']:.2f}"
            f"\nhybridgl w/ spatial guidance: {m['oIoU_final']:.2f} / {m['mIoU_final']:.2f}"
            + (f"\nprecision: {precision}" if precision is not None else "")
            + (f"\nfp16 range: {rescued['events']} overflow(s) rescued, {rescued['refs']} refs in {rescued['groups']} groups re-run in f32"
               if rescued and rescued.get("events", 0) > 0 else ""))


def write_report(args, text):
    """append the result lines to the run's result log (Hybridgl_main.py:233-248) and print them"""
    os.makedirs(args.result_dir, exist_ok=True)                         # Hybridgl_main.py:233-248
    name = "result_log_PhraseCut.txt" if args.dataset == "phrasecut" else f"result_log_{args.dataset}_{args.split}.txt"
    with open(os.path.join(args.result_dir, name), "a") as f:
        f.write(text)
    print(text)


def check_device_targets(args):
    """--device_targets belongs to the two branches that build no model, on REFER annotations"""
    if not getattr(args, "device_targets", False):
        return
    if not (getattr(args, "score_masks", "") or getattr(args, "proposal_ceiling", "") or getattr(args, "ensemble_masks", None)):
        raise SystemExit("--device_targets applies to --score_masks and --proposal_ceiling only: a run's own targets ride with its "
                         "items")
    if not args.real or args.dataset == "phrasecut":
        raise SystemExit("--device_targets needs --real REFER data: the polygons come from the REFER annotations (PhraseCut's "
                         "targets are Pillow's rasterisation of truncated vertices, the synthetic refs have no polygons)")


def offline_targets(args, dev):
    """((index, sentence), image id, target) of every sentence of the run that `args` describes, for the two branches that
    build no model.  Default: the items as a run builds them, minus what only the models read -- same indices, same targets;
    the target of a sentence is Sentence.target when set, else RefBatch.target.  --device_targets: index, sentence, image id,
    size and polygons from the REFER annotations alone (refer_io.PolygonTarget: no image file is opened, nothing is
    rasterised on the host); a ref whose annotation is an RLE dict keeps its pixel target."""
    if getattr(args, "device_targets", False):
        from .dist import shard_by_groups
        from .loader import pin_upload
        from .refer_io import ReferDataset
        ds = ReferDataset(args.refer_data_root, args.dataset, split_by(args.dataset), args.split)
        n = len(ds) if args.max_refs <= 0 else min(len(ds), args.max_refs)
        for i in shard_by_groups([ds.image_id(k) for k in range(n)], 0, 1):      # RealRefs.jobs
            ref = ds.refer.Refs[ds.ref_ids[i]]
            target = ds.target_polygons(i)
            if target is None:
                target = pin_upload(ds.target(i), dev)
            for j in range(min(len(ref["sent_ids"]), len(ds.sentence_raws[i]))):      # RealRefs.load's sentences
                yield (i, j), int(ref["image_id"]), target
        return
    _, jobs, make = dataset_items(args, dev, 0, 1, sam_img_size=0, gem=False)
    for i in jobs:
        ref = make(i)
        if ref is None:
            continue
        index = ref.index if ref.index is not None else i
        for j, sent in enumerate(ref.sentences):
            yield (index, j), ref.image_id, (sent.target if sent.target is not None else ref.target)


def score_masks(args, dev, directory=None):
    """--score_masks DIR: the metrics of a saved run (--save_masks) from its files and the dataset's ground truth alone -- no
    model is built, no checkpoint read.  The job list and the item makers are evaluate()'s; the target of a sentence is
    Sentence.target when set, else RefBatch.target.  The saved strings are decoded and met with the targets on the device
    (predictions.score: integer counts, exact), and every recomputed row is compared with the one the file stores.
    Returns (metrics as dist.metrics_from_rows reports them, {"rows": [n,6] int64, "mismatches": keys whose stored counts
    differ from the recomputed ones, "missing": dataset sentences without a record, "extra": records without a sentence})."""
    from . import dist as D
    from . import predictions as P
    resolve_defaults(args)
    check_device_targets(args)
    records = P.load(directory or args.score_masks)
    rows, missing, extra = P.score(records, ((key, t) for key, _, t in offline_targets(args, dev)))
    stored = {(r["index"], r["sentence"]): [r["I"], r["U"], r["I_final"], r["U_final"]] for r in records}
    mismatches = [(int(r[0]), int(r[1])) for r in rows if stored[(int(r[0]), int(r[1]))] != [int(v) for v in r[2:6]]]
    return D.metrics_from_rows(rows), {"rows": rows, "mismatches": mismatches, "missing": missing, "extra": extra}


def score_masks_main(args, dev):
    """the --score_masks branch of main(): report, result log, exit status"""
    m, rep = score_masks(args, dev)
    for name, what in (("missing", "dataset sentence without a saved record"), ("extra", "saved record without a dataset sentence"),
                       ("mismatches", "stored counts differ from the recomputed ones")):
        for k in rep[name]:
            print(f"{what}: index {k[0]} sentence {k[1]}")
    print(f"scored {len(rep['rows'])} saved sentences from {args.score_masks}: {len(rep['mismatches'])} mismatching, "
          f"{len(rep['missing'])} without a record, {len(rep['extra'])} without a sentence")
    write_report(args, report_text(args, m))
    if rep["mismatches"]:
        raise SystemExit(1)
    return m


RENDER_GROUP = 64      # pictures per ops.rle_paint call: the library's group limit


def render_masks(args, dev):
    """--render_masks DIR --render_out OUT: every saved sentence (--save_masks) painted over its image -- no model is built.  The
    records come from predictions.load, the images from the dataset the flags name (the items as a run builds them), the
    strings become runs on the device (ops.rle_from_strings) and RENDER_GROUP pictures leave one ops.rle_paint call; the PNG
    files are written on the host (render.save_png).  --render_which both: the pure winner in red, then the final one in the
    demo's blue over it.  Raises SystemExit for a record whose size differs from its image's, naming its key.  Returns the paths."""
    import numpy as np
    from . import ops, render
    from . import predictions as P
    resolve_defaults(args, loop=False)
    if not args.render_out:
        raise SystemExit("--render_masks needs --render_out OUT")
    by_key = {(r["index"], r["sentence"]): r for r in P.load(args.render_masks)}
    which = {"final": ["final"], "pure": ["pure"], "both": ["pure", "final"]}[args.render_which]
    rows = {"final": ops.rle_paint_style(**render.DEMO_STYLE), "pure": ops.rle_paint_style(**render.PURE_STYLE)}
    if args.render_which == "pure":
        rows["pure"] = rows["final"]      # alone, either winner wears the demo's style
    os.makedirs(args.render_out, exist_ok=True)
    paths, pending = [], []

    def flush():
        if not pending:
            return
        strings = [rec[w] for _, rec, _ in pending for w in which]
        buf, _, n_counts = ops.rle_strings_pack(strings)
        S = len(strings)
        d = buf.to(dev, non_blocking=True)
        slots, table, _ = ops.rle_from_strings(d[8 * (S + 1):], d[:8 * (S + 1)].view(torch.int64), S, max(int(n_counts.max()), 1))
        counts = [len(which)] * len(pending)
        pics, _, status = ops.rle_paint(slots, table, [tuple(im.shape[:2]) for _, _, im in pending], counts,
                                        np.tile(np.arange(len(which), dtype=np.int32), len(pending)), counts,
                                        np.stack([rows[w] for _ in pending for w in which]), base=[im for _, _, im in pending])
        codes = status[:, 0].cpu().numpy().reshape(len(pending), len(which))
        for (key, _, _), pic, code in zip(pending, pics, codes):
            if code.any():
                raise SystemExit(f"--render_masks: index {key[0]} sentence {key[1]}: the saved string does not decode to a mask of "
                                 f"the stated size (code {int(code.max())})")
            paths.append(os.path.join(args.render_out, f"{key[0]:06d}_{key[1]}.png"))
            render.save_png(paths[-1], pic)
        pending.clear()

    _, jobs, make = dataset_items(args, dev, 0, 1, sam_img_size=0, gem=False)
    full = lambda: bool(args.render_limit) and len(paths) + len(pending) >= args.render_limit
    for i in jobs:
        if full():
            break
        ref = make(i)
        if ref is None:
            continue
        index = ref.index if ref.index is not None else i
        for j in range(len(ref.sentences)):
            rec = by_key.get((index, j))
            if rec is None:
                continue
            if [int(v) for v in rec["size"]] != [int(v) for v in ref.sam_img.shape[:2]]:
                raise SystemExit(f"--render_masks: index {index} sentence {j}: the record's size {list(rec['size'])} differs from "
                                 f"the image's {list(ref.sam_img.shape[:2])}")
            if full():
                break
            pending.append(((index, j), rec, ref.sam_img))
            if len(pending) == RENDER_GROUP:
                flush()
    flush()
    print(f"painted {len(paths)} of {len(by_key)} saved sentences from {args.render_masks} into {args.render_out}")
    return paths


def check_ensemble_flags(args):
    """what --ensemble_masks needs and what it does not go with"""
    dirs = list(getattr(args, "ensemble_masks", None) or [])
    if len(dirs) < 2:
        raise SystemExit(f"--ensemble_masks takes two or more directories, got {len(dirs)}: one run is its own ensemble")
    w = getattr(args, "ensemble_weights", None)
    if w is not None and len(w) != len(dirs):
        raise SystemExit(f"--ensemble_weights has {len(w)} values for {len(dirs)} directories: one weight per directory")
    if getattr(args, "score_masks", "") or getattr(args, "proposal_ceiling", ""):
        raise SystemExit("--ensemble_masks does not combine with --score_masks or --proposal_ceiling: score the ensemble's own "
                         "--ensemble_out afterwards")
    if not getattr(args, "ensemble_out", ""):
        raise SystemExit("--ensemble_masks needs --ensemble_out: the directory that receives the voted predictions")


def ensemble_masks(args, dev):
    """--ensemble_masks DIR DIR [DIR ...] --ensemble_out OUT: the saved runs voted into one prediction (predictions.ensemble),
    scored against the dataset's ground truth as --score_masks scores a run (predictions.score over offline_targets) and saved
    to OUT with the counts filled in -- no model is built, no checkpoint read.  Returns (metrics, {"rows", "missing", "extra",
    "path"})."""
    from . import dist as D
    from . import predictions as P
    resolve_defaults(args)
    check_ensemble_flags(args)
    check_device_targets(args)
    records = P.ensemble(list(args.ensemble_masks), rule=args.ensemble_rule, weights=args.ensemble_weights, device=dev)
    rows, missing, extra = P.score(records, ((key, t) for key, _, t in offline_targets(args, dev)))
    counts = {(int(r[0]), int(r[1])): [int(v) for v in r[2:6]] for r in rows}
    for rec in records:      # a record without a target keeps zeros: --score_masks on OUT will name it as extra
        rec["I"], rec["U"], rec["I_final"], rec["U_final"] = counts.get((rec["index"], rec["sentence"]), [0, 0, 0, 0])
    path = P.save(records, args.ensemble_out, 0)
    return D.metrics_from_rows(rows), {"rows": rows, "missing": missing, "extra": extra, "path": path}


def ensemble_masks_main(args, dev):
    """the --ensemble_masks branch of main(): report, result log, one line that names the rule and the sets"""
    check_ensemble_flags(args)
    try:
        m, rep = ensemble_masks(args, dev)
    except (OSError, ValueError) as e:
        raise SystemExit(f"hybridgl_amd.main: {e}")
    for name, what in (("missing", "dataset sentence without a saved record"), ("extra", "saved record without a dataset sentence")):
        for k in rep[name]:
            print(f"{what}: index {k[0]} sentence {k[1]}")
    write_report(args, report_text(args, m))
    w = args.ensemble_weights
    print(f"ensemble of {len(args.ensemble_masks)} saved runs by {args.ensemble_rule}"
          + (f" with weights {' '.join(str(v) for v in w)}" if w else "")
          + f" ({', '.join(args.ensemble_masks)}): {len(rep['rows'])} sentences written to {rep['path']} (no model built)")
    return m


def proposal_ceiling(args, dev):
    """--proposals_dir DIR --proposal_ceiling OUT: the ceiling of a proposal store against the dataset's ground truth from the
    files alone -- no model is built, no checkpoint read.  Jobs, items and targets are those of score_masks(); the stored runs
    meet the encoded targets on the device (proposals.ceiling: integer counts, exact).  Returns ({"oIoU", "mIoU", "cum",
    "n_sentences"}: the "ceiling" block of HybridGLPipeline.sweep_metrics() for a run fed from the same store, rows [n,5])."""
    from . import dist as D
    from . import proposals as P
    resolve_defaults(args, loop=False)
    check_proposal_flags(args)
    check_device_targets(args)
    rows = P.ceiling(args.proposals_dir, offline_targets(args, dev), cap=getattr(args, "proposal_cap", 0) or None, device=dev,
                     group=max(int(getattr(args, "group", 16) or 16), 1))
    cm = D.metrics_from_rows(rows[:, [0, 1, 3, 4, 3, 4]])
    return {"oIoU": cm["oIoU"], "mIoU": cm["mIoU"], "cum": cm["cum"][:2], "n_sentences": cm["n_sentences"]}, rows


def proposal_ceiling_main(args, dev):
    """the --proposal_ceiling branch of main(): the file and one line"""
    import json
    if not getattr(args, "proposals_dir", ""):
        raise SystemExit("--proposal_ceiling needs --proposals_dir: the store whose ceiling is asked for")
    try:
        c, rows = proposal_ceiling(args, dev)
    except ValueError as e:
        raise SystemExit(f"hybridgl_amd.main: {e}")
    with open(args.proposal_ceiling, "w") as f:
        json.dump(c, f, indent=1)
    print(f"proposal ceiling of {args.proposals_dir} over {c['n_sentences']} sentences (no model built): oIoU {c['oIoU']:.2f} "
          f"mIoU {c['mIoU']:.2f}")
    return c


def save_masks(pipe, directory, rank=0):
    """--save_masks: DIR/masks.rank{rank}.jsonl, one JSON line per sentence this rank scored, keyed like dist.ROW_FIELDS:
    {"index": dataset position, "sentence": sentence number, "size": [H, W], "pure", "final": the winning masks (pure CLIP /
    with spatial guidance) as COCO compressed RLE strings (sam.coco_encode_rle), "I", "U", "I_final", "U_final": the metric
    row's counts}.  Returns the path."""
    from . import predictions as P
    from .sam import coco_encode_rle
    records = []
    for rec, row in zip(pipe.predictions(), pipe.partial_rows()):
        assert (rec["index"], rec["sentence"]) == (int(row[0]), int(row[1]))
        enc = lambda counts: coco_encode_rle({"size": rec["size"], "counts": counts})["counts"]
        records.append({"index": rec["index"], "sentence": rec["sentence"], "size": rec["size"], "pure": enc(rec["pure"]),
                        "final": enc(rec["final"]), "I": int(row[2]), "U": int(row[3]), "I_final": int(row[4]),
                        "U_final": int(row[5])})
    return P.save(records, directory, rank)


def evaluate(args, model, gen, gem_model, dev, rank=0, world=1, dist=None):
    """The loop of Hybridgl_main.py:79-247 over this rank's share of the dataset: loader threads -> HybridGLPipeline.run ->
    one exchange of the metric rows.  Returns (metrics of the whole job, stats of this rank: refs, seconds of the loop,
    seconds the loop waited for the loader, host seconds spent preparing items, images decoded, image-cache hits,
    refs skipped)."""
    import time
    from .loader import Prefetcher
    from .pipeline import EmptyProposals, HybridGLPipeline
    from . import dist as D
    resolve_defaults(args)
    k_clamp = args.k_clamp if args.k_clamp != "auto" else ("persistent" if world == 1 else "per_ref")
    save_dir = getattr(args, "save_masks", "")
    sweep = None
    if getattr(args, "sweep", ""):
        import inspect
        from .sweep import parse_sweep_spec
        own = inspect.signature(HybridGLPipeline.__init__).parameters      # the run's values: the pipeline's defaults
        sweep = parse_sweep_spec(args.sweep, *(own[n].default for n in ("r", "alpha", "k1", "k2")))
    check_proposal_flags(args)
    recorder = None
    if getattr(args, "save_proposals", ""):
        from .proposals import ProposalRecorder, generator_settings
        recorder = gen = ProposalRecorder(gen, args.save_proposals, generator_settings(
            gen, sam_model=args.sam_model, precision=getattr(args, "precision", None), proposal_cap=getattr(args, "proposal_cap", 0)),
            strings=getattr(args, "rle_strings", "host"))
    pipe = HybridGLPipeline(model, fusion_mode=args.fusion_mode, masking_block=getattr(args, "masking_block", 9), mask_generator=gen,
                            use_sam_masks=args.real, gem_model=gem_model, k_clamp=k_clamp, record_predictions=bool(save_dir), sweep=sweep,
                            on_overflow=getattr(args, "on_overflow", "raise"), view_prompt=getattr(args, "view_prompt", "") or None)
    rr, jobs, make = dataset_items(args, dev, rank, world, sam_img_size=1024 if gen else 0, gem=gem_model is not None)
    if rr is not None and getattr(gen, "prefetch", None) is not None:
        rr.proposals = gen      # files, JSON and run lengths are the loader threads' work
    # Hybridgl_main.py:45,79: DataLoader(num_workers=4) feeding the loop; here loader threads feed the grouped loop
    loader = Prefetcher(jobs, make, workers=args.workers, depth=2 * args.group + 2, device=dev)
    cap = getattr(args, "proposal_cap", 0) or None
    if getattr(args, "prepare", False) and args.group > 1:
        # workspaces, allocator blocks and kernel instantiations of a full group, before the first item arrives
        if recorder is not None:
            recorder.recording = False      # the rehearsal's synthetic images are not the dataset's
        pipe.prepare(group=args.group, H=640, W=640, proposals=cap or args.proposals)
        if recorder is not None:
            recorder.recording = True
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if args.group <= 1:      # ref by ref on one stream (Hybridgl_main.py:79-230 as written)
        n = 0
        for ref in loader:
            if ref is None:
                continue
            try:
                pipe.step(ref)
                n += 1
            except EmptyProposals:      # counted in pipe.skipped
                pass
    else:
        n = pipe.run(loader, group=args.group, proposal_cap=cap)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if save_dir:
        save_masks(pipe, save_dir, rank)      # this rank's own sentences: no collective
    if recorder is not None:
        recorder.flush()      # this rank's own images (shard_by_groups): no collective
    m = pipe.metrics(dist)      # one all-gather of the metric rows; identical on every rank
    stats = {"refs": n, "seconds": dt, "seconds_job": D.max_over_ranks(dt, dist, dev), "loader_wait_s": loader.wait_s, "loader_make_s": loader.make_s,
             "images_decoded": rr.decoded if rr is not None else None, "image_cache_hits": pipe.cache_hits,
             "skipped": pipe.skipped, "groups": pipe.groups_run,
             "workers": args.workers, "group": args.group,
             # this rank's own (ranks rescue independently); zeros without --on_overflow rescue
             "split_overflow_rescued": dict(pipe.rescue_stats, positions=list(pipe.rescue_stats["positions"]))}
    if recorder is not None:
        stats["proposals_saved"] = recorder.written
    if getattr(args, "proposals_dir", ""):
        stats["proposal_store"] = gen.settings()
        if getattr(gen, "mask_nms_thresh", None) is not None:      # this rank's own images
            stats["proposals_thinned"] = {"thr": gen.mask_nms_thresh, "metric": gen.mask_nms_metric, "score": gen.mask_nms_score,
                                          "before": int(gen.thinned[0]), "after": int(gen.thinned[1])}
    if sweep is not None:      # one more exchange of rows, on every rank
        stats["sweep"] = sweep_report(sweep, pipe.sweep_metrics(dist))
    return m, stats


def main(args):
    from . import dist as D
    if not torch.cuda.is_available():
        # the reference falls back to the CPU (Hybridgl_main.py:30-34); this package is the MI355X hot path and nothing else:
        # libhybridgl.so's entries return HGL_ENODEVICE without a HIP device (tests/test_abi.py)
        raise SystemExit("hybridgl_amd.main: no HIP device is visible.  This package has no CPU implementation of the hot path (by "
                         "design: a CPU fallback would void every parity claim); the reference's CPU configuration (BASELINE "
                         "configs[0]) is covered by the oracle tests: python -m pytest tests -m 'not gpu'")
    rank, local_rank, world = D.env_rank()
    dev = torch.device("cuda", local_rank % torch.cuda.device_count())
    if getattr(args, "ensemble_masks", None) or getattr(args, "ensemble_out", "") or getattr(args, "ensemble_weights", None):
        check_ensemble_flags(args)      # before any model exists, like the two branches below
        check_device_targets(args)
        if world > 1:
            raise SystemExit("--ensemble_masks runs on one rank: start it without a launcher (world size 1)")
        torch.cuda.set_device(dev)
        return ensemble_masks_main(args, dev)
    check_device_targets(args)
    check_mask_nms_flags(args)
    if getattr(args, "score_masks", ""):      # before any model exists: files and ground truth only
        if world > 1:
            raise SystemExit("--score_masks runs on one rank: start it without a launcher (world size 1)")
        torch.cuda.set_device(dev)
        return score_masks_main(args, dev)
    if getattr(args, "render_masks", ""):      # likewise: files and the dataset's images only
        if world > 1:
            raise SystemExit("--render_masks runs on one rank: start it without a launcher (world size 1)")
        torch.cuda.set_device(dev)
        return render_masks(args, dev)
    if getattr(args, "proposal_ceiling", ""):      # likewise: the store's files and ground truth only
        if world > 1:
            raise SystemExit("--proposal_ceiling runs on one rank: start it without a launcher (world size 1)")
        torch.cuda.set_device(dev)
        return proposal_ceiling_main(args, dev)
    cores = D.pin_rank_to_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))   # launch + loader threads of a rank on its own cores
    D.size_host_threads(cores, args.workers)
    torch.cuda.set_device(dev)
    dist = D.init_process_group(os.environ.get("HYBRIDGL_DIST_BACKEND", "nccl"), dev) if world > 1 else None
    model, gen, gem_model = build_models(args, dev)
    if rank == 0:
        print(f"fusion mode={args.fusion_mode}")
        if world > 1:
            print(f"ranks: {dist.get_world_size()} ({dist.get_backend()}), host cores per rank: {len(cores) or 'unpinned'}")
    m, stats = evaluate(args, model, gen, gem_model, dev, rank, world, dist)
    if stats["skipped"]:
        # the reference would fail on an image without proposals; count and go on
        print(f"{stats['skipped']} refs skipped: the proposal stage returned no mask")
    if dist is not None:
        dist.destroy_process_group()
    sweep = stats.pop("sweep", None)
    if rank != 0:
        return m
    if "proposal_store" in stats:
        print(f"proposals from {args.proposals_dir} (no SAM model built); generator settings of the store: "
              + (", ".join(f"{k}={v}" for k, v in stats["proposal_store"].items()) or "none recorded (no meta.json)")
              + ("".join(f"; thinned on load by mask NMS: thr={t['thr']:g} metric={t['metric']} score={t['score']}, "
                         f"{t['before']} -> {t['after']} proposals" for t in [stats["proposals_thinned"]])
                 if "proposals_thinned" in stats else ""))
    if sweep is not None:
        import json
        b = sweep["best"]
        print(f"sweep: {len(sweep['configs'])} configurations; proposal ceiling oIoU {sweep['ceiling']['oIoU']:.2f} mIoU "
              f"{sweep['ceiling']['mIoU']:.2f}; best final oIoU {b['oIoU_final']:.2f} at r={b['r']} alpha={b['alpha']} k1={b['k1']} k2={b['k2']}")
        if getattr(args, "sweep_json", ""):
            json.dump(sweep, open(args.sweep_json, "w"), indent=1)
    if getattr(args, "stats_json", ""):
        import json
        stats["refs_per_s"] = stats["refs"] / stats["seconds"] if stats["seconds"] > 0 else 0.0
        stats["world"] = world
        stats["precision"] = args.precision
        stats["host_cores_per_rank"] = len(cores) if cores else len(os.sched_getaffinity(0))
        json.dump({"stats": stats, "metrics": m}, open(args.stats_json, "w"))
    write_report(args, report_text(args, m, args.precision, stats.get("split_overflow_rescued")))
    return m


if __name__ == "__main__":
    main(default_argument_parser().parse_args())
