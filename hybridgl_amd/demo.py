"""One image, one sentence, one call: the mirror of the reference's demo.py.

    from hybridgl_amd.demo import HybridGL
    hgl = HybridGL()                                     # CLIP ViT-B/16, SAM ViT-H, GEM: built once
    seg = hgl.segment("cat.jpg", "the cat on left")[0]   # a Segmentation
    render.save_png("result.png", seg.overlay())         # the chosen mask painted over the image, on the device

    python -m hybridgl_amd.demo --image cat.jpg --text "the cat on left" --out result.png

The item is built from the pieces the evaluator's loader uses (main.RealRefs.load: pin_upload, transforms.to_tensor_normalize,
transforms.gem_img_transform, main.sentence_strings, GEMWrapper.prompts, tokenize, token_len) and scored by
HybridGLPipeline.step, so a sentence gets here what it gets in an evaluation.  spaCy stays outside: what the reference's
script parses out of the sentence (demo.py:84-118) comes in as a parse record -- the keys of the evaluator's --parse_json
records, tools/make_parse_records.py being the producer -- with RealRefs.load's defaults for a missing one: the noun phrase is
the sentence, there are no other nouns, the flags are "none".  The overlay is render.DEMO_STYLE (demo.py:212-219)."""
import argparse
import dataclasses
import sys

import torch

from . import ops, render

OUTLINE_INK = (255, 255, 255)      # the final winner's outline over a heat picture
PARSE_KEYS = ("sentence_for_spacy", "noun_phrase", "other_nouns", "dirflag", "relaflag")


@dataclasses.dataclass
class Explanation:
    """what the scoring tail was given and what it computed for one text (HybridGL(explain=True)), on the device"""
    heat: torch.Tensor         # float32 [H,W]: the raw GEM heat-map, before min-max and the direction weight
    dirflag: str               # "none" / "left" / "right" / "middle": the weight gen_dir_mask multiplies the map with
    black: float               # the relation's coherence constant (Hybridgl_main.py:211-216)
    score_clip: torch.Tensor   # float32 [N]: the pure CLIP score of every proposal; its argmax is index_pure
    score_neg: torch.Tensor    # float32 [N]: the score against the other nouns
    gem_score: torch.Tensor    # float32 [N]: the coherence score, ops.coherence_scores(heat, proposals, dirflag, black)


@dataclasses.dataclass
class Segmentation:
    text: str
    index_pure: int            # the winning proposal of the pure CLIP score, into the image's proposal list
    index_final: int           # ... with spatial guidance: the reference's result_seg_final
    rle_pure: dict             # COCO RLE dicts {"size": [H, W], "counts": str}, the strings written on the device
    rle_final: dict
    n_proposals: int
    image: torch.Tensor = dataclasses.field(repr=False)        # uint8 [H,W,3] on the device
    proposals: torch.Tensor = dataclasses.field(repr=False)    # bool [N,H,W] on the device
    winners: tuple = dataclasses.field(repr=False)             # (slots, table) of the call's winners on the device, 2 per text
    row: int = 0                                               # this text's first entry in `winners`: pure, then final
    explanation: Explanation = dataclasses.field(default=None, repr=False)      # with HybridGL(explain=True)

    def _which(self, which):
        if which not in ("pure", "final"):
            raise ValueError(f"which: {which!r} ('pure' or 'final')")
        return which == "final"

    def mask(self, which="final"):
        """the winning proposal, bool [H,W] on the device"""
        return self.proposals[self.index_final if self._which(which) else self.index_pure]

    def overlay(self, style=render.DEMO_STYLE, which="final"):
        """the winning mask painted over the image: uint8 [H,W,3] on the device, through ops.rle_paint on the encoded winner"""
        row = ops.rle_paint_style(**style) if isinstance(style, dict) else style
        return render.overlay(self.image, self.winners, order=[self.row + int(self._which(which))], style=row)

    def _explained(self):
        if self.explanation is None:
            raise RuntimeError("this Segmentation carries no explanation: build HybridGL(explain=True)")
        return self.explanation

    def heat_overlay(self, ramp="heat", outline=True, with_status=False):
        """the guided heat-map the scorer used -- min-max normalised, times the direction weight -- over the image (ops.heat_paint),
        with the final winner's outline on top (ops.rle_paint, the heat picture as its base): uint8 [H,W,3] on the device.
        with_status: (picture, status [1,4] int32 = code, bits of mn, mx, peak of ops.heat_paint)"""
        ex = self._explained()
        pics, _, status = render.heatmap_group([self.image], [ex.heat], [ex.dirflag], ramp=ramp)
        pic = pics[0]
        if outline:
            pic = render.overlay(pic, self.winners, order=[self.row + 1], style=ops.rle_paint_style(outline=OUTLINE_INK))
        return (pic, status) if with_status else pic

    def topk_order(self, k=3):
        """the k proposals with the highest score_clip, best LAST (the paint order): int32 [k] on the device, from a stable
        descending sort there -- the shortlist the final choice is drawn from when k is the pipeline's k1"""
        ex = self._explained()
        k = max(0, min(int(k), self.n_proposals))
        return torch.argsort(ex.score_clip, descending=True, stable=True)[:k].flip(0).to(torch.int32)

    def topk_overlay(self, k=3):
        """the k proposals with the highest score_clip over the image, in palette colours (the best is palette colour 0) with
        outlines, the best painted last: uint8 [H,W,3] on the device; the order never leaves it"""
        order = self.topk_order(k)
        n = int(order.numel())
        slots, table = ops.rle_encode(self.proposals.contiguous(), order)
        return render.overlay(self.image, (slots, table), style=render.proposal_styles(n)[::-1].copy() if n else None)


class HybridGL:
    """The three models, built once the way main.build_models builds them, behind one private ref-by-ref pipeline.  amg: the
    mask generator's settings over demo.py:44-54's (points_per_side=8, pred_iou_thresh=0.7, stability_score_thresh=0.7,
    crop_n_layers=0, crop_n_points_downscale_factor=1, min_mask_region_area=800); clip_checkpoint / sam_checkpoint / bpe_vocab:
    files in place of the packages' defaults.  explain: every Segmentation carries an Explanation (the pipeline's keep_explain).
    view_prompt: what CLIP is shown for a proposal (the pipeline's view_prompt: a struct, a preset name or a spec)."""

    def __init__(self, clip_model="ViT-B/16", sam_model="default", clip_checkpoint=None, sam_checkpoint=None, bpe_vocab=None,
                 precision=None, fusion_mode="G2L", heatmap="device", amg=None, device="cuda", explain=False,
                 view_prompt=None):
        from .backbone import CLIPViTFM
        from .main import AMG_DEFAULTS
        from .pipeline import HybridGLPipeline
        from .sam import SamAutomaticMaskGenerator, sam_model_registry
        from .tokenizer import SimpleTokenizer
        from .weights import CLIP_CONFIGS
        if heatmap not in ("device", "given"):
            raise ValueError(f"heatmap: {heatmap!r} ('device' or 'given')")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        precision = precision or ops.default_precision()
        settings = {k: v for k, v in AMG_DEFAULTS["refer"].items() if k != "group"}
        settings.update(amg or {})
        self.model = CLIPViTFM(model_name=clip_model, checkpoint=clip_checkpoint, device=self.device, precision=precision).eval()
        sam = sam_model_registry[sam_model](checkpoint=sam_checkpoint, device=self.device, precision=precision)
        self.generator = SamAutomaticMaskGenerator(sam, **settings)
        self.gem_model = None
        if heatmap == "device":
            from .gem import create_gem_model
            self.gem_model = create_gem_model(clip_model, clip=self.model)
        self.heatmap = heatmap
        self.tokenizer = SimpleTokenizer(bpe_vocab or None)
        self.context_length = CLIP_CONFIGS[clip_model]["context_length"]
        self._pipe = HybridGLPipeline(self.model, fusion_mode=fusion_mode, mask_generator=self.generator, use_sam_masks=True,
                                      gem_model=self.gem_model, k_clamp="per_ref", record_predictions=True,
                                      keep_explain=bool(explain), view_prompt=view_prompt)
        self._image = None      # (the caller's object, image id, sam_img, image_norm, tensor_img) of the last image
        self._calls = 0

    # ---- the item ----------------------------------------------------------------------------------------------------------
    def _tensors(self, image):
        """(image id, sam_img, image_norm, tensor_img) of `image`; the same object (or the same path) as last time is the same
        image: its id and its tensors are the last call's, and the pipeline's one-entry cache answers for everything that
        depends on the image alone"""
        from . import transforms as T
        last = self._image
        same = last is not None and (image is last[0] or (isinstance(image, str) and image == last[0]))
        if not same:
            sam_img = render._image_u8(image, self.device)
            norm = T.to_tensor_normalize(sam_img)
            timg = T.gem_img_transform(sam_img) if self.heatmap == "device" else None
            self._image = (image, (last[1] + 1) if last else 0, sam_img, norm, timg)
        return self._image[1:]

    def ref_batch(self, image, texts, parse=None):
        """the RefBatch of one call, as main.RealRefs.load builds it for a ref of the dataset (the ground truth aside)"""
        from .gem import GEMWrapper
        from .loader import pin_upload
        from .main import sentence_strings
        from .pipeline import RefBatch, Sentence
        from .tokenizer import tokenize
        texts = [texts] if isinstance(texts, str) else list(texts)
        parse = [parse] if isinstance(parse, dict) else list(parse or [])
        if not texts or (parse and len(parse) != len(texts)):
            raise ValueError(f"segment: {len(texts)} texts and {len(parse)} parse records")
        image_id, sam_img, image_norm, tensor_img = self._tensors(image)
        H, W = sam_img.shape[:2]
        dev = self.device
        strings, sents = [], []
        for k, raw in enumerate(texts):
            rec = dict(parse[k] or {}) if parse else {}
            if set(rec) - set(PARSE_KEYS):
                raise ValueError(f"parse record {k}: unknown keys {sorted(set(rec) - set(PARSE_KEYS))} (known: {list(PARSE_KEYS)})")
            raw = rec.get("sentence_for_spacy", raw)
            row = len(strings)
            others = list(rec.get("other_nouns", []))
            strings += sentence_strings(raw, rec)
            attn = gem_row = None
            if self.heatmap == "device":
                gem_row = len(strings)
                strings += GEMWrapper.prompts([rec.get("noun_phrase", raw)])
            else:
                attn = torch.ones((H, W), dtype=torch.float32, device=dev)     # uniform: no spatial guidance
            sents.append(Sentence(row, row + 1, list(range(row + 2, row + 2 + len(others))), rec.get("dirflag", "none"),
                                  rec.get("relaflag", "none"), len(others), attn, gem_row=gem_row))
        tokens = tokenize(strings, context_length=self.context_length, tokenizer=self.tokenizer)
        placeholder = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
        return RefBatch(sam_img, None, image_norm, placeholder, torch.zeros((1, 4), dtype=torch.int64, device=dev),
                        pin_upload(tokens, dev), torch.zeros((H, W), dtype=torch.uint8, device=dev), sents, None, image_id,
                        tensor_img=tensor_img, token_len=int(tokens.argmax(axis=1).max()) + 1, index=self._calls)

    # ---- the call ----------------------------------------------------------------------------------------------------------
    def segment(self, image, texts, parse=None):
        """image: uint8 [H,W,3] array, tensor or a path; texts: one string or a list; parse: one record per text (PARSE_KEYS),
        or None.  Returns one Segmentation per text.  pipeline.EmptyProposals when the mask generator keeps no proposal."""
        from .sam import strings_from_device
        texts = [texts] if isinstance(texts, str) else list(texts)
        ref = self.ref_batch(image, texts, parse)
        pipe = self._pipe
        for log in (pipe.iu_log, pipe.iu_owner, pipe.idx_log, pipe._pred_done):      # one call, one ref: nothing accumulates
            log.clear()
        pipe.step(ref)
        self._calls += 1
        n = len(texts)
        records = pipe.predictions()      # waits for the winners' runs; the indices are winning_indices()'s
        assert len(records) == n
        proposals = pipe.last_image()[1]
        H, W = ref.sam_img.shape[:2]
        idx = torch.stack(pipe.idx_log)      # [n,2] int32 on the device: the tail's own
        winners = ops.rle_encode(proposals, idx.reshape(-1), ops.rle_slot_words(H, W))
        strings = [{"size": [H, W], "counts": b.decode("ascii")} for b in strings_from_device(*winners, H, W)]
        kept = pipe.explained()
        assert len(kept) in (0, n)
        explain = [Explanation(e["heat"], e["dirflag"], e["black"], e["score_clip"], e["score_neg"], e["gem_score"]) for e in kept] or [None] * n
        return [Segmentation(texts[j], records[j]["pure_index"], records[j]["final_index"], strings[2 * j], strings[2 * j + 1],
                             int(proposals.shape[0]), ref.sam_img, proposals, winners, 2 * j, explain[j]) for j in range(n)]

    def all_proposals(self, seg):
        """every proposal of a Segmentation's image painted over it, largest area first (ties in stored order), in the
        palette with outlines: uint8 [H,W,3] on the device.  The order is sorted on the device and never read back."""
        return paint_all(seg.image, seg.proposals)


def paint_all(image, masks):
    """masks bool / uint8 [N,H,W] on the device over image uint8 [H,W,3]: every mask in its palette colour, half and half, with
    an outline; the largest first, so that small masks stay visible"""
    N = int(masks.shape[0])
    slots, table = ops.rle_encode(masks.contiguous(), None)
    order = torch.argsort(table[:, 2], descending=True, stable=True).to(torch.int32)      # the encoder's own areas
    return render.overlay(image, (slots, table), order=order, style=render.proposal_styles(N))


def scores_record(seg):
    """one text's explanation as plain numbers: the three score rows, both indices, and mn / mx / peak of the guided map"""
    ex = seg._explained()
    _, status = seg.heat_overlay(outline=False, with_status=True)
    st = status[0].cpu()
    mn, mx, peak = (float(v) for v in st[1:].view(torch.float32))
    return {"text": seg.text, "index_pure": seg.index_pure, "index_final": seg.index_final, "dirflag": ex.dirflag, "black": ex.black,
            "score_clip": ex.score_clip.cpu().tolist(), "score_neg": ex.score_neg.cpu().tolist(), "gem_score": ex.gem_score.cpu().tolist(),
            "status": {"code": int(st[0]), "mn": mn, "mx": mx, "peak": peak}}


def default_argument_parser():
    from .main import AMG_DEFAULTS
    p = argparse.ArgumentParser(prog="python -m hybridgl_amd.demo", description="segment one image by one sentence; write the overlay")
    p.add_argument("--image", required=True)
    p.add_argument("--text", required=True)
    p.add_argument("--out", required=True, help="PNG: the chosen mask painted over the image (demo.py:212-219)")
    p.add_argument("--which", default="final", choices=["final", "pure"])
    p.add_argument("--parse_json", default="", help="the sentence's parse record, or records keyed by the sentence")
    p.add_argument("--noun_phrase", default=None)
    p.add_argument("--other_nouns", nargs="*", default=None)
    p.add_argument("--dirflag", default=None)
    p.add_argument("--relaflag", default=None)
    p.add_argument("--all_proposals", default="", metavar="OUT2", help="PNG: every proposal, largest first, in palette colours")
    p.add_argument("--heat_out", default="", metavar="PNG", help="the guided heat-map over the image, the final winner outlined")
    p.add_argument("--topk_out", default="", metavar="PNG", help="the --topk proposals with the highest CLIP score, best last")
    p.add_argument("--topk", type=int, default=3, metavar="K")
    p.add_argument("--scores_json", default="", metavar="OUT", help="per text: the three score rows, both indices, the heat-map's mn / mx / peak")
    p.add_argument("--fusion_mode", default="G2L", choices=["G2L", "L2G", "G2L&L2G", "crop"])
    p.add_argument("--view_prompt", default="", metavar="SPEC_OR_PRESET",
                   help="what CLIP is shown for a proposal: a preset (hybridgl, black, gray, keep, red_circle, masked_crop, crop) or "
                        "key=value,... over one (ops.parse_view_prompt); a box window needs --fusion_mode crop")
    p.add_argument("--heatmap", default="device", choices=["device", "given"])
    p.add_argument("--clip_model", default="ViT-B/16")
    p.add_argument("--sam_model", default="default")
    p.add_argument("--bpe_vocab", default="")
    p.add_argument("--precision", default=None, choices=["f16x3", "f32", "f16"])
    for k, v in AMG_DEFAULTS["refer"].items():      # demo.py:44-54: the REFER scripts' settings
        if k != "group":
            p.add_argument("--" + k, type=type(v), default=None)
    p.add_argument("--box_nms_thresh", type=float, default=0.7)
    return p


def parse_record(args):
    """the one record of the command line: --parse_json (a record, or records keyed by the sentence), else the four flags"""
    flags = {k: getattr(args, k) for k in ("noun_phrase", "other_nouns", "dirflag", "relaflag") if getattr(args, k) is not None}
    if args.parse_json:
        import json
        if flags:
            raise SystemExit("--parse_json does not go with --noun_phrase / --other_nouns / --dirflag / --relaflag")
        doc = json.load(open(args.parse_json))
        return doc if set(doc) <= set(PARSE_KEYS) and doc else doc.get(args.text, {})
    return flags


def main(argv=None):
    from .main import AMG_DEFAULTS
    from .pipeline import EmptyProposals
    args = default_argument_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("hybridgl_amd.demo: no HIP device is visible (this package has no CPU implementation of the hot path)")
    amg = {k: getattr(args, k) for k in AMG_DEFAULTS["refer"] if k != "group" and getattr(args, k) is not None}
    amg["box_nms_thresh"] = args.box_nms_thresh
    rec = parse_record(args)
    hgl = HybridGL(args.clip_model, args.sam_model, bpe_vocab=args.bpe_vocab or None, precision=args.precision,
                   fusion_mode=args.fusion_mode, heatmap=args.heatmap, amg=amg,
                   explain=bool(args.heat_out or args.topk_out or args.scores_json), view_prompt=args.view_prompt or None)
    try:
        seg = hgl.segment(args.image, args.text, rec or None)[0]
    except EmptyProposals:
        print(f"no proposal survives the mask generator's filters on {args.image}: nothing to choose from", file=sys.stderr)
        return 2
    render.save_png(args.out, seg.overlay(which=args.which))
    print(f"{args.text!r}: proposal {seg.index_final} of {seg.n_proposals} (pure CLIP: {seg.index_pure}) -> {args.out}")
    if args.all_proposals:
        render.save_png(args.all_proposals, hgl.all_proposals(seg))
    if args.heat_out:
        render.save_png(args.heat_out, seg.heat_overlay())
    if args.topk_out:
        render.save_png(args.topk_out, seg.topk_overlay(args.topk))
    if args.scores_json:
        import json
        with open(args.scores_json, "w") as f:
            json.dump([scores_record(seg)], f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
