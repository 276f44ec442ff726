"""Per-ref evaluation step of Hybridgl_main.main (Hybridgl_main.py:79-230) on the GPU.

One `RefBatch` = one dataset item: an image, its mask proposals, its sentences (already
tokenised; the spaCy parse records are inputs -- an external package in the reference,
SURVEY.md 8c).  `HybridGLPipeline.step` runs, without any host synchronisation, the
reference's per-ref work:

    views   Hybridgl_main.py:93-125   hgl_synthesize_views
    hybrid  Hybridgl_main.py:128      hgl_clip_hybrid_forward
    text    Hybridgl_main.py:146-161  hgl_clip_encode_text (all strings of the ref in one batch)
    heat    Hybridgl_main.py:200-201  hgl_gem_image_features (once per image), hgl_gem_heatmap and
                                      hgl_resize_bilinear_aa (all sentences in one call) when a gem model is
                                      given; otherwise Sentence.imgattn is an input
    tail    Hybridgl_main.py:153-230  hgl_coherence_scores, hgl_score_sentence, hgl_iou_select

and accumulates cum_I/cum_U and the per-sentence IoUs on the device (Hybridgl_main.py:52-55,
240-247).  Metrics are read back once, at the end.
"""
import os
import time
from dataclasses import dataclass, field, replace
from typing import List, Optional

import numpy as np
import torch

from . import ops, synth
from .staging import HarvestQueue, PinnedPool


@dataclass
class Sentence:
    """One referring expression after the (external) spaCy pre-processing of
    Hybridgl_main.py:131-146,156,176: token rows index into RefBatch.tokens."""
    sentence_row: int
    noun_phrase_row: int
    other_noun_rows: List[int]
    dirflag: str = "none"          # extract_dir_phrase (utils.py:100-133)
    relaflag: str = "none"         # extract_rela_word  (utils.py:206-238)
    n_nouns: int = 0               # len(nouns) of extract_nouns (Hybridgl_main.py:184)
    imgattn: Optional[torch.Tensor] = None  # [H,W] fp32: gem_model(...) resized to the image (:200-202)
    target: Optional[torch.Tensor] = None   # [H,W] per-phrase ground truth (Hybridgl_main_PhraseCut.py:117-119); else RefBatch.target
    gem_row: Optional[int] = None  # token row of "a photo of a {noun_phrase}." (the GEM prompt) when the heat-map is computed here


@dataclass
class RefBatch:
    sam_img: torch.Tensor      # [H,W,3] uint8   image['sam_img']
    blurred: Optional[torch.Tensor]  # [H,W,3] uint8   cv2.GaussianBlur(sam_img,(15,15),0)  (:99); None = computed in the step
    image_norm: torch.Tensor   # [3,H,W] fp32    image['image'] (ImageNet-normalised)
    masks: torch.Tensor        # [N,H,W] bool    SAM proposals (:86-87)
    boxes: torch.Tensor        # [N,4] int64     XYWH (:89-90)
    tokens: torch.Tensor       # [T,77] int32    every string of the ref
    target: torch.Tensor       # [H,W] bool/uint8 ground truth
    sentences: List[Sentence] = field(default_factory=list)
    sam_resized: Optional[torch.Tensor] = None  # [h,w,3] uint8: sam_img after ResizeLongestSide (PIL, host)
    image_id: Optional[int] = None  # COCO image id.  CONTRACT: items with the same image_id carry the same image tensors
                                    # (sam_img, image_norm, tensor_img); with a mask generator their proposals, hybrid and GEM
                                    # features are computed once per image (unit merging in run(), the image cache, step()'s
                                    # one-entry cache).  With GIVEN proposals run() never merges items.
    tensor_img: Optional[torch.Tensor] = None   # [3,448,448] fp32: image['tensor_img'] = gem.get_gem_img_transform()(img)
    token_len: Optional[int] = None   # 1 + the largest EOT position of `tokens` (host knowledge of the tokenizer): the text
                                      # encoder then computes only that prefix of the 77 positions (exact: causal mask)
    index: Optional[int] = None       # position in the loader's order (Hybridgl_main.py:45,79); under sharding the metric rows
                                      # of all ranks are put back into this order (hybridgl_amd/dist.py)
    ready: Optional[object] = None    # torch.cuda.Event recorded behind the uploads of this item (hybridgl_amd/loader.py: the
                                      # copies run on a loader thread's stream); consumers make their stream wait for it


class EmptyProposals(RuntimeError):
    """the proposal stage kept no mask for this image"""


@dataclass
class _Live:
    """One image of a CLIP stage: its items, then an image-cache entry -- masks bool [n,H,W], boxes XYWH, hybrid features [n,E],
    GEM image features -- of which the stage computes what is still None."""
    refs: list
    masks: Optional[torch.Tensor]
    boxes: Optional[torch.Tensor]
    hybrid: Optional[torch.Tensor] = None
    gem: Optional[torch.Tensor] = None

@dataclass
class _Group:
    """A group in flight between run()'s stages: _sam_begin makes it, _sam_end adds props and ready, _clip_group consumes it."""
    LATE = object()              # in `held`: the group whose CLIP stage is enqueued next files this image's cache entry
    gid: int                     # its number in groups_run
    units: list
    held: list                   # per unit: the image-cache entry pinned at look-up (a later put may evict it from the dict),
                                 # LATE, or None (not cached -- or cached as "no proposals")
    fresh: Optional[list] = None     # the indices of the units that go through the generator
    state: object = None         # the generator's group state
    ev_enc: object = None        # the event behind its encoder pass
    props: Optional[list] = None     # per unit (masks u8 [n,H,W], boxes XYWH) or None = an image of the cache; no list: the items' own
    ready: object = None         # the event behind the proposal stage


def _adopt(ref, streams, produced=None):
    """An item whose tensors were produced on another stream than the ones that consume it -- uploaded on a loader thread's
    stream (RefBatch.ready), or built lazily on the caller's stream while the loop runs (`produced`: an event recorded
    there behind it): the consuming streams wait for that event, and the tensors are recorded on them so that the caching
    allocator does not hand their blocks to the next upload while a consumer still reads them."""
    ev = ref.ready if ref.ready is not None else produced
    if ev is None:
        return
    ts = [ref.sam_img, ref.blurred, ref.image_norm, ref.masks, ref.boxes, ref.tokens, ref.target, ref.sam_resized, ref.tensor_img]
    for s in ref.sentences:
        ts += [s.imgattn, s.target]
    for st in streams:
        st.wait_event(ev)
        for t in ts:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(st)


def _rows(text, rows):
    """rows of the text-feature matrix without a host->device index copy when they are consecutive."""
    if not rows:
        return None
    if list(rows) == list(range(rows[0], rows[0] + len(rows))):
        return text[rows[0]:rows[0] + len(rows)]
    return text.index_select(0, torch.as_tensor(rows, device=text.device)).contiguous()


def black_for(relaflag):
    """Hybridgl_main.py:211-216."""
    return 1.95 if relaflag == "big" else (1.5 if relaflag == "small" else 1.8)


_SIDE_STREAMS = {}


def _side_streams(device):
    """The three side streams of the loop (proposal stage, CLIP stage, text / GEM stage), ONE set per device for every
    pipeline object of the process: ops.workspace keeps one grow-only arena per (tag, stream), so pipelines that each
    brought their own streams would each leave ~30 GB of arenas behind (bench.py builds a dozen pipelines)."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = tuple(torch.cuda.Stream(dev) for _ in range(3))
    return _SIDE_STREAMS[key]


class HybridGLPipeline:
    def __init__(self, model, fusion_mode="G2L", masking_block=9, r=0.5, alpha=0.6, k1=3, k2=6, res=224,
                 mask_generator=None, use_sam_masks=False, fixed_proposals=None, cleanup_given_masks=False,
                 gem_model=None, k_clamp="persistent", image_cache=32, record_predictions=False, sweep=None,
                 on_overflow="raise", keep_explain=False, view_prompt=None):
        """mask_generator: a hybridgl_amd.sam.SamAutomaticMaskGenerator; when given, every step runs the
        SAM proposal stage (encoder, decoder, post-processing, NMS) on ref.sam_img first.
        use_sam_masks=False keeps ref.masks for the CLIP stage (fixed N; synthetic benchmark, where
        random SAM weights give an arbitrary number of proposals); True feeds the SAM proposals.
        k_clamp: "persistent" = the reference's quirk (Hybridgl_main.py:178-181: once an image yields fewer than k1 / k2
        proposals, k1 / k2 stay clamped for every LATER item of the process -- under sharding "later" means later on the
        same rank, so a run that meets such an image depends on the number of ranks); "per_ref" = the clamp applies
        to that item only (order- and sharding-independent; differs from the reference after such an image).
        record_predictions: keep every sentence's two winning masks as run lengths (predictions()): each tail is followed
        by one ops.rle_encode of the winners, selected by the tail's own device indices, and an asynchronous copy of the
        runs to pinned host memory -- no read-back of an index or a pixel, no synchronisation in the loop.
        sweep: a list of (r, alpha, k1, k2): every fused tail is followed by ONE ops.score_group_sweep call on the same operands
        that scores them under all these configurations (each with its own k1 / k2 under the k_clamp rule) and counts the
        proposal ceiling; sweep_rows() / ceiling_rows() / sweep_metrics() report them.  The pipeline's own configuration runs
        exactly as without a sweep.  A ref the fused tail cannot serve raises ValueError then.
        on_overflow: what run() does when an activation leaves the fp16 range in f16x3 / f16 mode.  "raise" (default): it
        raises ops.SplitOverflow at the offending group.  "rescue": the groups that were in flight are run again in f32 and
        the loop goes on (run()'s docstring; rescue_stats); step() and metrics() are the same in both modes.
        keep_explain: keep, on the device, what the tail of the most recent ref (step) or group (run) was given and what it
        computed per sentence -- explained(); nothing is computed or copied for it, and nothing changes with it off.
        view_prompt: what CLIP is shown for a proposal -- an ops.view_prompt struct, a preset name or a `key=value,...` spec
        (ops.parse_view_prompt).  None or the default prompt is the reference's pair of views through hgl_synthesize_views, as
        ever; anything else goes through hgl_synthesize_views_prompt with the proposals' boxes.  A box window moves the local
        view out of the frame the patch masks and the global stream live in, so it takes fusion_mode="crop"."""
        prompt = ops.parse_view_prompt(view_prompt)
        self.view_prompt = None if ops.view_prompt_is_default(prompt) else prompt
        if self.view_prompt is not None and self.view_prompt.window == 1 and fusion_mode != "crop":
            raise ValueError(f"view_prompt: a box window needs fusion_mode='crop', not {fusion_mode!r} (the patch masks and the "
                             "global view stay in the frame)")
        if k_clamp not in ("persistent", "per_ref"):
            raise ValueError("k_clamp must be 'persistent' or 'per_ref'")
        if on_overflow not in ("raise", "rescue"):
            raise ValueError("on_overflow must be 'raise' or 'rescue'")
        self.on_overflow = on_overflow
        self.keep_explain = bool(keep_explain)
        self._explained = []
        # run(on_overflow="rescue"): moved totals met, groups / refs done again in f32, and those refs' dataset positions
        self.rescue_stats = {"events": 0, "groups": 0, "refs": 0, "positions": []}
        self._rescue_bufs = PinnedPool()      # pinned int32 [3] snapshot buffers that are free
        self._rs = None           # the running loop's rescue state
        # run(): proposals, hybrid features and GEM features of the last `image_cache` images with an image_id (the dataset
        # yields one item per REF, Hybridgl_main.py:79, and the refs of an image are not always neighbours: RefCOCO has 2.6
        # refs per image).  0 = off.  Entries are device tensors: ~25 MB per 640 x 480 image with 64 proposals.
        self.image_cache = int(image_cache)
        self._img_cache = {}
        self._cache_cap = self.image_cache      # run() widens it to two groups
        self.cache_hits = 0
        # step(): (image id, image-cache entry) of the last image that had an id -- a cache of one, apart from _img_cache
        self._last = (None, (None, None, None, None))
        self.last_proposals = None      # what the proposal stage of the last step() / group returned
        # images skipped for want of a proposal; run(): groups begun, refs scored by the running call
        self.skipped = self.groups_run = self._done = 0
        self.collected = None      # run(collect=True): step()'s return value per ref
        self.group_marks = self.stage_marks = None      # opt-in timelines: a list assigned from outside switches one on
        self._s_sam = self._s_clip = self._s_text = self._ev = None      # _streams() makes them
        self.k_clamp = k_clamp
        # the per-sentence tail as ONE hgl_score_ref call per ref (HYBRIDGL_FUSED_TAIL=0: the per-sentence launches)
        self.fused_tail = os.environ.get("HYBRIDGL_FUSED_TAIL", "1") != "0"
        # run(): the tails of ALL refs of a group in one hgl_score_group call (HYBRIDGL_GROUP_TAIL=0: one hgl_score_ref per ref)
        self.group_tail = os.environ.get("HYBRIDGL_GROUP_TAIL", "1") != "0"
        self.stagger = os.environ.get("HYBRIDGL_STAGGER", "decoder")   # which part of the next group's SAM stage the CLIP stage runs beside
        self._k0 = (k1, k2)
        self.model = model
        self.gem_model = gem_model              # hybridgl_amd.gem.GEMWrapper: heat-maps computed on the device
        self.mask_generator = mask_generator
        self.use_sam_masks = use_sam_masks
        self.fixed_proposals = fixed_proposals
        self.cleanup_given_masks = cleanup_given_masks
        self.fusion_mode = fusion_mode
        self.masking_block = masking_block
        self.r, self.alpha, self.k1, self.k2 = r, alpha, k1, k2  # Hybridgl_main.py:57-63
        self.res = res
        dev = model.device
        # metric accumulators stay on the device: [cum_I, cum_U, cum_I_final, cum_U_final]
        self.cum = torch.zeros(4, dtype=torch.int64, device=dev)
        self.iu_log = []  # per sentence (IU_pure, IU_final) device tensors
        self.iu_owner = []  # per sentence (dataset position of its ref, sentence number)
        self.idx_log = []   # per sentence: device int32 [2] = (index of the pure-CLIP winner, index with spatial guidance)
        self._n_refs = 0
        self.record_predictions = bool(record_predictions)
        self._pred_free = PinnedPool()      # pinned staging buffers whose copies have completed
        self._pred_pending = HarvestQueue(self._pred_free)      # in log order: (ref position, sentences, H, W, slot words, pinned buffer)
        self._pred_done = []      # per sentence, in log order: ((H, W), counts of the pure winner, counts of the final one)
        self.sweep = None
        if sweep is not None:
            self.sweep = [(float(t[0]), float(t[1]), int(t[2]), int(t[3])) for t in sweep]
            if not self.sweep:
                raise ValueError("sweep: no configuration")
            self._sweep_k0 = [[t[2], t[3]] for t in self.sweep]
            self._sweep_k = [list(k) for k in self._sweep_k0]      # the clamp of Hybridgl_main.py:178-181, per configuration
            self.sweep_cum = torch.zeros((len(self.sweep), 4), dtype=torch.int64, device=dev)
            self.sweep_cum_ceiling = torch.zeros(2, dtype=torch.int64, device=dev)
            self._sweep_log = []      # per tail: (idx [C,S,2], iu [C,S,4], ceiling [S,3]) device tensors, in the order of iu_log

    def _views(self, r0, masks, boxes, out=None):
        """The two CLIP views of one image's proposals (Hybridgl_main.py:93-125): hgl_synthesize_views for the default prompt,
        hgl_synthesize_views_prompt with the proposals' boxes (XYWH, as the records carry them) for any other."""
        p = self.view_prompt
        blurred = None
        if p is None or p.global_bg == 0:
            blurred = r0.blurred if r0.blurred is not None else ops.gaussian_blur_u8(r0.sam_img, 15)   # :99
        if p is None:
            return ops.synthesize_views(r0.sam_img, blurred, r0.image_norm, masks, self.res, out=out)
        bx = ops.xywh_to_view_boxes(boxes) if ops.view_prompt_needs_boxes(p) else None
        return ops.synthesize_views_prompt(r0.sam_img, blurred, r0.image_norm, masks, p, boxes=bx, res=self.res, out=out)

    def _join_side_streams(self, cur, outs):
        """The caller's stream waits for both side streams; every tensor that leaves them is recorded on the caller's
        stream so that the caching allocator does not hand its block to later side-stream work while the caller reads it."""
        e1, e2 = torch.cuda.Event(), torch.cuda.Event()
        e1.record(self._s_sam)
        e2.record(self._s_clip)
        cur.wait_event(e1)
        cur.wait_event(e2)

        def rec(x):
            if isinstance(x, torch.Tensor):
                if x.is_cuda:
                    x.record_stream(cur)
            elif isinstance(x, (tuple, list)):
                for y in x:
                    rec(y)
        rec(outs)
        rec(self.last_proposals)

    def step(self, ref: RefBatch, run_sam=True):
        """One dataset item; returns the device tensors of the last sentence (idx, scores).
        run_sam=False: the proposal stage of this ref is not part of this call (it ran earlier / on another stream)."""
        _adopt(ref, (torch.cuda.current_stream(),))
        gen_here = self.mask_generator if run_sam else None
        # Per-image caching: the dataset yields one item per REF and the same image backs
        # several consecutive refs (Hybridgl_main.py:79); proposals, views and hybrid features depend on the
        # image only, so they are computed once per image.  Results are identical.
        from_gen = self.mask_generator is not None and self.use_sam_masks     # given proposals belong to the ITEM, not to the image
        hit = self._last[1] if ref.image_id is not None and self._last[0] == ref.image_id else (None, None, None, None)
        # (the GEM features are the image's whatever the source of the proposals)
        unit = _Live([ref], *hit) if from_gen else _Live([ref], None, None, gem=hit[3])
        # The text encoder (9 strings: small, latency-bound kernels) is independent of the image path: it runs on its
        # own stream underneath the SAM / CLIP image kernels and is joined before the scoring tail -- so the text half of
        # the stage is enqueued here, ahead of the proposal stage and its read-backs, and the rest of the stage after it.
        front = self._stage_text([unit], serial=False)
        if unit.hybrid is None:
            if gen_here is not None:
                # Hybridgl_main.py:85 mask_generator.generate(sam_img), kept on the device
                # a proposal store (hybridgl_amd/proposals.py) is keyed by the image id; SAM's own generator is called as ever
                by_id = {"image_id": ref.image_id} if getattr(gen_here, "wants_image_ids", False) else {}
                if self.use_sam_masks and getattr(gen_here, "crop_n_layers", 0) > 0:
                    # PhraseCut configuration (Hybridgl_main_PhraseCut.py:56-62): crop layers, cross-crop NMS
                    prop = gen_here.generate_device_crops(ref.sam_img, **by_id)[:4]
                elif self.use_sam_masks or self.fixed_proposals is not None:
                    prop = gen_here.generate_device(ref.sam_img, resized=ref.sam_resized,
                                                    fixed_n=self.fixed_proposals, **by_id)
                else:  # proposal kernels only, nothing read back
                    prop = gen_here.propose(ref.sam_img, resized=ref.sam_resized)
                if self.use_sam_masks:
                    if prop[0].shape[0] == 0:
                        self.skipped += 1
                        raise EmptyProposals("no proposals")
                    ref = replace(ref, masks=prop[0].view(torch.bool) if prop[0].dtype == torch.uint8 else prop[0],
                                  boxes=prop[1].contiguous())
                self.last_proposals = prop
                if self.cleanup_given_masks and not self.use_sam_masks:
                    # synthetic benchmark: the small-region clean-up runs on the proposal-shaped seeded masks
                    # (random-weight SAM logits are pixel noise, which is not what the clean-up sees in practice)
                    cm, _ = gen_here.cleanup_fixed(ref.masks.view(torch.uint8))
                    ref = replace(ref, masks=cm.view(torch.bool))
            unit.masks, unit.boxes = ref.masks, ref.boxes
        (out,) = self._stage([unit], front, now=True)
        if ref.image_id is not None:
            self._last = (ref.image_id, (unit.masks, unit.boxes, unit.hybrid, unit.gem) if from_gen else (None, None, None, unit.gem))
        return out

    def last_image(self):
        """(image id, masks bool [N,H,W], boxes XYWH [N,4]): the generator's proposals for the last image step() scored, which a
        step() on the same image id uses again; Nones before there is one, or when the proposals were the items' own."""
        return (self._last[0],) + self._last[1][:2]

    _DEFERRED = object()

    # ---- predictions: the winning masks of every sentence as run lengths (record_predictions=True) --------------------------
    def _record_tail(self, ref_index, n, masks, idx):
        """One ops.rle_encode of the 2n winners of a tail (idx [n,2]: the device tensor the tail wrote) and one asynchronous
        copy of table and slots into a pinned buffer, both on the current stream; nothing here waits for the device."""
        _, H, W = masks.shape
        sw = ops.rle_slot_words(H, W)
        flat = torch.empty(ops.rle_block_words("set", 2 * n, sw), dtype=torch.int32, device=masks.device)
        ops.rle_encode(masks, idx.reshape(-1), sw, out=flat)
        self._harvest_predictions()
        host = self._pred_free.take(flat.numel(), torch.int32)
        host[:flat.numel()].copy_(flat, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pred_pending.put(ev, (ref_index, n, H, W, sw, host), (host,))

    def _harvest_predictions(self, wait=False):
        """The copies that have completed (wait=True: all of them), oldest first, reduced to their counts arrays; their
        staging buffers return to the pool.  Host memory grows with the number of runs, not with pixels."""
        from .sam import counts_from_set
        for ref_index, n, H, W, sw, host in self._pred_pending.drain(wait):
            rows = counts_from_set(*ops.rle_split(host.numpy(), 2 * n, sw), H, W)      # copies: the buffer is reused
            for j in range(n):
                self._pred_done.append(((H, W), rows[2 * j], rows[2 * j + 1]))

    def predictions(self):
        """The winning masks of every sentence scored so far, ordered and keyed like partial_rows(): a list of
        {"index": dataset position, "sentence": sentence number, "pure_index", "final_index": the proposal indices of
        winning_indices(), "size": [H, W], "pure", "final": column-major run lengths (the `counts` of sam.mask_to_rle)}.
        Waits for the copies still in flight."""
        if not self.record_predictions:
            raise RuntimeError("predictions(): this pipeline does not record them; build it with record_predictions=True")
        self._harvest_predictions(wait=True)
        win = self.winning_indices()
        assert len(self._pred_done) == len(self.iu_owner) == len(win)
        return [{"index": int(o[0]), "sentence": int(o[1]), "pure_index": int(w[0]), "final_index": int(w[1]),
                 "size": [int(hw[0]), int(hw[1])], "pure": [int(v) for v in a], "final": [int(v) for v in b]}
                for o, w, (hw, a, b) in zip(self.iu_owner, win, self._pred_done)]

    # ---- explanations: what the tail of the most recent ref or group saw (keep_explain=True) --------------------------------
    def _explain(self, ref_index, recs, sc, sn, gm):
        """recs: per sentence (heat-map, dirflag, black); sc / sn / gm: per sentence the tail's score_clip, score_neg, gem_score [N]"""
        for j, (heat, dirflag, black) in enumerate(recs):
            self._explained.append({"index": ref_index, "sentence": j, "heat": heat, "dirflag": dirflag, "black": black,
                                    "score_clip": sc[j], "score_neg": sn[j], "gem_score": gm[j]})

    def explained(self):
        """Per sentence of the most recent ref (step) or group (run), in log order: {"index": dataset position, "sentence",
        "heat": the raw heat-map [H,W] the tail was given, "dirflag", "black", "score_clip", "score_neg", "gem_score": [N]},
        device tensors all; the fused tail and the per-sentence tail fill the same values.  Empty without keep_explain."""
        return list(self._explained)

    def _flush_tails(self, defer):
        """the deferred tails of a group's refs in one hgl_score_group call; returns each ref's last-sentence tensors, in order"""
        outs = ops.score_group(defer, self.model.model._logit_scale_exp, self.r, self.alpha, cum=self.cum, want_scores=True)
        if self.sweep is not None:
            self._sweep_tails(defer)
        last = [self._file_tail(q, out) for q, out in zip(defer, outs)]
        defer.clear()
        return last

    def _sweep_tails(self, refs):
        """the same tails (the dicts handed to ops.score_group, each with its sweep_k) under every configuration of the sweep"""
        outs = ops.score_group_sweep([dict(q, k1=[k[0] for k in q["sweep_k"]], k2=[k[1] for k in q["sweep_k"]]) for q in refs],
                                     [t[:2] for t in self.sweep], self.model.model._logit_scale_exp, cum=self.sweep_cum,
                                     cum_ceiling=self.sweep_cum_ceiling)
        self._sweep_log.extend(outs)

    def _score_ref(self, ref, hybrid, text, heat, defer=None):
        """the per-sentence tail of Hybridgl_main.py:153-230 for one ref; returns the tensors of its last sentence.  defer (a
        list): a ref whose tail the fused kernels serve is appended to it instead (for _flush_tails) and _DEFERRED returned"""
        scale = self.model.model._logit_scale_exp
        ref_index, fused = self._ref_state(ref, hybrid.shape[0], text)
        if fused is None:
            return None
        heats = iter(heat) if heat is not None else None
        q = self._request(ref, hybrid, text, [s.imgattn if s.imgattn is not None else next(heats) for s in ref.sentences], ref_index)
        if fused and defer is not None:
            defer.append(q)
            return self._DEFERRED
        if fused:
            # hgl_score_ref: every mask byte read once for all sentences' heat-maps, one scoring workgroup per sentence,
            # both IoUs of every sentence and the accumulators of Hybridgl_main.py:52-55 in the same four launches
            out = ops.score_ref(hybrid, text, ref.boxes, ref.masks, q["sentences"], scale, self.r, q["k1"], q["k2"], self.alpha,
                                cum=self.cum, want_scores=True)
            if self.sweep is not None:
                self._sweep_tails([q])
            return self._file_tail(q, out)
        out = [], [], [], [], []      # per sentence: idx [2], (IU_pure, IU_final), score_clip, score_neg, gem_score
        for s, r in zip(ref.sentences, q["sentences"]):
            gem = ops.coherence_scores(r["imgattn"], ref.masks, r["dirflag"], r["black"])
            idx, sc, sn = ops.score_sentence(hybrid, text[s.sentence_row], text[s.noun_phrase_row], _rows(text, s.other_noun_rows),
                                             ref.boxes, gem, scale, self.r, q["k1"], q["k2"], self.alpha, r["relaword"],
                                             r["has_other_nouns"])
            iu0 = ops.iou_select(ref.masks, idx, 0, r["target"])
            iu1 = ops.iou_select(ref.masks, idx, 1, r["target"])
            self.cum[0:2] += iu0
            self.cum[2:4] += iu1
            for col, v in zip(out, (idx, (iu0, iu1), sc, sn, gem)):
                col.append(v)
        return self._file_tail(q, out)

    def _ref_state(self, ref, n, text):
        """What a ref with n proposals changes before its tail, whichever route serves it: the k1 / k2 clamp and the count of refs
        -> (its dataset position, whether the fused kernels serve it -- None for a ref without a sentence)."""
        # the k1/k2 clamp of Hybridgl_main.py:178-181 persists across refs in the reference
        if self.k_clamp == "per_ref":
            self.k1, self.k2 = self._k0
        self.k1 = min(self.k1, n)
        self.k2 = min(self.k2, n)
        if self.sweep is not None:      # the same rule for every configuration's own pair
            if self.k_clamp == "per_ref":
                self._sweep_k = [list(k) for k in self._sweep_k0]
            self._sweep_k = [[min(k[0], n), min(k[1], n)] for k in self._sweep_k]
        ref_index = ref.index if ref.index is not None else self._n_refs
        self._n_refs += 1
        if not ref.sentences:        # an item without a sentence scores nothing (the reference's inner loop does not run)
            return ref_index, None
        fused = self.fused_tail and text.is_contiguous() and all(
            list(s.other_noun_rows) == list(range(s.other_noun_rows[0], s.other_noun_rows[0] + len(s.other_noun_rows)))
            for s in ref.sentences if s.other_noun_rows)
        if self.sweep is not None and not fused:
            raise ValueError(f"sweep: the fused tail cannot serve ref {ref_index} (other-noun rows that are not consecutive, text "
                             "that is not contiguous, or HYBRIDGL_FUSED_TAIL=0), and the sweep runs on the fused tail's operands")
        return ref_index, fused

    def _request(self, ref, hybrid, text, attn, ref_index):
        """One ref's tail as ops.score_ref / ops.score_group / _sweep_tails take it, under the clamp as it stands; attn: the
        heat-map of every sentence.  (other_row0 / n_other mean something only to the fused kernels, which take consecutive rows.)"""
        recs = [dict(sentence_row=s.sentence_row, noun_phrase_row=s.noun_phrase_row,
                     other_row0=s.other_noun_rows[0] if s.other_noun_rows else 0, n_other=len(s.other_noun_rows),
                     dirflag=s.dirflag, relaword=s.relaflag, has_other_nouns=s.n_nouns != 0, black=black_for(s.relaflag),
                     imgattn=a if a.is_contiguous() else a.contiguous(), target=s.target if s.target is not None else ref.target)
                for s, a in zip(ref.sentences, attn)]
        q = dict(hybrid=hybrid, text=text, boxes=ref.boxes, masks=ref.masks, sentences=recs, k1=self.k1, k2=self.k2, ref_index=ref_index)
        if self.sweep is not None:
            q["sweep_k"] = self._sweep_k
        return q

    def _file_tail(self, q, out):
        """A finished tail (q: its request) into the logs; out = (idx, iu, score_clip, score_neg, gem_score), per sentence: a fused
        tail's tensors or the per-sentence route's lists with iu as (IU_pure, IU_final) pairs.  Returns the last sentence's."""
        idx, iu, sc, sn, gm = out
        self._log_tail(q["ref_index"], len(q["sentences"]), idx, iu, q["masks"])
        if self.keep_explain:
            self._explain(q["ref_index"], [(r["imgattn"], r["dirflag"], r["black"]) for r in q["sentences"]], sc, sn, gm)
        return idx[-1], sc[-1], sn[-1], gm[-1]

    def _log_tail(self, ref_index, n, idx, iu, masks=None):
        for j in range(n):
            self.iu_log.append((iu[j, 0:2], iu[j, 2:4]) if torch.is_tensor(iu) else iu[j])
            self.iu_owner.append((ref_index, j))
            self.idx_log.append(idx[j])
        if self.record_predictions:
            self._record_tail(ref_index, n, masks, idx if torch.is_tensor(idx) else torch.stack(idx))

    # ---- the evaluation loop at the grouped rate ----------------------------------------------------------------------
    def _streams(self):
        if self._s_sam is None:
            self._s_sam, self._s_clip, self._s_text = _side_streams(self.model.device)
            self._ev = torch.cuda.Event()
        return self._s_sam, self._s_clip

    @staticmethod
    def _units(loader, group, merge=True):
        """Groups of up to `group` IMAGE UNITS in the loader's order; a unit = the consecutive items that share an
        image_id (the dataset yields one item per ref, Hybridgl_main.py:79; proposals, views and hybrid features depend on
        the image only).  Items without an image_id are units of their own; merge=False makes every item its own unit
        (proposals GIVEN per item: two items of one image may carry different masks / boxes, and a unit uses its first
        item's)."""
        units, cur = [], None
        for ref in loader:
            if ref is None:      # an item the dataset filtered out entirely (PhraseCut seen / unseen modes)
                continue
            if merge and cur is not None and ref.image_id is not None and ref.image_id == cur[0].image_id:
                cur.append(ref)
                continue
            if cur is not None:
                units.append(cur)
                if len(units) == group:
                    yield units
                    units = []
            cur = [ref]
        if cur is not None:
            units.append(cur)
        if units:
            yield units

    @staticmethod
    def balanced_group(total, group):
        """The group size run() uses for `total` items at most `group` at a time: the same number of groups, equally
        full (20 refs, group 16 -> 10 + 10 instead of 16 + 4: the proposal stage of the second group then has a CLIP stage
        of its own size beside it, and no stage meets a shape it has not seen)."""
        total, group = int(total), max(int(group), 1)
        if total <= group:
            return max(total, 1)
        n_groups = -(-total // group)
        return -(-total // n_groups)

    def prepare(self, group=16, H=640, W=640, proposals=64, n_sent=3, tail=None, serial=False, slack=1 << 30):
        """Everything run() would otherwise do on first use, done once, up front: every grow-only workspace (ops.workspace,
        one arena per stage and stream) and every block of the caching allocator sized for a full group of `group` images
        of H x W with up to `proposals` masks each AND for a ragged last group of `tail` images (default: a quarter of a
        group); every kernel instantiation, LDS reservation and per-shape table of those two group sizes touched.  After
        it, the first run() costs what the hundredth does, whatever the length of the caller's warm-up.  It runs the
        product loop itself on seeded synthetic items (synthetic_ref), so nothing can be missed by construction; metric
        rows, logs and the image cache are restored afterwards.  ~1 s per call at the benchmark geometry."""
        dev = self.model.device
        gen = self.mask_generator
        tail = max(1, group // 4) if tail is None else int(tail)
        use_gem = self.gem_model is not None
        items = [synthetic_ref(90000 + j, dev, N=proposals, H=H, W=W, n_sent=n_sent, sam_img_size=1024 if gen is not None else 0,
                               gem=use_gem, device_blur=True)[0] for j in range(min(group, 4))]
        if self.record_predictions:      # what the loop has recorded so far is filed before the rehearsal's records are dropped
            self._harvest_predictions(wait=True)
        keep = self._checkpoint()
        extras = (self.groups_run, self.group_marks, self.stage_marks, dict(self.rescue_stats, positions=list(self.rescue_stats["positions"])))
        self.group_marks = self.stage_marks = None
        cap = proposals if (gen is not None and self.use_sam_masks) else None
        try:
            # two full groups (the second one's proposal stage runs beside the first one's CLIP stage: both streams' arenas
            # reach their steady size), then a ragged group
            for n in (2 * group, tail):
                self.run((items[i % len(items)] for i in range(n)), group=group, proposal_cap=cap, serial=serial)
            if cap is not None:
                # the generator decides how many masks the synthetic images yield; the CLIP stage is sized for the full
                # `proposals` per image by one more pass over the items' own (seeded) masks
                self.use_sam_masks = False
                try:
                    for n in (group, tail):
                        self.run((items[i % len(items)] for i in range(n)), group=group, serial=serial)
                finally:
                    self.use_sam_masks = True
            torch.cuda.synchronize(dev)
            # The caching allocator keeps one pool per stream and the loop's tensors differ a little from group to group (the
            # number of proposals is data): leave `slack` bytes of cached, splittable blocks behind on every stream of the loop
            # so that a request a few MB above anything seen here is served from the pool, not by hipMalloc in the middle of a
            # group (sized for 288 GB of HBM: 4 x 1 GiB is 1.4 % of the device)
            if slack > 0:
                streams = [torch.cuda.current_stream(dev)] + ([] if serial else list(self._streams()) + [self._s_text])
                for st in streams:
                    with torch.cuda.stream(st):
                        blocks = [torch.empty(int(slack) // 2, dtype=torch.uint8, device=dev) for _ in range(2)]
                        del blocks
            torch.cuda.synchronize(dev)
        finally:
            self._rollback(keep)      # (the predictions' staging buffers stay, sized for this geometry; the records go)
            self.groups_run, self.group_marks, self.stage_marks, self.rescue_stats = extras
        return self

    def run(self, loader, group=16, proposal_cap=None, collect=False, serial=False, total=None):
        """The loop of Hybridgl_main.py:79-230 over a whole loader, taken `group` images at a time on two streams:

            SAM stream   group g+1: ONE encoder pass over its images, per image decoder + post-processing + NMS, small-region
                         clean-up + second NMS (SamAutomaticMaskGenerator.group_begin / group_cleanup / group_finish: the
                         survivor counts of the whole group are read back in TWO device->host copies, not 2 per image)
            CLIP stream  group g: one text-encoder batch over the strings of all its refs, one GEM tower pass over its
                         images, one hybrid forward over the ACTUAL proposals of all its images (ragged counts, images of
                         different sizes), then the per-sentence tail of every ref in the loader's order

        The CLIP stage of group g is enqueued before the host waits for the counts of group g+1, so the device always has
        work.  `loader` yields RefBatch items (device tensors; hybridgl_amd.loader.Prefetcher prepares them on background
        threads, Hybridgl_main.py:45).  Results per ref are those of step() -- every mask row, string and image is
        independent -- up to the summation order of the SAM encoder's split-K, which only a single-image pass uses.
        Without a mask generator (or with run_sam=False semantics: use_sam_masks=False and no generator) the proposals are
        RefBatch.masks / boxes.  Images for which the generator keeps no mask are skipped and counted (self.skipped; the
        reference would fail on them).  Returns the number of refs scored; collect=True also keeps step()'s per-ref
        return values in self.collected.  serial=True: the same work with every stage on the CURRENT stream, back to back
        (per-kernel timing with events on one stream).  total: the number of items the loader will yield, when known -- the
        groups are then equally full (balanced_group) instead of full groups and a remainder.

        on_overflow="rescue" (and a model in f16x3 / f16): every group is a transaction (hybridgl_amd/rescue.py).  Behind
        each CLIP stage the CLIP stream waits for the proposal stage beside it and copies the three range counters to pinned
        memory (ops.split_overflow_snapshot); the next proposal stage starts behind that copy, so the copy sees the same
        work in every run.  The host reads it one group later.  An unchanged total commits the group; a moved one drains the
        device, rolls the logs, accumulators, clamp and image cache back to the checkpoint before the oldest uncommitted
        group (at most three are), clears the counters and runs those groups again under ops.forced_precision("f32"),
        serially on the current stream, proposal stage included.  The loop then goes on in the models' own precision with an
        empty pipeline.  What the f32 re-run files in the image cache is used by later groups like any other entry.
        run() ends by waiting for the verdict on its last groups.  A ProposalRecorder as the generator is refused in this mode
        (ValueError): its files are no part of the roll-back.  self.rescue_stats counts events, groups, refs and the
        dataset positions done again; groups_run counts the loop's groups, not re-runs."""
        gen = self.mask_generator
        if total is not None:
            group = self.balanced_group(total, group)
        cur = torch.cuda.current_stream()
        serial = bool(serial)
        if serial:
            s_sam = s_clip = cur
        else:
            s_sam, s_clip = self._streams()
        led = None
        if self._rescue_wanted():
            from .proposals import ProposalRecorder
            from .rescue import RescueLedger
            if isinstance(gen, ProposalRecorder):
                # its files and its list of the images it has written are no part of _checkpoint / _rollback: the store would
                # keep the proposals of the pass a rescue has just rejected
                raise ValueError("on_overflow='rescue' cannot run with a ProposalRecorder (--save_proposals): a rolled-back group's "
                                 "proposals would stay in the store; record the store with on_overflow='raise'")
            led = RescueLedger()
            # the total the loop starts from, in stream order before anything of this run
            self._rs = dict(snaps=[], gate=None, base=self._snapshot(None, cur), cap=proposal_cap, group=group, cur=cur,
                            s_sam=s_sam, s_clip=s_clip, serial=serial)
        if not serial:
            self._ev.record(cur)
            s_sam.wait_event(self._ev)
            s_clip.wait_event(self._ev)
        self.collected = [] if collect else None
        self._done = 0
        pending = None
        # items of one image are merged into a unit only when the proposals come from the generator (then they are a function
        # of the image); with given proposals every item keeps its own masks / boxes, as step() does
        it = iter(self._units(loader, group, merge=gen is not None and self.use_sam_masks))
        # the three-word read-back is switched on at the object that makes the read-back, and only there: a wrapper that hands
        # attribute reads on to its generator would answer for it and keep the assignment to itself
        snapshot_was = vars(gen).get("overflow_snapshot") if led is not None and hasattr(gen, "__dict__") else None
        if snapshot_was is not None:
            gen.overflow_snapshot = True
        try:
            for units in it:
                self.groups_run += 1
                if self.group_marks is not None:      # host-side stamp of every group boundary (tools/first_use.py)
                    self.group_marks.append(time.perf_counter())
                produced = None
                if not serial:      # items a lazy loader built on the caller's stream just now
                    produced = torch.cuda.Event()
                    produced.record(cur)
                for u in units:
                    for r in u:
                        _adopt(r, (s_sam, s_clip), produced)
                if led is not None:
                    led.open(self.groups_run, units)
                    if self._rs["gate"] is not None and not serial:      # no proposal stage beside a snapshot
                        s_sam.wait_event(self._rs["gate"])
                g = self._sam_begin(self.groups_run, units, pending, s_sam, proposal_cap, serial, group)
                if pending is not None:
                    with torch.cuda.stream(s_clip):
                        if g.ev_enc is not None:
                            s_clip.wait_event(g.ev_enc)
                        self._clip_group(pending, serial, led)
                seen = self._sam_end(g, s_sam, led is not None)
                enqueued = pending.gid if pending is not None else None      # the group whose CLIP stage went out just now
                pending = g
                if led is not None:
                    if self._rescue_judge(led, it, seen):
                        pending = None
                    elif enqueued is not None:
                        self._rescue_stage_end(enqueued, g.ready)
            if pending is not None:
                with torch.cuda.stream(s_clip):
                    self._clip_group(pending, serial, led)
                if led is not None:
                    self._rescue_stage_end(pending.gid, None)
            if led is not None:
                self._rescue_judge(led, it, None)
        finally:
            if led is not None:
                self._rs = None
                if snapshot_was is not None:
                    gen.overflow_snapshot = snapshot_was
        if not serial:
            self._join_side_streams(cur, self.collected)
        return self._done

    def _sam_begin(self, gid, units, pending, s_sam, proposal_cap, serial, group):
        """The image-cache look-up of a group and everything of its proposal stage up to the first count read-back, enqueued on
        s_sam without a wait -> the _Group (held, fresh, the generator's group state and the event behind its encoder pass)."""
        gen = self.mask_generator
        # images seen lately (or in the group whose CLIP stage is about to be enqueued: it files them before this
        # group's CLIP stage looks): no proposal stage, no hybrid forward for them
        cached = [False] * len(units)
        g = _Group(gid, units, held=[None] * len(units))
        if self.image_cache > 0 and gen is not None and self.use_sam_masks:
            self._cache_cap = max(self.image_cache, 2 * group)
            in_pending = {u[0].image_id for u in pending.units} if pending is not None else set()
            for i, u in enumerate(units):
                iid = u[0].image_id
                if iid is None:
                    continue
                if iid in self._img_cache:
                    cached[i], g.held[i] = True, self._img_cache[iid]
                elif iid in in_pending:
                    cached[i], g.held[i] = True, g.LATE
        fresh = g.fresh = [i for i, c in enumerate(cached) if not c]
        if gen is not None and fresh:
            with torch.cuda.stream(s_sam):
                self._stage_mark("sam_begin")
                imgs = [units[i][0].sam_img for i in fresh]
                if self.use_sam_masks:
                    # stagger = "decoder": the CLIP stage of the previous group starts when THIS group's encoder pass
                    # is through, so its large GEMMs run beside the latency-bound rest of the proposal stage (decoder,
                    # post-processing, NMS, clean-up) instead of beside the encoder's equally matrix-bound GEMMs
                    if self.stagger == "decoder" and not serial:
                        g.ev_enc = torch.cuda.Event()
                    # everything of the group up to its first count read-back is enqueued here without a wait (with crop
                    # layers, the PhraseCut configuration: every crop of every image); the read-backs come after the CLIP
                    # stage of the previous group has been enqueued
                    if getattr(gen, "wants_image_ids", False):      # a store is keyed by the image, not by its pixels
                        g.state = gen.group_begin(imgs, proposal_cap, g.ev_enc, image_ids=[units[i][0].image_id for i in fresh])
                    else:
                        g.state = gen.group_begin(imgs, proposal_cap, g.ev_enc)
                else:    # proposal kernels only; their output is not consumed (synthetic benchmark, seeded masks)
                    self.last_proposals = gen.propose_batch(imgs)[-1]
                    if self._rs is not None and not serial:      # the stage-end snapshot beside it waits for this (no `ready` here)
                        self._rs["beside"] = torch.cuda.Event()
                        self._rs["beside"].record(s_sam)
        return g

    def _sam_end(self, g, s_sam, rescue=False):
        """The rest of a group's proposal stage: waits for its counts and enqueues what they decide -- g.props and g.ready, the
        event behind the stage -> the range counters' total that rode on the read-back (rescue mode and a generator that
        takes ops.split_overflow_snapshot there) or None."""
        gen = self.mask_generator
        units, seen = g.units, None
        if g.state is not None:
            with torch.cuda.stream(s_sam):
                stc = gen.group_cleanup(g.state)
                if rescue:
                    seen = int(stc.overflow) if getattr(gen, "__dict__", {}).get("overflow_snapshot", False) else None
                elif stc.overflow:
                    # fail at THIS group, not in metrics() after the whole dataset: the counter rode on the group's
                    # count read-back (everything the device had finished by then, on any stream).  The counters are
                    # process-global: cleared here, or every later run() of the process -- the f32 rerun this message
                    # recommends included -- would trip over the same count at its first group
                    ops.split_overflow_count(reset=True)
                    raise ops.SplitOverflow(
                        f"activations exceeded the fp16 range (|x| > 65504) in f16x3 / f16 mode by group {self.groups_run} of the "
                        f"loop ({stc.overflow} GPU threads saw one; refs up to dataset position {units[-1][-1].index}): the "
                        "results from the previous group on contain inf / NaN; rerun with HYBRIDGL_PRECISION=f32 (or precision='f32')")
                got = [p[:2] for p in gen.group_finish(stc)]
                g.ready = torch.cuda.Event()
                g.ready.record(s_sam)
                self._stage_mark("sam_end")
            g.props = [None] * len(units)          # None = take it from the image cache
            for i, pr in zip(g.fresh, got):
                g.props[i] = pr
        elif len(g.fresh) < len(units):
            g.props = [None] * len(units)
        return seen

    # ---- checkpoint and roll-back of everything a stage appends to or adds into (prepare(), on_overflow="rescue") -------------
    def _checkpoint(self):
        """The loop's state as of now; the accumulators are cloned on the current stream, the logs are append-only and kept as
        lengths.  step()'s last-image record is no part of it: run(), and so a rescue inside it, never touches it."""
        cp = dict(cum=self.cum.clone(), n_log=len(self.iu_log), n_refs=self._n_refs, skipped=self.skipped,
                  cache=dict(self._img_cache), cache_hits=self.cache_hits, k=(self.k1, self.k2), done=self._done,
                  collected=len(self.collected) if self.collected is not None else None,
                  n_pred=len(self._pred_done) + sum(p[1] for p in self._pred_pending))      # sentences recorded, filed or in flight
        if self.sweep is not None:
            cp["sweep"] = (self.sweep_cum.clone(), self.sweep_cum_ceiling.clone(), len(self._sweep_log), [list(k) for k in self._sweep_k])
        return cp

    def _rollback(self, cp):
        """Back to _checkpoint()'s state.  The caller has made sure that the device work since then has ended (or orders it before
        the copies enqueued here on the current stream).  Image-cache entries put since then leave, those evicted since then
        return; the staging buffers of the predictions stay, their records go."""
        self.cum.copy_(cp["cum"])
        n = cp["n_log"]
        del self.iu_log[n:], self.iu_owner[n:], self.idx_log[n:]
        self._n_refs, self.skipped, self._done = cp["n_refs"], cp["skipped"], cp["done"]
        self._img_cache, self.cache_hits = cp["cache"], cp["cache_hits"]
        self.k1, self.k2 = cp["k"]
        if cp["collected"] is not None and self.collected is not None:
            del self.collected[cp["collected"]:]
        if self.sweep is not None:
            self.sweep_cum.copy_(cp["sweep"][0])
            self.sweep_cum_ceiling.copy_(cp["sweep"][1])
            del self._sweep_log[cp["sweep"][2]:]
            self._sweep_k = cp["sweep"][3]
        if self.record_predictions:
            self._harvest_predictions(wait=True)
            del self._pred_done[cp["n_pred"]:]

    # ---- on_overflow="rescue": the device side of hybridgl_amd/rescue.py --------------------------------------------------------
    def _rescue_wanted(self):
        """rescue mode, and a model of the loop that splits into fp16 planes (with f32 models the mode is a no-op)"""
        if self.on_overflow != "rescue":
            return False
        owners = [getattr(w, "model", None) for w in (self.model, self.gem_model, self.mask_generator)]
        return any(ops.split_mode(getattr(o, "precision", "f32")) for o in owners if o is not None)

    def _snapshot(self, gid, stream):
        """(gid, pinned int32 [3], event): the three range counters as of this point of `stream`, nothing waited for"""
        buf = self._rescue_bufs.take(3, torch.int32)
        with torch.cuda.stream(stream):
            ops.split_overflow_snapshot(buf)
            ev = torch.cuda.Event()
            ev.record(stream)
        return gid, buf, ev

    def _snapshot_total(self, snap):
        _, buf, ev = snap
        ev.synchronize()
        total = sum(int(v) for v in buf.tolist())
        self._rescue_bufs.give(buf)
        return total

    def _rescue_stage_end(self, gid, ready):
        """The snapshot behind the CLIP stage of group gid (just enqueued), taken when the proposal stage beside it (`ready`) has
        ended as well; the next proposal stage waits for it (run()), so it counts the same work in every run."""
        rs = self._rs
        beside = rs.pop("beside", None)      # proposal kernels whose output nobody consumes (use_sam_masks=False with a generator)
        for ev in (ready, beside):
            if ev is not None and not rs["serial"]:
                rs["s_clip"].wait_event(ev)
        snap = self._snapshot(gid, rs["s_clip"])
        rs["snaps"].append(snap)
        rs["gate"] = snap[2]

    def _rescue_judge(self, led, it, seen):
        """The verdicts that are due: the stage-end snapshots enqueued a group ago (at the end of run(): all of them), oldest
        first, then the total `seen` on the newest group's read-back.  True: groups were re-run, the pipeline is empty."""
        rs = self._rs
        if rs["base"] is not None:
            led.base, rs["base"] = self._snapshot_total(rs["base"]), None
        while rs["snaps"]:
            snap = rs["snaps"].pop(0)
            d = led.stage_end(snap[0], self._snapshot_total(snap))
            if d.kind == "rescue":
                self._rescue(led, d, it)
                return True
        if seen is not None:
            d = led.read_back(seen)
            if d.kind == "rescue":
                self._rescue(led, d, it)
                return True
        return False

    def _rescue(self, led, d, it):
        """A total moved: drain, roll back, clear the counters, run the groups in flight again in f32 on the current stream."""
        rs = self._rs
        cur, dev = rs["cur"], self.model.device
        if d.pull_next:      # (rescue.py: the decision the next stage-end snapshot would have led to)
            nxt = next(it, None)
            if nxt is not None:
                self.groups_run += 1
                led.open(self.groups_run, nxt)
        torch.cuda.synchronize(dev)
        for snap in rs["snaps"]:
            self._rescue_bufs.give(snap[1])
        rs["snaps"], rs["gate"] = [], None
        cp = led.oldest_checkpoint()
        if cp is not None:
            self._rollback(cp)
        ops.split_overflow_count(reset=True, sync=False)      # the device is idle
        gids = led.in_flight()
        stats = self.rescue_stats
        stats["events"] += 1
        with torch.cuda.stream(cur), ops.forced_precision("f32"):
            for gid in gids:
                units = led.payload(gid)
                here = torch.cuda.Event()
                here.record(cur)
                for u in units:
                    for r in u:
                        _adopt(r, (cur,), here)
                g = self._sam_begin(gid, units, None, cur, rs["cap"], True, rs["group"])
                self._sam_end(g, cur, True)
                self._clip_group(g, serial=True)
                stats["groups"] += 1
                for u in units:
                    stats["refs"] += len(u)
                    stats["positions"] += [r.index for r in u]
        led.rescued(0)
        if not rs["serial"]:
            # the loop's streams go on behind the re-run; what it filed in the image cache is read on the CLIP stream from now on
            for entry in self._img_cache.values():
                for t in entry or ():
                    if isinstance(t, torch.Tensor):
                        t.record_stream(rs["s_clip"])
            self._ev.record(cur)
            rs["s_sam"].wait_event(self._ev)
            rs["s_clip"].wait_event(self._ev)

    def _clip_group(self, g, serial, led=None):
        """CLIP + scoring stage of one group on the current stream: its units resolved against the proposal stage's output
        and the image cache, the stage over those that have proposals, their entries filed in the image cache, the refs
        counted in _done.  In rescue mode (led) the checkpoint before the group is taken first."""
        if led is not None:
            led.checkpoint(g.gid, self._checkpoint())
        units, props, held = g.units, g.props, g.held
        cur = torch.cuda.current_stream()
        if g.ready is not None:
            cur.wait_event(g.ready)
        self._stage_mark("clip_begin")
        gen, live = self.mask_generator, []
        for i, refs in enumerate(units):
            if props is not None and props[i] is None:      # an image of the cache
                hit = self._img_cache.get(refs[0].image_id) if held[i] is g.LATE else held[i]
                if hit is None:                              # filed as "no proposals"
                    self.skipped += len(refs)
                    continue
                self.cache_hits += 1
                live.append(_Live(refs, *hit))
            elif props is not None:
                mk, bx = props[i]
                if mk.shape[0] == 0:
                    self.skipped += len(refs)
                    if self.image_cache > 0 and refs[0].image_id is not None:
                        self._cache_put(refs[0].image_id, None)
                    continue
                mk.record_stream(cur)
                bx.record_stream(cur)
                live.append(_Live(refs, mk.view(torch.bool) if mk.dtype == torch.uint8 else mk, bx.contiguous()))
            else:
                mk = refs[0].masks
                if self.cleanup_given_masks and gen is not None:
                    mk = gen.cleanup_fixed(mk.view(torch.uint8))[0].view(torch.bool)
                live.append(_Live(refs, mk, refs[0].boxes))
        if not live:
            return
        outs = self._stage(live, self._stage_text(live, serial))
        for u in live:
            if self.image_cache > 0 and props is not None and u.refs[0].image_id is not None:
                self._cache_put(u.refs[0].image_id, (u.masks, u.boxes, u.hybrid, u.gem))
        if self.collected is not None:
            self.collected += outs
        self._done += len(outs)
        self._stage_mark("clip_end")

    def _stage_text(self, live, serial):
        """The text half of _stage, enqueued ahead of the rest: ONE text-encoder batch over the strings of all refs of `live`, the
        GEM tower for the images that need it, the heat-maps of the sentences that bring none.  serial: on the current stream
        (run(serial=True), a rescue's re-run); else on the text stream, behind what the current stream holds now."""
        m = self.model
        cur = torch.cuda.current_stream()
        self._streams()
        s_text = cur if serial else self._s_text
        ev_in, ev_text = torch.cuda.Event(), torch.cuda.Event()
        ev_in.record(cur)
        s_text.wait_event(ev_in)
        refs = [r for u in live for r in u.refs]
        offs = np.cumsum([0] + [r.tokens.shape[0] for r in refs])
        heats = []
        with torch.cuda.stream(s_text):
            lens = [r.token_len for r in refs]
            text_all = m.model.encode_text(torch.cat([r.tokens for r in refs], dim=0) if len(refs) > 1 else refs[0].tokens,
                                           seq_len=None if any(v is None for v in lens) else max(lens))
            texts = [text_all[offs[k]:offs[k + 1]] for k in range(len(refs))]
            # GEM image tower once per IMAGE that has a sentence without a given heat-map (Hybridgl_main.py:200-201:
            # gem_model(tensor_img, [noun_phrase])[0] -> T.Resize((h, w), antialias=True); the tower depends on the image only --
            # the reference re-runs it for every sentence -- and the prompts' text features come out of the text batch above)
            wants = [u for u in live if any(s.imgattn is None for r in u.refs for s in r.sentences)]
            if any(s.imgattn is None and (self.gem_model is None or r.tensor_img is None or s.gem_row is None)
                   for u in wants for r in u.refs for s in r.sentences):
                raise ValueError("a sentence without imgattn needs gem_model, RefBatch.tensor_img and Sentence.gem_row")
            need = [u for u in wants if u.gem is None]
            timgs = [u.refs[0].tensor_img for u in need]
            if len(need) > 1 and all(t.shape == timgs[0].shape for t in timgs):
                feats = self.gem_model.image_features_batch(torch.stack(timgs, dim=0))
            else:
                feats = [self.gem_model.image_features(t) for t in timgs]
            for u, f in zip(need, feats):
                u.gem = f
                u.gem.record_stream(cur)
            for (u, ref), text in zip(((u, r) for u in live for r in u.refs), texts):
                gem_rows = [s.gem_row for s in ref.sentences if s.imgattn is None]
                heat = None
                if gem_rows:
                    from . import gem as G
                    maps = self.gem_model.heatmap(u.gem, _rows(text, gem_rows), ref.tensor_img.shape[-1])
                    heat = G.resize_antialias(maps, ref.sam_img.shape[:2])     # Hybridgl_main.py:201
                    heat.record_stream(cur)
                heats.append(heat)
            ev_text.record(s_text)
        text_all.record_stream(cur)
        return texts, heats, ev_text

    def _stage(self, live, front, now=False):
        """The CLIP + scoring stage (Hybridgl_main.py:93-230) on the current stream, under run() (a group's units) and step()
        (one unit): the views and ONE hybrid forward over the units that have no hybrid features yet, the join with the text
        half (`front` = _stage_text(live, serial)), every ref's tail in order -- called as the ref comes (now), else the fused
        tails in one hgl_score_group call (HYBRIDGL_GROUP_TAIL).  -> step()'s (hybrid, text, last sentence) per ref."""
        texts, heats, ev_text = front
        todo = [u for u in live if u.hybrid is None]       # images whose hybrid features are not cached
        if todo:
            moff = np.cumsum([0] + [u.masks.shape[0] for u in todo])
            local = torch.empty((int(moff[-1]), 3, self.res, self.res), dtype=torch.float32, device=todo[0].masks.device)
            glob = torch.empty_like(local)
            for j, u in enumerate(todo):
                self._views(u.refs[0], u.masks, u.boxes, out=(local[moff[j]:moff[j + 1]], glob[moff[j]:moff[j + 1]]))
            hybrid_all = self.model(local, glob, [u.masks for u in todo], masking_block=self.masking_block, fusion_mode=self.fusion_mode)
            for j, u in enumerate(todo):
                u.hybrid = hybrid_all[moff[j]:moff[j + 1]]
        torch.cuda.current_stream().wait_event(ev_text)
        self._explained = []                         # explained() speaks of this ref / group alone
        defer = [] if self.group_tail and not now else None      # the refs whose tails go into ONE hgl_score_group call at the end
        outs, waiting = [], []                       # waiting: the deferred refs' (hybrid, text), in order

        def flush():
            outs.extend((h0, t0, o0) for (h0, t0), o0 in zip(waiting, self._flush_tails(defer)))
            waiting.clear()
        for (u, ref), text, heat in zip(((u, r) for u in live for r in u.refs), texts, heats):
            out = self._score_ref(replace(ref, masks=u.masks, boxes=u.boxes), u.hybrid, text, heat, defer)
            if out is self._DEFERRED:
                waiting.append((u.hybrid, text))
                continue
            if defer:      # a ref the group call does not serve: the deferred ones before it are logged first (order)
                flush()
            outs.append((u.hybrid, text, out))
        if defer:
            flush()
        return outs

    def _stage_mark(self, label, stream=None):
        """opt-in timeline of the loop (self.stage_marks = [] before run(); bench.py's timed_region, tools/first_use.py): a
        timing event on `stream` (default: the current one) plus the host time of the call"""
        marks = self.stage_marks
        if marks is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        marks.append((label, self.groups_run, ev, time.perf_counter()))

    def stage_timeline(self, base_event, t0):
        """[(label, group number, device ms since base_event, host ms since t0)] of the marks; call after a synchronize"""
        return [(lb, g, round(base_event.elapsed_time(ev), 2), round((th - t0) * 1e3, 2)) for lb, g, ev, th in (self.stage_marks or [])]

    def _cache_put(self, image_id, entry):
        """most recently used last; the oldest entry leaves when the cache is full"""
        self._img_cache.pop(image_id, None)
        self._img_cache[image_id] = entry
        while len(self._img_cache) > self._cache_cap:
            self._img_cache.pop(next(iter(self._img_cache)))

    def partial_rows(self):
        """This process's per-sentence rows [n, 6] int64 = (dataset position, sentence, I, U, I_final, U_final)
        (hybridgl_amd.dist.ROW_FIELDS): the unit that ranks exchange.  One device->host copy."""
        if not self.iu_log:
            return np.zeros((0, 6), dtype=np.int64)
        iu = torch.stack([torch.cat([a.reshape(2), b.reshape(2)]) for a, b in self.iu_log]).cpu().numpy().astype(np.int64)
        return np.concatenate([np.asarray(self.iu_owner, dtype=np.int64).reshape(-1, 2), iu], axis=1)

    def winning_indices(self):
        """[n_sentences, 2] int64: per sentence the proposal indices (pure CLIP, with spatial guidance) into that ref's
        proposal list, in the order the sentences were scored.  One device->host copy."""
        if not self.idx_log:
            return np.zeros((0, 2), dtype=np.int64)
        return torch.stack(self.idx_log).cpu().numpy().astype(np.int64)

    # ---- the sweep's reports (sweep=...) --------------------------------------------------------------------------------------
    def _sweep_on(self, what):
        if self.sweep is None:
            raise RuntimeError(f"{what}: this pipeline runs no sweep; build it with sweep=[(r, alpha, k1, k2), ...]")

    def sweep_rows(self):
        """[C, n, 6] int64: partial_rows() of every configuration of the sweep (dist.ROW_FIELDS), sentences in the order of
        partial_rows().  One device->host copy."""
        self._sweep_on("sweep_rows()")
        C, n = len(self.sweep), len(self.iu_owner)
        out = np.zeros((C, n, 6), dtype=np.int64)
        if n:
            out[:, :, 0:2] = np.asarray(self.iu_owner, dtype=np.int64).reshape(1, n, 2)
            out[:, :, 2:6] = torch.cat([iu for _, iu, _ in self._sweep_log], dim=1).cpu().numpy()
        return out

    def sweep_indices(self):
        """[C, n, 2] int64: winning_indices() of every configuration"""
        self._sweep_on("sweep_indices()")
        if not self._sweep_log:
            return np.zeros((len(self.sweep), 0, 2), dtype=np.int64)
        return torch.cat([idx for idx, _, _ in self._sweep_log], dim=1).cpu().numpy().astype(np.int64)

    def ceiling_rows(self):
        """[n, 5] int64 = (dataset position, sentence, proposal, I, U): per sentence the proposal with the largest IoU against
        its target -- the bound no scoring of these proposals exceeds.  One device->host copy."""
        self._sweep_on("ceiling_rows()")
        n = len(self.iu_owner)
        out = np.zeros((n, 5), dtype=np.int64)
        if n:
            out[:, 0:2] = np.asarray(self.iu_owner, dtype=np.int64).reshape(n, 2)
            out[:, 2:5] = torch.cat([cl for _, _, cl in self._sweep_log], dim=0).cpu().numpy()
        return out

    def sweep_metrics(self, dist=None):
        """sweep.sweep_metrics_from_rows of the job: {"configs": one metrics() dict per configuration (with its r, alpha, k1,
        k2), "ceiling": {oIoU, mIoU, cum, n_sentences}, "best": index of the largest oIoU_final}; with an initialised
        torch.distributed the rows of all ranks are gathered first (ONE dist.gather_rows exchange for all configurations)."""
        from . import dist as D, sweep as SW
        self._sweep_on("sweep_metrics()")
        packed = D.gather_rows(SW.pack_rows(self.sweep_rows(), self.ceiling_rows()), dist, self.model.device)
        rows, ceil6 = SW.unpack_rows(packed, len(self.sweep))
        return SW.sweep_metrics_from_rows(rows, ceil6, self.sweep)

    def metrics(self, dist=None):
        """Hybridgl_main.py:240-247: overall IoU and mean IoU, pure and with spatial guidance; with an initialised
        torch.distributed (`dist`) the rows of all ranks are gathered first (the job's metrics, on every rank)."""
        from . import dist as D
        rows = self.partial_rows()
        overflow = 0
        clip = self.model.model
        if ops.split_mode(getattr(clip, "precision", "f32")):
            overflow = ops.split_overflow_count(reset=True)
        # exchange first, raise afterwards and on EVERY rank: a rank that raised before the all-gather would leave the others
        # waiting in the collective
        m = D.gather_metrics(rows, dist, self.model.device)
        overflow = int(D.max_over_ranks(float(overflow), dist, self.model.device))
        if overflow:     # an activation beyond the fp16 range voids the run: raise, do not report
            from ._lib import HybridGLError
            raise HybridGLError(f"activations exceeded the fp16 range (|x| > 65504) in f16x3 / f16 mode ({overflow} GPU threads saw one on "
                                "some rank): the results contain inf / NaN; rerun with HYBRIDGL_PRECISION=f32 (or precision='f32')")
        return m


def synthetic_ref(i, device, N=64, H=640, W=640, n_sent=3, context=77, vocab=49408, sam_img_size=0, gem=False, gem_size=448,
                  device_blur=False):
    """The benchmark item of SURVEY.md 8d: 640x640 image, 64 proposals, 3 queries, each with a
    sentence, a noun phrase and one other noun (9 token rows).  Returns (RefBatch, numpy dict).
    gem=True: the heat-map is NOT an input; the ref carries tensor_img [3,gem_size,gem_size] and one more token
    row per sentence (the GEM prompt), and the pipeline computes the heat-maps on the device.
    device_blur=True: RefBatch.blurred is None and the step runs cv2.GaussianBlur's fixed-point filter itself."""
    img = synth.synth_image(H, W, 1000 + i)
    blur = synth.box_blur_u8(img)
    norm = synth.imagenet_normalize(img)
    masks = synth.synth_masks(N, H, W, 2000 + i)
    boxes = synth.boxes_from_masks(masks)
    tokens = synth.synth_tokens(3 * n_sent, context, vocab, 3000 + i)
    tensor_img = None
    if gem:
        from .gem import get_gem_img_transform
        tokens = np.concatenate([tokens, synth.synth_tokens(n_sent, context, vocab, 5000 + i)], axis=0)
        tensor_img = get_gem_img_transform(gem_size)(img).numpy()
    gt = masks[(7 * i) % N]
    sents, attn_np = [], []
    for j in range(n_sent):
        dirflag, relaflag, n_nouns = synth.PARSE_RECORDS[j % len(synth.PARSE_RECORDS)]
        attn = synth.synth_heatmap(H, W, 4000 + 10 * i + j)
        attn_np.append(attn)
        sents.append(Sentence(3 * j, 3 * j + 1, [3 * j + 2], dirflag, relaflag, n_nouns,
                              None if gem else torch.from_numpy(attn).to(device), gem_row=3 * n_sent + j if gem else None))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    resized = None   # ResizeLongestSide runs on the device (hgl_resize_pil_bilinear), inside the step
    ref = RefBatch(t(img), None if device_blur else t(blur), t(norm), t(masks), t(boxes), t(tokens), t(gt), sents, resized,
                   tensor_img=t(tensor_img) if gem else None, token_len=int(tokens.argmax(axis=1).max()) + 1, index=i)
    host = dict(img=img, blur=blur, norm=norm, masks=masks, boxes=boxes, tokens=tokens, gt=gt, attn=attn_np,
                tensor_img=tensor_img)
    return ref, host
