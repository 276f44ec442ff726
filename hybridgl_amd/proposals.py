"""SAM proposals as an artefact on disk: written beside a normal run, read back in place of the mask generator.

The proposals of an image are a function of the image and the generator's settings alone, and every axis of an experiment
that lies behind them (fusion mode, masking block, CLIP model, precision of the CLIP stage, the GEM heat-map) re-runs SAM for
nothing.  A store is a directory in the file format of the reference's scripts/amg.py:229-232 with --convert-to-rle:

    <image_id>.json   the list SamAutomaticMaskGenerator.generate() returns in "coco_rle" mode (automatic_mask_generator.py:
                      137-195): records {"segmentation": {"size": [H, W], "counts": COCO string}, "area", "bbox" XYWH,
                      "predicted_iou", "point_coords", "stability_score", "crop_box"}; an image without a proposal is []
    meta.json         the generator's settings (generator_settings), for the reader's report

ProposalStore     the directory: atomic writes (temporary name, then rename), reads that name the image when a file is bad
ProposalRecorder  wraps a generator that speaks group_begin / group_cleanup / group_finish: after group_finish one
                  ops.rle_encode per image over its survivors and asynchronous copies into pinned staging; the files are
                  written once the copies have completed, at later group boundaries and in flush().  Nothing waits in the loop.
StoredProposals   answers the same three calls (and generate_device for HybridGLPipeline.step) from a store: the runs are
                  parsed and packed on the loader threads (prefetch), one upload and one ops.rle_decode_group per group bring
                  them back as pixels with their boxes.  It never runs SAM: a missing or inconsistent file is a ValueError.
compare           two stores image by image, every mask of one against every mask of the other (ops.rle_match on the runs: no
                  mask becomes pixels): did SAM's set move, or only the scoring?
                      python -m hybridgl_amd.proposals compare DIR_A DIR_B [--iou LIST] [--json OUT]
ceiling           the best proposal of a store per target -- the bound no scoring of these proposals exceeds -- without CLIP.
thin              a store made smaller: per image the greedy suppression by MASK overlap (ops.rle_nms on the runs: no mask becomes
                  pixels) that SAM's box NMS leaves undone; the result is a store like any other.
                      python -m hybridgl_amd.proposals thin DIR_IN DIR_OUT --thr T [--metric iou|containment] [--score ...] [--json OUT]
clean             a store re-tuned: postprocess_small_regions at another min_mask_region_area -- small holes filled, small islands
                  dropped (ops.rle_remove_small_regions on the runs: no mask becomes pixels), the boxes taken again, the second
                  box NMS -- so a store saved at one value answers what another would have given without the ViT-H encoder.
                      python -m hybridgl_amd.proposals clean DIR_IN DIR_OUT --min_area A [--nms_thresh T] [--json OUT]"""
import collections
import json
import os
import threading

import numpy as np
import torch

from . import ops
from .sam import build_records, counts_from_set      # noqa: F401  (build_records: the one record builder, importable from here)
from .staging import HarvestQueue, PinnedPool

RECORD_KEYS = ("segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box")


def generator_settings(gen, **extra):
    """what meta.json records of a SamAutomaticMaskGenerator: grid, thresholds and NMS, crop layers, clean-up area and the
    model's mask threshold; `extra`: what only the caller knows (SAM variant, precision, proposal_cap)"""
    meta = {"points_per_side": [int(round(len(g) ** 0.5)) for g in gen.point_grids], "points_per_batch": int(gen.points_per_batch),
            "pred_iou_thresh": float(gen.pred_iou_thresh), "stability_score_thresh": float(gen.stability_score_thresh),
            "stability_score_offset": float(gen.stability_score_offset), "box_nms_thresh": float(gen.box_nms_thresh),
            "crop_nms_thresh": float(gen.crop_nms_thresh), "crop_n_layers": int(gen.crop_n_layers),
            "crop_overlap_ratio": float(gen.crop_overlap_ratio), "min_mask_region_area": int(gen.min_mask_region_area),
            "mask_threshold": float(getattr(gen.model, "mask_threshold", 0.0))}
    meta.update(extra)
    return meta


class ProposalStore:
    """a directory of <image_id>.json record lists and one meta.json"""

    def __init__(self, directory):
        self.directory = os.fspath(directory)

    def path(self, image_id):
        return os.path.join(self.directory, f"{image_id}.json")

    def _write(self, path, obj):
        os.makedirs(self.directory, exist_ok=True)
        tmp = f"{path}.tmp.{os.getpid()}.{threading.get_ident()}"
        try:
            with open(tmp, "w") as f:
                json.dump(obj, f)
            os.replace(tmp, path)      # the final name never holds a partial file
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    def write(self, image_id, records):
        self._write(self.path(image_id), list(records))

    def write_meta(self, meta):
        self._write(os.path.join(self.directory, "meta.json"), dict(meta))

    def meta(self):
        """the settings the writer recorded ({} for a store the upstream script produced)"""
        path = os.path.join(self.directory, "meta.json")
        if not os.path.exists(path):
            return {}
        with open(path) as f:
            return json.load(f)

    def has(self, image_id):
        return os.path.exists(self.path(image_id))

    def image_ids(self):
        """the ids of the images the directory holds a file for, sorted: integers where the name is a number (the datasets'
        ids), the name itself otherwise (a store the upstream script wrote from file names)"""
        names = [n[:-5] for n in os.listdir(self.directory) if n.endswith(".json") and n != "meta.json"]
        ids = [int(n) if n.isdigit() and str(int(n)) == n else n for n in names]
        return sorted(ids, key=lambda v: (isinstance(v, str), v))

    def records(self, image_id):
        """the stored list, as generate() returned it in coco_rle mode; ValueError naming the image for a missing or garbled file"""
        path = self.path(image_id)
        if not os.path.exists(path):
            raise ValueError(f"proposal store {self.directory}: image {image_id} has no file ({os.path.basename(path)})")
        try:
            with open(path) as f:
                recs = json.load(f)
        except (json.JSONDecodeError, UnicodeDecodeError) as e:
            raise ValueError(f"proposal store {self.directory}: image {image_id}: {os.path.basename(path)} is not valid JSON ({e})") from None
        if not isinstance(recs, list):
            raise ValueError(f"proposal store {self.directory}: image {image_id}: expected a list of records")
        for k, r in enumerate(recs):
            seg = r.get("segmentation") if isinstance(r, dict) else None
            if (not isinstance(seg, dict) or not isinstance(seg.get("counts"), str) or not isinstance(seg.get("size"), list)
                    or len(seg["size"]) != 2 or any(key not in r for key in RECORD_KEYS)
                    or not isinstance(r["bbox"], list) or len(r["bbox"]) != 4):
                raise ValueError(f"proposal store {self.directory}: image {image_id} entry {k}: not a coco_rle record "
                                 f"(keys {sorted(RECORD_KEYS)}, segmentation {{size, counts string}})")
        return recs


class _Recorded:
    """a group on its way through a ProposalRecorder: the wrapped generator's state and the images' ids"""
    __slots__ = ("inner", "ids", "overflow")


class ProposalRecorder:
    """A generator that writes what it hands out.  Every call goes to the wrapped generator unchanged -- the run's rows and
    report are those of an unwrapped run -- and the survivors of every image with an id are encoded (ops.rle_encode: runs,
    not pixels) and copied to pinned staging behind it.  A staging buffer is reused only after its copy's event; the files
    are written when the events have completed: at later group boundaries, and in flush().

    strings "host": the runs are copied, n * (4 + ceil(H*W/32)) words per image, and become strings one record at a time in
    _harvest.  "device": ops.rle_to_strings runs behind the encode and ONE copy brings offsets | status | the first string_cap
    bytes (default ops.RLE_STRING_CAP_PER_ENTRY per proposal); _harvest slices.  Only when the strings did not fit, or an entry
    is a bit plane (form 1), does it go back to the device buffers it kept: a second call at the true size, the host codec for
    that entry, one wait.  The files are byte-identical."""
    wants_image_ids = True

    def __init__(self, generator, store, meta=None, strings="host", string_cap=None):
        if strings not in ("host", "device"):
            raise ValueError(f"ProposalRecorder: strings {strings!r} (host or device)")
        self.strings, self.string_cap = strings, string_cap
        self.fallbacks = 0      # images whose strings needed the device buffers again
        self.generator = generator
        self.store = store if isinstance(store, ProposalStore) else ProposalStore(store)
        self.recording = True       # False: calls pass through unrecorded (a rehearsal on images that are not the dataset's)
        self.written = 0
        self._pool = PinnedPool()
        self._pending = HarvestQueue(self._pool)      # payloads (image_id, H, W, n, sw, runs host, scalars host, kept)
        self._seen = set()
        if meta is not None:
            self.store.write_meta(meta)

    def __getattr__(self, name):      # thresholds, crop_n_layers, model, ...: the wrapped generator's
        if name == "generator":
            raise AttributeError(name)
        return getattr(self.generator, name)

    # ---- the three calls of HybridGLPipeline.run
    def group_begin(self, images, cap=None, encoded_event=None, image_ids=None):
        st = _Recorded()
        st.ids = list(image_ids) if image_ids is not None else [None] * len(images)
        st.inner = self.generator.group_begin(images, cap, encoded_event)
        st.overflow = 0
        return st

    def group_cleanup(self, st):
        st.inner = self.generator.group_cleanup(st.inner)
        st.overflow = st.inner.overflow
        return st

    def group_finish(self, st):
        out = self.generator.group_finish(st.inner)
        self._harvest()
        for iid, p in zip(st.ids, out):
            self._record(iid, p[0], p[1], p[2], p[3], p[4])
        return out

    # ---- the calls of HybridGLPipeline.step
    def generate_device(self, image, resized=None, fixed_n=None, image_id=None):
        out = self.generator.generate_device(image, resized=resized, fixed_n=fixed_n)
        self._harvest()
        self._record(image_id, *out[:5])
        return out

    def generate_device_crops(self, image, image_id=None):
        (m, xywh, iou, stab, src), size = self.generator.crops_of_one(image)      # generate_device_crops, with the sources kept
        self._harvest()
        self._record(image_id, m, xywh, iou, stab, src)
        return (m, xywh, iou, stab) + self.generator._sources(src, *size)

    # ---- staging
    def _record(self, image_id, masks, xywh, iou, stab, src):
        if not self.recording:
            return
        if image_id is None:
            raise ValueError("ProposalRecorder: an item without an image_id cannot be stored")
        if image_id in self._seen:      # the image came back after the loop's image cache had dropped it: the same proposals
            return
        self._seen.add(image_id)
        n, H, W = (int(v) for v in masks.shape)
        if n == 0:
            self._pending.put(None, (image_id, H, W, 0, 0, None, None, None))      # no copy to wait for: written in its turn
            return
        sw = ops.rle_slot_words(H, W)
        flat = torch.empty(ops.rle_block_words("set", n, sw), dtype=torch.int32, device=masks.device)
        ops.rle_encode(masks if masks.is_contiguous() else masks.contiguous(), None, sw, out=flat)
        # the few scalars per proposal ride along: rows iou, stability, source, x, y, w, h (all exact in float64)
        sc = [iou.double()[None], stab.double()[None], src.double()[None], xywh.double().t()]
        kept = None
        if self.strings == "device":
            cap = int(self.string_cap) if self.string_cap is not None else ops.RLE_STRING_CAP_PER_ENTRY * n
            slots, table = ops.rle_split(flat, n, sw)
            out = torch.empty(ops.rle_strings_bytes(n, cap), dtype=torch.uint8, device=masks.device)
            ops.rle_to_strings(slots, table, cap, out=out)
            sc.append(table[:, 2].double()[None])      # the areas, which the host mode reads from the table
            kept, flat = (flat, cap), out              # the encoded set stays on the device until the file is written
        runs = self._pool.take(flat.numel(), flat.dtype)
        runs[:flat.numel()].copy_(flat, non_blocking=True)
        sc = torch.cat(sc)
        scal = self._pool.take(sc.numel(), torch.float64)
        scal[:sc.numel()].copy_(sc.reshape(-1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.put(ev, (image_id, H, W, n, sw, runs, scal, kept), (runs, scal))

    def _strings(self, n, sw, H, W, staged, kept):
        """the strings of one image out of the staged offsets | status | bytes; `kept`: the encoded set on the device and the cap"""
        from .sam import strings_from_bytes
        flat, cap = kept
        data, offsets, status = ops.rle_strings_split(staged[:ops.rle_strings_bytes(n, cap)], n, cap)
        total = int(offsets[n])
        slots, table = ops.rle_split(flat, n, sw)
        if total > cap or (status == 1).any():
            self.fallbacks += 1
        if total > cap:      # the offsets are true under any cap: once more at the size they give, and one wait
            d, _, st = ops.rle_to_strings(slots, table, total)
            data, status = d.cpu().numpy(), st.cpu().numpy()
        return strings_from_bytes(data[:total].tobytes(), offsets, status, slots, table, H, W)

    def _harvest(self, wait=False):
        """write the files of the copies that have completed (wait=True: of all), oldest first; their buffers return to the pool"""
        for image_id, H, W, n, sw, runs, scal, kept in self._pending.drain(wait):
            if n == 0:
                self.store.write(image_id, [])
            else:
                rows = 7 if kept is None else 8
                s = scal.numpy()[:rows * n].reshape(rows, n)
                if kept is None:
                    slots, table = ops.rle_split(runs.numpy(), n, sw)
                    counts, strings, areas = counts_from_set(slots, table, H, W), None, table[:, 2]
                else:
                    counts, strings, areas = None, self._strings(n, sw, H, W, runs.numpy(), kept), s[7].astype(np.int64)
                pts, cbs = self.generator._sources(torch.from_numpy(s[2].astype(np.int64)), H, W)
                self.store.write(image_id, build_records(H, W, counts, areas, s[3:7].T.astype(np.int64), s[0].astype(np.float32),
                                                         s[1].astype(np.float32), pts, cbs, strings))
            self.written += 1

    def forget(self):
        """record every image again when it next comes by (a second pass over the same images rewrites their files)"""
        self._seen.clear()

    def flush(self):
        """wait for the copies still in flight and write their files; returns the number of images written so far"""
        self._harvest(wait=True)
        return self.written


class _Rows:
    """the proposals of one stored image, packed on a loader thread: ONE pinned int32 buffer = table [n,4] | slots [n,sw] |
    the bits of predicted_iou [n] | of stability_score [n] (| of area [n], where the walk is ordered by it), the numpy views of
    its parts (_split_group), and the stored boxes for the check"""
    __slots__ = ("n", "H", "W", "sw", "buf", "table", "slots", "iou", "stab", "area", "bbox", "soff", "sbytes")


class _Stored:
    __slots__ = ("ids", "sizes", "counts", "first", "rows", "masks", "boxes", "iou", "stab", "host", "ev", "overflow")


def _split_group(flat, S, sw, area):
    """(slots [S,sw], table [S,4], cols [2,S] = the bits of predicted_iou | of stability_score, area bits [S] or, without
    `area`, nothing) as views of a flat int32 buffer that holds S entries in the layout of _Rows.buf (ops.RLE_BLOCKS "group") --
    an image's rows, a staged group or its upload: numpy array and tensor alike"""
    table, slots, cols, extra = ops.rle_block("group", flat, S, sw, C=int(bool(area)))
    return slots, table, cols, extra


def _group_words(S, sw, area):
    """the int32 words of that layout"""
    return ops.rle_block_words("group", S, sw, C=int(bool(area)))


def _stage_group(rows, counts, area, buf):
    """The host half of a group: the first counts[g] entries of every image's rows, image after image, into the int32 numpy
    buffer `buf` as table [S,4] | slots [S,sw] | iou bits [S] | stab bits [S] (| area bits [S] with `area`).  Returns (S, sw,
    first [G+1]: where each image's entries begin); sw is the widest slot among the images that contribute an entry, and words
    beyond an entry's n_counts stay as the buffer had them: they are never read.  _group_words(S, sw, area) words are written."""
    first = np.cumsum([0] + [int(n) for n in counts])
    S = int(first[-1])
    if S == 0:
        return 0, 0, first
    sw = max(r.sw for r, n in zip(rows, counts) if n)
    slots, table, cols, extra = _split_group(buf, S, sw, area)
    for r, n, e in zip(rows, counts, first):
        if n:
            table[e:e + n] = r.table[:n]
            slots[e:e + n, :r.sw] = r.slots[:n]
            cols[0, e:e + n] = r.iou[:n]
            cols[1, e:e + n] = r.stab[:n]
            if area:
                extra[e:e + n] = r.area[:n]
    return S, sw, first


def _back_layout(S, G, thin, device_strings):
    """The one int32 read-back of a StoredProposals group of S entries in G images: (its words, the slices of its parts).
    aux: boxes | status [2,S,4].  Thinning only: out_src [S] and out_n [G] of ops.rle_select; nms: the output block of ops.rle_nms
    = out_idx [S] | result [S,4] | out_n [G], and codes: the result rows inside it.  Reading strings on the device only: read, the
    codec's status [S,4].  The parts lie in this order without a gap; a part the mode does not have is empty."""
    t = int(bool(thin))      # without thinning the blocks of ops.rle_select and ops.rle_nms are those of no entry in no image
    aux = ops.rle_block_words("aux", S)
    src, n = (aux + v for v in ops.rle_block_ends("back", t * S, G=t * G))
    idx, res, nms = (n + v for v in ops.rle_block_ends("nms", t * S, G=t * G))
    end = nms + 4 * S * bool(device_strings)
    return end, {"aux": slice(0, aux), "out_src": slice(aux, src), "out_n": slice(src, n), "nms": slice(n, nms),
                 "codes": slice(idx, res), "read": slice(nms, end)}


def _undecoded(store, image_id, entry, code, what="mask of the stated size"):
    return ValueError(f"proposal store {store.directory}: image {image_id} entry {entry}: its counts do not decode to a {what} "
                      f"(status {code})")


class StoredProposals:
    """The mask generator's place in HybridGLPipeline taken by a ProposalStore.  No SAM model, no checkpoint.

    prefetch(image_id, size) is the host half -- file, JSON, sam.rle_counts_from_string, packing into one pinned buffer -- and
    belongs on the loader threads (RealRefs.load / RealPhraseCut.load call it); an image nobody prefetched is read where it
    is first asked for.  Per group the loop's thread concatenates the staged rows, issues one upload and one
    ops.rle_decode_group, and reads status and boxes back once, in group_cleanup.  cap: the first `cap` entries of an image.

    mask_nms_thresh: thin every image's list by mask overlap as it loads -- what thin() would have written to a second store,
    without the store.  All of an image's entries are uploaded; ops.rle_nms (mask_nms_metric, and mask_nms_score: one of
    THIN_SCORES, the order of the walk) decides, ops.rle_select moves the survivors to the front of the image's range in stored
    order with their IoU / stability columns, and the one ops.rle_decode_group runs over the compacted set with the original
    counts: the positions behind the survivors decode to empty masks that nobody is handed.  The caps then apply to the
    survivors.  The survivors' counts and source indices ride back in the read-back that carries boxes and status: still one
    per group, no further synchronisation.  thinned = [entries read, entries handed out] over the images met so far, each image
    counted once (noted in group_cleanup).

    strings "host": sam.rle_counts_from_string per record on the loader thread, counts padded to the widest entry on the bus.
    "device": the loader keeps every record's string bytes (ops.rle_strings_pack: offsets | bytes | iou bits | stability bits
    (| area bits) in the one pinned buffer, the slot width from the number of bytes that end a count), group_begin uploads the
    strings as they are and ops.rle_from_strings makes them the slots and the table the same chain takes.  The codec's status
    rides in the group's one read-back; group_cleanup raises for a string that did not read, before the decode's own checks.
    Rows and metrics are those of the host mode bit for bit."""
    wants_image_ids = True
    crop_n_layers = 0      # HybridGLPipeline.step: one generate_device call, whatever produced the store

    def __init__(self, store, device, cap=None, keep=256, mask_nms_thresh=None, mask_nms_metric="iou", mask_nms_score="predicted_iou",
                 strings="host"):
        if strings not in ("host", "device"):
            raise ValueError(f"StoredProposals: strings {strings!r} (host or device)")
        self.strings = strings
        self.store = store if isinstance(store, ProposalStore) else ProposalStore(store)
        self.device = torch.device(device)
        self.cap = cap
        self.keep = int(keep)
        self.mask_nms_thresh = None if mask_nms_thresh is None else float(mask_nms_thresh)
        self.mask_nms_metric, self.mask_nms_score = mask_nms_metric, mask_nms_score
        if self.mask_nms_thresh is not None:
            if self.mask_nms_thresh != self.mask_nms_thresh:
                raise ValueError("StoredProposals: mask_nms_thresh is NaN")
            if mask_nms_metric not in ops.NMS_METRIC:
                raise ValueError(f"StoredProposals: mask_nms_metric {mask_nms_metric!r} (one of {sorted(ops.NMS_METRIC)})")
            if mask_nms_score not in THIN_SCORES:
                raise ValueError(f"StoredProposals: mask_nms_score {mask_nms_score!r} (one of {list(THIN_SCORES)})")
        self._thinned = {}      # image id -> (entries read, entries handed out)
        self._rows = collections.OrderedDict()      # image id -> _Rows, the last `keep` images
        self._lock = threading.Lock()
        self._up = PinnedPool()                     # upload staging: a buffer returns with the event behind its upload
        self._back = PinnedPool(floor=4096)         # read-back buffers group_cleanup has finished with
        self.loaded = 0                             # images parsed (<= images asked for)

    def records(self, image_id):
        return self.store.records(image_id)

    @property
    def thinned(self):
        return [sum(v[0] for v in self._thinned.values()), sum(v[1] for v in self._thinned.values())]

    def settings(self):
        return self.store.meta()

    # ---- host half (loader threads)
    def prefetch(self, image_id, size=None):
        """parse and pack image `image_id` unless it is staged already; size (H, W): the image's, checked against every record"""
        if image_id is None:
            raise ValueError("StoredProposals: an item without an image_id has no stored proposals")
        with self._lock:
            rows = self._rows.get(image_id)
            if rows is not None:
                self._rows.move_to_end(image_id)
        if rows is None:
            rows = self._load(image_id, size)
            with self._lock:
                self._rows[image_id] = rows
                self.loaded += 1
                while len(self._rows) > self.keep:
                    self._rows.popitem(last=False)
        if size is not None and rows.n and (rows.H, rows.W) != tuple(int(v) for v in size):
            raise ValueError(f"proposal store {self.store.directory}: image {image_id} entry 0: size {[rows.H, rows.W]} differs "
                             f"from the image's {[int(v) for v in size]}")
        return rows

    def _load(self, image_id, size):
        recs = self.store.records(image_id)
        rows = _Rows()
        n = rows.n = len(recs)
        rows.H, rows.W = (int(v) for v in (size if size is not None else (recs[0]["segmentation"]["size"] if recs else (0, 0))))
        by_area = self.mask_nms_thresh is not None and self.mask_nms_score == "area"
        if self.strings == "device":
            return self._load_strings(image_id, recs, rows, by_area)
        _, counts = _record_runs(self.store, image_id, recs, (rows.H, rows.W))
        rows.sw = max([len(c) for c in counts] + [1])
        rows.buf = torch.zeros(_group_words(n, rows.sw, by_area), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        rows.slots, rows.table, (rows.iou, rows.stab), rows.area = _split_group(rows.buf.numpy(), n, rows.sw, by_area)
        for k, c in enumerate(counts):
            rows.table[k, 0] = len(c)
            rows.slots[k, :len(c)] = np.asarray(c, dtype=np.uint32).view(np.int32)
        rows.iou.view(np.float32)[:] = [r["predicted_iou"] for r in recs]
        rows.stab.view(np.float32)[:] = [r["stability_score"] for r in recs]
        if by_area:
            rows.area.view(np.float32)[:] = [float(r["area"]) for r in recs]
        rows.bbox = np.asarray([r["bbox"] for r in recs], dtype=np.int64).reshape(n, 4)
        return rows

    def _load_strings(self, image_id, recs, rows, by_area):
        """_load with the strings kept as bytes: ONE pinned buffer = offsets int64 [n+1] | bytes, padded to a word | the bits of
        predicted_iou [n] | of stability_score [n] (| of area [n]); no string is parsed here"""
        n = rows.n
        for k, r in enumerate(recs):
            if tuple(int(v) for v in r["segmentation"]["size"]) != (rows.H, rows.W):
                raise ValueError(f"proposal store {self.store.directory}: image {image_id} entry {k}: size {r['segmentation']['size']} "
                                 f"differs from the image's {[rows.H, rows.W]}")
        try:
            packed, offsets, n_counts = ops.rle_strings_pack([r["segmentation"]["counts"] for r in recs])
        except ValueError as e:
            raise ValueError(f"proposal store {self.store.directory}: image {image_id}: bad counts string ({e})") from None
        rows.sw = max([int(v) for v in n_counts] + [1])
        head = (packed.numel() + 3) // 4 * 4
        rows.buf = torch.zeros(head + 4 * n * (2 + by_area), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        host = rows.buf.numpy()
        host[:packed.numel()] = packed.numpy()
        rows.soff, rows.sbytes = host[:8 * (n + 1)].view(np.int64), host[8 * (n + 1):packed.numel()]
        tail = host[head:].view(np.int32)
        rows.iou, rows.stab, rows.area = tail[:n], tail[n:2 * n], tail[2 * n:]
        rows.slots = rows.table = None
        rows.iou.view(np.float32)[:] = [r["predicted_iou"] for r in recs]
        rows.stab.view(np.float32)[:] = [r["stability_score"] for r in recs]
        if by_area:
            rows.area.view(np.float32)[:] = [float(r["area"]) for r in recs]
        rows.bbox = np.asarray([r["bbox"] for r in recs], dtype=np.int64).reshape(n, 4)
        return rows

    def _upload_strings(self, st, by_area):
        """The device mode's front of group_begin: the first counts[g] strings of every image, image after image, staged as
        offsets int64 [S+1] | iou bits [S] | stab bits [S] (| area bits [S]) | bytes, in ONE upload.  Returns (S, sw, first,
        (offsets, bytes, cols, area) on the device): _stage_group's three and the views of the upload; None in place of the views
        for a group without an entry, which uploads nothing."""
        first = np.cumsum([0] + [int(n) for n in st.counts])
        S = int(first[-1])
        if S == 0:
            return 0, 0, first, None
        sw = max(r.sw for r, n in zip(st.rows, st.counts) if n)
        T = sum(int(r.soff[n]) for r, n in zip(st.rows, st.counts))
        words = 2 * (S + 1) + S * (2 + by_area) + (T + 3) // 4
        host = self._up.take(words, torch.int32)
        h = host.numpy()[:words]
        offs = h[:2 * (S + 1)].view(np.int64)
        cols = h[2 * (S + 1):2 * (S + 1) + 2 * S].reshape(2, S)
        extra = h[2 * (S + 1) + 2 * S:2 * (S + 1) + S * (2 + by_area)]
        data = h[2 * (S + 1) + S * (2 + by_area):].view(np.uint8)
        base = 0
        for r, n, e in zip(st.rows, st.counts, first):
            if n:
                t = int(r.soff[n])
                offs[e:e + n] = r.soff[:n] + base
                data[base:base + t] = r.sbytes[:t]
                cols[0, e:e + n] = r.iou[:n]
                cols[1, e:e + n] = r.stab[:n]
                if by_area:
                    extra[e:e + n] = r.area[:n]
                base += t
        offs[S] = base
        dev = self._upload(host, words)
        a, b = 2 * (S + 1) + 2 * S, 2 * (S + 1) + S * (2 + by_area)
        return S, sw, first, (dev[:2 * (S + 1)].view(torch.int64), dev[b:].view(torch.uint8)[:T], dev[2 * (S + 1):a].reshape(2, S), dev[a:b])

    # ---- device half (the loop's thread)
    def _upload(self, host, words):
        """the first `words` of a staging buffer on the device: one copy, and the buffer back in the pool behind its event"""
        dev = torch.empty(words, dtype=torch.int32, device=self.device)
        dev.copy_(host[:words], non_blocking=True)
        up = torch.cuda.Event()
        up.record()
        self._up.give(host, up)
        return dev

    def group_begin(self, images, cap=None, encoded_event=None, image_ids=None):
        if image_ids is None or len(image_ids) != len(images):
            raise ValueError("StoredProposals: the image ids of the group are needed (RefBatch.image_id)")
        st = _Stored()
        st.overflow = 0
        st.ids = list(image_ids)
        st.sizes = [tuple(int(v) for v in im.shape[:2]) for im in images]
        st.rows = [self.prefetch(iid, size) for iid, size in zip(st.ids, st.sizes)]
        thin = self.mask_nms_thresh is not None
        by_area = thin and self.mask_nms_score == "area"
        caps = [c for c in (cap, self.cap) if c]
        # thinning: every stored entry goes up, and the caps apply to the survivors
        st.counts = [r.n if thin else min([r.n] + caps) for r in st.rows]
        if encoded_event is not None:      # there is no encoder pass to wait for
            encoded_event.record(torch.cuda.current_stream(self.device))
        st.ev = None
        dev_strings = self.strings == "device"
        G = len(st.rows)
        if dev_strings:
            S, sw, st.first, parts = self._upload_strings(st, by_area)
            if S == 0:
                return st
        else:
            # (room for the group however wide its slots are; a group without an entry stages nothing)
            room = _group_words(sum(st.counts), max([r.sw for r in st.rows] + [0]), by_area)
            host = self._up.take(room, torch.int32) if room else torch.empty(0, dtype=torch.int32)
            S, sw, st.first = _stage_group(st.rows, st.counts, by_area, host.numpy())
            if S == 0:
                return st
            slots, table, cols, area = _split_group(self._upload(host, _group_words(S, sw, by_area)), S, sw, by_area)
        # ONE int32 buffer leaves in one copy into pooled pinned memory: boxes | status and, thinning, | out_src | out_n | the
        # NMS's out_idx, result, out_n (| the string codec's status, reading strings on the device); group_cleanup reads it,
        # where SAM reads its first counts, and hands the buffer back
        words, part = _back_layout(S, G, thin, dev_strings)
        back = torch.empty(words, dtype=torch.int32, device=self.device)
        if dev_strings:
            offs, data, cols, area = parts
            slots, table, _ = ops.rle_from_strings(data, offs, S, sw, status=back[part["read"]].view(S, 4))
        if thin:
            scores = {"predicted_iou": cols[0], "stability_score": cols[1], "area": area, "stored": None}[self.mask_nms_score]
            if scores is not None:
                scores = scores.view(torch.float32)
            result = ops.rle_nms(slots, table, st.sizes, st.counts, scores, self.mask_nms_thresh, self.mask_nms_metric,
                                 out=back[part["nms"]])[2]
            slots, table, cols, _, _ = ops.rle_select(slots, table, st.sizes, st.counts, nms_result=result, cols=cols,
                                                      max_keep=min(caps) if caps else None,
                                                      back=back[part["out_src"].start:part["out_n"].stop])
        st.iou, st.stab = cols[0].view(torch.float32), cols[1].view(torch.float32)
        st.masks, st.boxes = self._decode(slots, table, st.sizes, st.counts, back[part["aux"]].view(2, S, 4))[:2]
        st.host = self._back.take(words, torch.int32)
        st.host[:words].copy_(back, non_blocking=True)
        st.ev = torch.cuda.Event()
        st.ev.record()
        return st

    def _decode(self, slots, table, sizes, counts, aux):
        """the group's pixels, boxes (aux[0]) and status (aux[1]): two launches whatever the group holds"""
        return ops.rle_decode_group(slots, table, sizes, counts, aux=aux)

    def _check_image(self, iid, r, codes, srcs, boxes, status):
        """what a store is held to, image by image: every uploaded entry decodes (codes: the NMS's, where it ran), and of the
        entries handed out (position p is record srcs[p]) the first that did not decode, or whose stored bbox is not the box
        of its mask, raises -- its status before its box"""
        what = f"{r.H} x {r.W} mask"
        bad = np.flatnonzero(codes != 0)
        if len(bad):
            raise _undecoded(self.store, iid, int(bad[0]), int(codes[bad[0]]), what)
        xywh = np.concatenate([boxes[:, :2], boxes[:, 2:] - boxes[:, :2]], 1)
        # (an empty mask has no box: the reference stores its zero box moved by the crop's origin, whatever that is)
        off = (status[:, 1] > 0) & (xywh != r.bbox[srcs]).any(1)
        bad = np.flatnonzero((status[:, 0] != 0) | off)
        if len(bad):
            p = int(bad[0])
            k = int(srcs[p])
            if status[p, 0] != 0:
                raise _undecoded(self.store, iid, k, int(status[p, 0]), what)
            raise ValueError(f"proposal store {self.store.directory}: image {iid} entry {k}: the stored bbox "
                             f"{r.bbox[k].tolist()} is not the box of its mask {xywh[p].tolist()}")

    def group_cleanup(self, st):
        if st.ev is None:
            return st
        thin = self.mask_nms_thresh is not None
        S, G = int(st.first[-1]), len(st.rows)
        st.ev.synchronize()
        words, part = _back_layout(S, G, thin, self.strings == "device")
        h = st.host.numpy()[:words].copy()
        self._back.give(st.host)
        st.host = None
        read = h[part["read"]].reshape(-1, 4)[:, 0]      # the string codec's codes, reading strings on the device (else nothing)
        boxes, status = h[part["aux"]].reshape(2, S, 4)
        out_src, out_n = h[part["out_src"]], h[part["out_n"]]      # (these three are empty without thinning)
        codes = h[part["codes"]].reshape(-1, 4)[:, 0]      # the NMS's result rows: every source entry's code
        kept = []
        for g, (iid, r, n, e) in enumerate(zip(st.ids, st.rows, st.counts, st.first)):
            bad = np.flatnonzero(read[e:e + n])
            if len(bad):
                code = int(read[e + bad[0]])
                raise ValueError(f"proposal store {self.store.directory}: image {iid} entry {int(bad[0])}: bad counts string (code {code}: " +
                                 {2: "it ends inside a count", 3: "a count of more than 7 characters"}.get(code, "not read") + ")")
            k = int(out_n[g]) if thin else n
            self._check_image(iid, r, codes[e:e + n], out_src[e:e + k] if thin else np.arange(k), boxes[e:e + k], status[e:e + k])
            kept.append(k)
            if thin:
                self._thinned[iid] = (n, k)
        if thin:
            st.masks = [m[:k] for m, k in zip(st.masks, kept)]
            st.counts = kept      # st.first keeps the uploaded layout: the survivors lead every image's range
        return st

    def group_finish(self, st):
        """per image (masks u8 [n,H,W], boxes_xywh int64 [n,4], iou [n], stability [n], None)"""
        from .sam import _xywh
        out = []
        for g, ((H, W), n, e) in enumerate(zip(st.sizes, st.counts, st.first)):
            if n == 0:
                f32 = torch.empty((0,), dtype=torch.float32, device=self.device)
                out.append((torch.empty((0, H, W), dtype=torch.uint8, device=self.device),
                            torch.empty((0, 4), dtype=torch.int64, device=self.device), f32, f32, None))
                continue
            out.append((st.masks[g], _xywh(st.boxes[e:e + n]), st.iou[e:e + n], st.stab[e:e + n], None))
        return out

    def generate_group(self, images, image_ids, cap=None):
        return self.group_finish(self.group_cleanup(self.group_begin(images, cap, None, image_ids)))

    def generate_device(self, image, resized=None, fixed_n=None, image_id=None):
        """HybridGLPipeline.step: the image's proposals as a group of one"""
        if fixed_n is not None:
            raise ValueError("StoredProposals: fixed_n is the synthetic benchmark's switch; a store hands out what it holds")
        return self.generate_group([image], [image_id])[0]


def _store(x):
    return x if isinstance(x, ProposalStore) else ProposalStore(x)


def _record_runs(store, image_id, recs, expect=None):
    """(size (H, W), the run lists of the records).  expect: the image's size, which every record must state; without it the
    records must agree with entry 0 on a size an image can have, and the size of an empty list is None"""
    from .sam import rle_counts_from_string
    size, runs = expect, []
    for k, r in enumerate(recs):
        hw = tuple(int(v) for v in r["segmentation"]["size"])
        if expect is not None and hw != tuple(expect):
            raise ValueError(f"proposal store {store.directory}: image {image_id} entry {k}: size {r['segmentation']['size']} "
                             f"differs from the image's {list(expect)}")
        size = size or hw
        if expect is None and (hw != size or hw[0] <= 0 or hw[1] <= 0 or hw[0] * hw[1] >= 1 << 31):
            raise ValueError(f"proposal store {store.directory}: image {image_id} entry {k}: size {list(hw)} "
                             + (f"differs from entry 0's {list(size)}" if hw != size else "is no image size"))
        try:
            runs.append(rle_counts_from_string(r["segmentation"]["counts"]))
        except Exception as e:
            raise ValueError(f"proposal store {store.directory}: image {image_id} entry {k}: bad counts string ({e})") from None
    return size, runs


def _image_runs(store, image_id, cap=None):
    """(size (H, W) or None for an image without a record, the run lists of its first `cap` records)"""
    recs = store.records(image_id)
    if cap:
        recs = recs[:int(cap)]
    return _record_runs(store, image_id, recs)


def _pack(runs, device):
    """run lists -> (slots, table) on the device, as predictions._pack packs a set's strings (the sizes ride in the call)"""
    return ops.rle_pack(runs, 1, 1, device=device)


def _check_decoded(store, ids, counts, match):
    """every entry of `match` [S,4] (host) must have decoded with code 0"""
    e = 0
    for iid, n in zip(ids, counts):
        bad = np.flatnonzero(match[e:e + n, 0] != 0)
        if len(bad):
            raise _undecoded(store, iid, int(bad[0]), int(match[e + bad[0], 0]))
        e += n


def compare(a, b, thresholds=(0.5, 0.75, 0.9), device=None, group=16):
    """Two proposal stores (ProposalStore objects or directories), image by image: every mask of A's list against every mask of
    B's (ops.rle_match, `group` images per call; the strings' runs cross the bus, no mask becomes pixels).  The lists may differ
    in length and order.  Returns {"summary": ..., "per_image": {image_id: ...}}; per image: n_a, n_b; identical = the masks of A
    whose best partner in B is the same mask (I == area_a == area_b); at_iou = {t: [masks of A, masks of B with a partner at IoU
    >= t]} per threshold; mean_iou_a / min_iou_a / mean_iou_b / min_iou_b over each side's best IoU (None for an empty list; a
    mask without an intersecting partner, an empty mask included, counts 0).  The summary sums the counts, takes mean and
    minimum over all masks, and lists only_in_a, only_in_b (images one store lacks) and size_mismatch (images whose stores
    state different sizes: listed, not compared)."""
    a, b = _store(a), _store(b)
    thresholds = [float(t) for t in thresholds]
    ids_a, ids_b = a.image_ids(), b.image_ids()
    in_b = set(ids_b)
    in_a = set(ids_a)
    common = [i for i in ids_a if i in in_b]
    per_image, size_mismatch = {}, []

    def chunks():
        """the common images whose sizes agree, `group` at a time: only a chunk's run lists are held at once"""
        chunk = []
        for iid in common:
            (size_a, runs_a), (size_b, runs_b) = _image_runs(a, iid), _image_runs(b, iid)
            if size_a is not None and size_b is not None and size_a != size_b:
                size_mismatch.append(iid)
                continue
            chunk.append((iid, size_a or size_b or (1, 1), runs_a, runs_b))
            if len(chunk) >= max(int(group), 1):
                yield chunk
                chunk = []
        if chunk:
            yield chunk

    def side(best_iou):
        n = len(best_iou)
        return {"n": n, "at": [int((best_iou >= t).sum()) for t in thresholds], "sum": float(best_iou.sum()),
                "min": float(best_iou.min()) if n else None}

    for chunk in chunks():
        ca, cb = [len(c[2]) for c in chunk], [len(c[3]) for c in chunk]
        sa, ta = _pack([r for c in chunk for r in c[2]], device)
        sb, tb = _pack([r for c in chunk for r in c[3]], device)
        _, ma, mb = ops.rle_match(sa, ta, sb, tb, [c[1] for c in chunk], ca, cb, matrix=False)
        ma, mb = ma.cpu().numpy().astype(np.int64), mb.cpu().numpy().astype(np.int64)
        _check_decoded(a, [c[0] for c in chunk], ca, ma)
        _check_decoded(b, [c[0] for c in chunk], cb, mb)
        ea = eb = 0
        for (iid, _, _, _), na, nb in zip(chunk, ca, cb):
            xa, xb = ma[ea:ea + na], mb[eb:eb + nb]

            def best_iou(x, other):
                has = x[:, 2] >= 0
                partner = other[np.where(has, x[:, 2], 0), 1] if len(other) else np.zeros(len(x), np.int64)
                union = x[:, 1] + partner - x[:, 3]
                return np.where(has, x[:, 3] / np.maximum(union, 1), 0.0), has & (x[:, 3] == x[:, 1]) & (x[:, 3] == partner)

            iou_a, same = best_iou(xa, xb)
            iou_b, _ = best_iou(xb, xa)
            per_image[iid] = {"a": side(iou_a), "b": side(iou_b), "identical": int(same.sum())}
            ea += na
            eb += nb

    def report(rows):
        """the public shape of one image's (or all images') figures from the sides' sums"""
        na, nb = sum(r["a"]["n"] for r in rows), sum(r["b"]["n"] for r in rows)
        mins = {s: [r[s]["min"] for r in rows if r[s]["n"]] for s in "ab"}
        return {"n_a": na, "n_b": nb, "identical": sum(r["identical"] for r in rows),
                "at_iou": {t: [sum(r["a"]["at"][k] for r in rows), sum(r["b"]["at"][k] for r in rows)] for k, t in enumerate(thresholds)},
                "mean_iou_a": sum(r["a"]["sum"] for r in rows) / na if na else None, "min_iou_a": min(mins["a"]) if mins["a"] else None,
                "mean_iou_b": sum(r["b"]["sum"] for r in rows) / nb if nb else None, "min_iou_b": min(mins["b"]) if mins["b"] else None}

    summary = report(list(per_image.values()))
    summary.update({"n_images": len(per_image), "only_in_a": [i for i in ids_a if i not in in_b],
                    "only_in_b": [i for i in ids_b if i not in in_a], "size_mismatch": size_mismatch})
    return {"summary": summary, "per_image": {iid: report([r]) for iid, r in per_image.items()}}


def ceiling(store, targets, cap=None, device=None, group=16):
    """The best proposal of a store per target, without CLIP or GEM: rows [n,5] int64 = (index, sentence, proposal, I, U), the
    format and the rule of HybridGLPipeline.ceiling_rows() -- per target the proposal of its image with the largest I / U,
    compared exactly, the lowest index on a tie (proposal 0 with I = 0 when none intersects); an image without a proposal
    contributes no row, as the loop skips its refs.  targets: an iterable of ((index, sentence), image_id, target) in any order,
    a target being a mask [H,W] bool / uint8 device tensor or a refer_io.PolygonTarget; masks are encoded on the device
    (ops.rle_encode, as predictions.score encodes them), the polygon targets of a call are rasterised on the device, straight
    into run lengths, by ONE ops.rle_from_polygons call and never become pixels; either way they are
    met by the stored runs in ops.rle_match, `group` images per call.  device: where to (None: where the targets are).  cap:
    the first `cap` records of every image, as StoredProposals(cap=).  Rows are sorted by (index, sentence)."""
    from .predictions import _polygon_runs, _stack_masks
    from .refer_io import PolygonTarget
    store = _store(store)
    rows, runs_of, seen = [], {}, set()

    def flush(items):
        by_image = collections.OrderedDict()
        for key, iid, t in items:
            by_image.setdefault(iid, []).append((key, t))
        ids, sizes, ca, cb, runs, enc = [], [], [], [], [], []
        poly_keys, poly_entries, poly_counts = [], [], []      # the call's polygon targets, image by image
        for iid, its in by_image.items():
            H, W = (int(v) for v in its[0][1].shape[-2:])
            size, r = runs_of[iid]
            if not r:
                continue
            if size != (H, W) or any(tuple(int(v) for v in t.shape[-2:]) != (H, W) for _, t in its):
                raise ValueError(f"proposal store {store.directory}: image {iid}: size {list(size)} differs from its target's {[H, W]}")
            # an image's mask targets first, then its polygon targets: the rows carry their keys, the order is free
            pix = [it for it in its if not isinstance(it[1], PolygonTarget)]
            pol = [it for it in its if isinstance(it[1], PolygonTarget)]
            by_image[iid] = its = pix + pol
            if pix:
                gt = _stack_masks([t for _, t in pix], H, W)
                enc.append(ops.rle_encode(gt if device is None else gt.to(device)))
            else:
                enc.append(None)
            poly_keys += [k for k, _ in pol]
            poly_entries += [t.polygons for _, t in pol]
            poly_counts.append(len(pol))
            ids.append(iid)
            sizes.append((H, W))
            ca.append(len(r))
            cb.append(len(its))
            runs += r
        if not ids:
            return
        dev = next((e[0].device for e in enc if e is not None), device)
        if poly_entries:
            ps, pt = _polygon_runs("ceiling", [f"target {k}" for k in poly_keys], poly_entries, sizes, poly_counts, dev)
            dev = ps.device
            e, parts = 0, []
            for own, n in zip(enc, poly_counts):      # per image: its encoded masks, then its share of the polygon set
                if own is not None:
                    parts.append(own)
                if n:
                    parts.append((ps[e:e + n], pt[e:e + n]))
                e += n
            enc = parts
        sw = max(int(s.shape[1]) for s, _ in enc)
        sb = torch.cat([torch.cat([s, s.new_zeros((s.shape[0], sw - s.shape[1]))], 1) for s, _ in enc]).contiguous()
        tb = torch.cat([t for _, t in enc]).contiguous()
        sa, ta = _pack(runs, dev)
        _, ma, mb = ops.rle_match(sa, ta, sb, tb, sizes, ca, cb, matrix=False)
        ma, mb = ma.cpu().numpy().astype(np.int64), mb.cpu().numpy().astype(np.int64)
        _check_decoded(store, ids, ca, ma)
        if (mb[:, 0] != 0).any():      # ops.rle_encode with its default slot never loses a mask
            raise RuntimeError(f"ceiling: target {int(np.flatnonzero(mb[:, 0] != 0)[0])} of the call did not encode (status "
                               f"{int(mb[mb[:, 0] != 0][0, 0])})")
        ea = eb = 0
        for iid, na, nb in zip(ids, ca, cb):
            for j, (key, _) in enumerate(by_image[iid]):
                _, area_t, best, inter = mb[eb + j]
                best = max(int(best), 0)
                rows.append([key[0], key[1], best, int(inter), int(ma[ea + best, 1] + area_t - inter)])
            ea += na
            eb += nb

    pending, images = [], set()
    for key, iid, t in targets:
        key = (int(key[0]), int(key[1]))
        if key in seen:
            raise ValueError(f"ceiling: two targets for {key}")
        seen.add(key)
        if iid not in runs_of:
            runs_of[iid] = _image_runs(store, iid, cap)
        if iid not in images and len(images) >= max(int(group), 1):      # a group is full: the images met so far go in one call
            flush(pending)
            pending, images = [], set()
            runs_of = {iid: runs_of[iid]}
        images.add(iid)
        pending.append((key, iid, t))
    flush(pending)
    return np.asarray(sorted(rows), dtype=np.int64).reshape(-1, 5)


def _rewrite(op, src, dst, group, key, settings, extra, work):
    """What thin and clean share: the store `src` read `group` images at a time and written, image by image, to `dst`, a
    directory that holds no store yet.  work(chunk [(image_id, records)], sized [_record_runs of each], counts, check), called
    for a chunk that holds a record at all, does the operation's device work, has check(result [S,4] on the host) raise for an
    entry that did not decode, and returns per image (the records to write, the image's further counters: one per name in
    `extra`).  dst's meta is src's plus {key: settings and "source"}.  Returns {"per_image": {image_id: [before, after,
    *counters]}, "before": total, "after": total, and a total per name in `extra`}."""
    src, dst = _store(src), _store(dst)
    if os.path.realpath(src.directory) == os.path.realpath(dst.directory):
        raise ValueError(f"{op}: the source and the destination are the same directory ({src.directory})")
    if not os.path.isdir(src.directory):
        raise ValueError(f"{op}: {src.directory}: no such directory")
    if os.path.isdir(dst.directory) and any(n.endswith(".json") for n in os.listdir(dst.directory)):
        raise ValueError(f"{op}: {dst.directory} already holds a store")
    ids = src.image_ids()
    per_image = {}
    step = max(int(group), 1)
    for c0 in range(0, len(ids), step):
        chunk = [(iid, src.records(iid)) for iid in ids[c0:c0 + step]]
        sized = [_record_runs(src, iid, recs) for iid, recs in chunk]
        counts = [len(runs) for _, runs in sized]
        out = [([], [0] * len(extra))] * len(chunk)
        if sum(counts):
            out = work(chunk, sized, counts, lambda result: _check_decoded(src, [iid for iid, _ in chunk], counts, result))
        for (iid, recs), (kept, counters) in zip(chunk, out):
            dst.write(iid, kept)
            per_image[iid] = [len(recs), len(kept)] + list(counters)
    meta = dict(src.meta())
    meta[key] = dict(settings, source=src.directory)
    dst.write_meta(meta)
    return {"per_image": per_image,
            **{name: sum(v[i] for v in per_image.values()) for i, name in enumerate(["before", "after"] + list(extra))}}


THIN_SCORES = ("predicted_iou", "stability_score", "area", "stored")


def thin(src, dst, thr, metric="iou", score="predicted_iou", group=16, device=None):
    """A proposal store made smaller by mask NMS: for every image of `src` the records that ops.rle_nms keeps (`group` images
    per call; the strings' runs cross the bus, no mask becomes pixels) are written to `dst`, unchanged and in their stored
    order; an image without a proposal stays [].  An entry falls when a kept entry before it in the walk has ratio > thr with
    it; metric "iou" or "containment" (I / the smaller area: a part nested in a whole, or the whole, whichever comes later).
    score: the record field the walk is ordered by, descending, the stored index breaking ties -- "predicted_iou",
    "stability_score" or "area" (compared as float32) -- or "stored": the stored order itself.  dst's meta is src's plus
    {"thinned": {"thr", "metric", "score", "source"}}.  ValueError for dst == src, for a dst that holds a store already, for an
    unknown score or metric and for a record that does not decode.  An image may hold at most 4096 records.
    Returns {"per_image": {image_id: [before, after]}, "before": total, "after": total}."""
    if metric not in ops.NMS_METRIC:
        raise ValueError(f"thin: metric {metric!r} (one of {sorted(ops.NMS_METRIC)})")
    if score not in THIN_SCORES:
        raise ValueError(f"thin: score {score!r} (one of {list(THIN_SCORES)})")
    thr = float(thr)
    if thr != thr:
        raise ValueError("thin: the threshold is NaN")
    def kept(chunk, sized, counts, check):
        slots, table = _pack([r for _, runs in sized for r in runs], device)
        scores = None
        if score != "stored":
            scores = torch.tensor([float(r[score]) for _, recs in chunk for r in recs], dtype=torch.float32).to(slots.device)
        out_idx, out_n, result = ops.rle_nms(slots, table, [size or (1, 1) for size, _ in sized], counts, scores, thr, metric)
        out_idx, out_n, result = (x.cpu().numpy().astype(np.int64) for x in (out_idx, out_n, result))
        check(result)
        out, e = [], 0
        for (_, recs), n, k in zip(chunk, counts, out_n):
            out.append(([recs[i] for i in sorted(int(i) for i in out_idx[e:e + int(k)])], []))
            e += n
        return out

    return _rewrite("thin", src, dst, group, "thinned", {"thr": thr, "metric": metric, "score": score}, [], kept)


def clean(src, dst, min_area, nms_thresh=0.7, group=16, device=None):
    """postprocess_small_regions (automatic_mask_generator.py:324-372) on a proposal store: what the generator's
    min_mask_region_area would have done to the records of `src`, written to `dst` without a SAM model.  Per chunk of `group`
    images: holes smaller than min_area filled and islands smaller than it dropped in every record's mask
    (ops.rle_remove_small_regions in mode both; the strings' runs cross the bus, no mask becomes pixels), then the box NMS over
    the boxes of the cleaned masks at nms_thresh (the generator uses max(box_nms_thresh, crop_nms_thresh)), an untouched mask
    scoring 1.0 and a changed one 0.0 (sam.nms_segments; sam.nms for an image of more than 1024 records).  The kept records are
    written in the NMS's order, the order generate() hands them out in.  A kept record whose mask changed gets a new
    `segmentation`, `area` and `bbox`; its other fields, and an unchanged record, stay as they stood.  dst's meta is src's plus
    {"cleaned": {"min_area", "nms_thresh", "source"}}.  ValueError for dst == src, for a dst that holds a store already, for a
    negative min_area or a NaN threshold and for a record that does not decode.  An image may hold at most 4096 records.
    Returns {"per_image": {image_id: [before, after, changed among the kept]}, "before": total, "after": total, "changed": total}."""
    from . import sam
    min_area = int(min_area)
    if min_area < 0:
        raise ValueError(f"clean: min_area {min_area} (must not be negative)")
    nms_thresh = float(nms_thresh)
    if nms_thresh != nms_thresh:
        raise ValueError("clean: the threshold is NaN")
    def cleaned(chunk, sized, counts, check):
        S = sum(counts)
        sizes = [size or (1, 1) for size, _ in sized]
        slots, table = _pack([r for _, runs in sized for r in runs], device)
        dev, sw = slots.device, int(slots.shape[1])
        # an output slot of the plane's size loses no mask: runs where they fit, the bit plane otherwise; rle_from_slot reads either
        osw = max([sw] + [ops.rle_slot_words(H, W) for (H, W), n in zip(sizes, counts) if n])
        flat = torch.empty(ops.rle_block_words("clean", S, osw), dtype=torch.int32, device=dev)
        _, _, boxes, result = ops.rle_remove_small_regions(slots, table, sizes, counts, min_area, "both",
                                                           seg_cap=sw // 2 + max(W for _, W in sizes) + 1, slot_words=osw, out=flat)
        boxes = boxes.clone()      # a buffer of its own: the NMS wants its boxes 16-byte aligned, the view lies where table and slots end
        scores = (result[:, 2] == 0).to(torch.float32)
        keep = torch.ones(S, dtype=torch.uint8, device=dev)
        if max(counts) <= 1024:
            offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
            order, n = sam.nms_segments(boxes, scores, keep, offs, max(counts), nms_thresh)
            order, n = order.cpu().numpy().astype(np.int64), n.cpu().numpy().astype(np.int64)
        else:      # a list of any length, image by image
            order, n, e = np.zeros(S, np.int64), np.zeros(len(counts), np.int64), 0
            for k, c in enumerate(counts):
                if c:
                    o, nn = sam.nms(boxes[e:e + c].contiguous(), scores[e:e + c].contiguous(), keep[e:e + c].contiguous(), nms_thresh)
                    order[e:e + c], n[k] = o.cpu().numpy(), int(nn.cpu()[0])
                e += c
        h_table, h_slots, h_boxes, h_result = ops.rle_block("clean", flat.cpu().numpy(), S, osw)
        check(h_result)
        out, e = [], 0
        for k, ((_, recs), (size, _), c) in enumerate(zip(chunk, sized, counts)):
            kept, changed = [], 0
            for i in order[e:e + int(n[k])]:
                r, s = recs[int(i)], e + int(i)
                if h_result[s, 2]:
                    H, W = size
                    runs = sam.rle_from_slot(h_slots[s], int(h_table[s, 0]), int(h_table[s, 1]), H, W)
                    x0, y0, x1, y1 = (int(v) for v in h_boxes[s])
                    r = dict(r, segmentation=sam.coco_encode_rle({"size": [H, W], "counts": runs}), area=int(h_result[s, 1]),
                             bbox=[x0, y0, x1 - x0, y1 - y0])
                    changed += 1
                kept.append(r)
            out.append((kept, [changed]))
            e += c
        return out

    return _rewrite("clean", src, dst, group, "cleaned", {"min_area": min_area, "nms_thresh": nms_thresh}, ["changed"], cleaned)


IMAGE_NAMES = ("{0}.png", "{0}.jpg", "COCO_train2014_{0:012d}.jpg", "COCO_train2014_{0:012d}.png")


def render(src, out, images, limit=0, group=16, device=None):
    """Pictures of a proposal store: every stored proposal of an image painted over it in palette colours with outlines, the
    largest area first and the stored order among equals, so that small proposals stay visible (demo.paint_all's style).  The
    strings' runs cross the bus and `group` images leave one ops.rle_paint call; no entry is decoded to a byte mask.  images:
    the directory that holds the image files, named by the image id (IMAGE_NAMES); out: the directory of the {image_id}.png
    files.  ValueError for an image file that is missing or whose size differs from the records'.  Returns the paths."""
    from PIL import Image
    from . import render as R
    src = _store(src)
    if not os.path.isdir(src.directory):
        raise ValueError(f"render: {src.directory}: no such directory")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    os.makedirs(out, exist_ok=True)
    ids = src.image_ids()
    if limit:
        ids = ids[:int(limit)]
    paths = []
    step = min(max(int(group), 1), 64)
    for c0 in range(0, len(ids), step):
        chunk, pics, sized, order, styles = ids[c0:c0 + step], [], [], [], []
        for iid in chunk:
            path = next((p for p in (os.path.join(images, n.format(iid)) for n in IMAGE_NAMES) if os.path.exists(p)), None)
            if path is None:
                raise ValueError(f"render: no image file for image {iid} under {images}")
            pics.append(R._image_u8(np.array(Image.open(path).convert("RGB")), device))
            recs = src.records(iid)
            sized.append(_record_runs(src, iid, recs, expect=tuple(int(v) for v in pics[-1].shape[:2])))
            order += sorted(range(len(recs)), key=lambda k: (-int(recs[k]["area"]), k))
            styles.append(R.proposal_styles(len(recs)))
        counts = [len(runs) for _, runs in sized]
        slots, table = _pack([r for _, runs in sized for r in runs], device)
        painted, _, status = ops.rle_paint(slots, table, [tuple(p.shape[:2]) for p in pics], counts, np.asarray(order, dtype=np.int32),
                                           counts, np.concatenate(styles).reshape(-1, 4), base=pics)
        _check_decoded(src, chunk, counts, status.cpu().numpy())
        for iid, pic in zip(chunk, painted):
            paths.append(os.path.join(out, f"{iid}.png"))
            R.save_png(paths[-1], pic)
    return paths


def _jsonable(report):
    return {"summary": report["summary"], "per_image": [dict(v, image_id=k) for k, v in report["per_image"].items()]}


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m hybridgl_amd.proposals", description="stored SAM proposals (main.py --save_proposals)")
    sub = p.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compare", help="two stores, image by image, every mask against every mask")
    c.add_argument("dir_a")
    c.add_argument("dir_b")
    c.add_argument("--iou", default="0.5,0.75,0.9", metavar="LIST", help="the IoU thresholds of the report, comma-separated")
    c.add_argument("--json", default="", metavar="OUT", help="also write the summary and the per-image figures here")
    t = sub.add_parser("thin", help="a store made smaller by mask NMS; evaluate the result with main.py --proposals_dir")
    t.add_argument("dir_in")
    t.add_argument("dir_out")
    t.add_argument("--thr", type=float, required=True, help="an entry falls when a kept entry before it has ratio > THR with it")
    t.add_argument("--metric", default="iou", choices=sorted(ops.NMS_METRIC))
    t.add_argument("--score", default="predicted_iou", choices=list(THIN_SCORES), help="the order of the walk (stored: as stored)")
    t.add_argument("--json", default="", metavar="OUT", help="also write the per-image counts here")
    k = sub.add_parser("clean", help="a store with small holes filled and small islands dropped: the generator's min_mask_region_area, after the fact")
    k.add_argument("dir_in")
    k.add_argument("dir_out")
    k.add_argument("--min_area", type=int, required=True, help="a hole or an island of fewer pixels is filled / dropped")
    k.add_argument("--nms_thresh", type=float, default=0.7, help="the box NMS that follows (the generator's max(box_nms_thresh, crop_nms_thresh))")
    k.add_argument("--json", default="", metavar="OUT", help="also write the per-image counts here")
    r = sub.add_parser("render", help="every stored proposal of an image painted over it, on the device: one PNG per image")
    r.add_argument("dir_in")
    r.add_argument("out")
    r.add_argument("--images", required=True, metavar="ROOT", help="the directory of the image files, named by the image id")
    r.add_argument("--limit", type=int, default=0, metavar="N", help="the first N images of the store (0 = all)")
    args = p.parse_args(argv)
    if args.cmd == "render":
        try:
            paths = render(args.dir_in, args.out, args.images, args.limit)
        except (OSError, ValueError) as e:
            raise SystemExit(f"hybridgl_amd.proposals: {e}")
        print(f"painted {len(paths)} images of {args.dir_in} into {args.out}")
        return 0
    if args.cmd in ("thin", "clean"):
        try:
            if args.cmd == "thin":
                rep = thin(args.dir_in, args.dir_out, args.thr, args.metric, args.score)
            else:
                rep = clean(args.dir_in, args.dir_out, args.min_area, args.nms_thresh)
        except (OSError, ValueError) as e:
            raise SystemExit(f"hybridgl_amd.proposals: {e}")
        print(f"images: {len(rep['per_image'])}   proposals: {rep['before']} -> {rep['after']}"
              + (f"   changed among the kept: {rep['changed']}" if "changed" in rep else ""))
        if args.json:
            names = [name for name in rep if name != "per_image"]      # before, after and what else the operation counts
            with open(args.json, "w") as f:
                json.dump({**{name: rep[name] for name in names},
                           "per_image": [{"image_id": i, **dict(zip(names, v))} for i, v in rep["per_image"].items()]}, f)
        return 0
    try:
        thresholds = [float(v) for v in args.iou.split(",") if v.strip()]
        for d in (args.dir_a, args.dir_b):
            if not os.path.isdir(d):
                raise FileNotFoundError(f"{d}: no such directory")
        report = compare(args.dir_a, args.dir_b, thresholds)
    except (OSError, ValueError) as e:
        raise SystemExit(f"hybridgl_amd.proposals: {e}")
    s = report["summary"]
    fmt = lambda v: "-" if v is None else format(v, ".6f")
    print(f"images: {s['n_images']}   only in A: {len(s['only_in_a'])}   only in B: {len(s['only_in_b'])}"
          + (f"   size mismatch: {len(s['size_mismatch'])}" if s["size_mismatch"] else ""))
    print(f"masks: A {s['n_a']}, B {s['n_b']}, identical {s['identical']}")
    for t, (ka, kb) in s["at_iou"].items():
        print(f"IoU >= {t:g}: {ka} of A, {kb} of B have a partner")
    print(f"best IoU of A: mean {fmt(s['mean_iou_a'])}, min {fmt(s['min_iou_a'])};  of B: mean {fmt(s['mean_iou_b'])}, min {fmt(s['min_iou_b'])}")
    for iid, r in report["per_image"].items():
        if r["identical"] != r["n_a"] or r["n_a"] != r["n_b"]:
            print(f"  image {iid}: A {r['n_a']}, B {r['n_b']}, identical {r['identical']}, min best IoU {fmt(r['min_iou_a'])} / {fmt(r['min_iou_b'])}")
    for name in ("only_in_a", "only_in_b", "size_mismatch"):
        for iid in s[name]:
            print(f"  {name.replace('_', ' ')}: image {iid}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(_jsonable(report), f)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
