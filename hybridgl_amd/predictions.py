"""Saved predictions: the `masks.rank*.jsonl` files that `python -m hybridgl_amd.main --save_masks DIR` writes, read back,
scored against ground truth and compared set against set -- on the device, on run lengths (ops.rle_pack / ops.rle_iou: the
strings' counts cross the bus, no mask is expanded to bytes).

    records = predictions.load("runA")                        # [{"index", "sentence", "size", "pure", "final", "I", ...}]
    report = predictions.compare("runA", "runB")              # or two loaded sets
    python -m hybridgl_amd.predictions compare runA runB [--json OUT]
    voted = predictions.ensemble(["runA", "runB", "runC"], rule="majority")   # [{"index", "sentence", "size", "pure", "final"}]
    python -m hybridgl_amd.main <dataset flags> --ensemble_masks runA runB runC --ensemble_out OUT   # voted, scored and saved

Any producer that writes the same lines (the reference's own winners included) can be compared in the same way.
"""
import glob
import json
import os

import numpy as np

KEYS = ("index", "sentence", "size", "pure", "final", "I", "U", "I_final", "U_final")
MASKS = ("pure", "final")


def _check_record(rec, where):
    if not isinstance(rec, dict) or set(rec) != set(KEYS):
        raise ValueError(f"{where}: expected the keys {sorted(KEYS)}, got {sorted(rec) if isinstance(rec, dict) else type(rec).__name__}")
    for k in ("index", "sentence", "I", "U", "I_final", "U_final"):
        if isinstance(rec[k], bool) or not isinstance(rec[k], int):
            raise ValueError(f"{where}: {k!r} must be an integer, got {rec[k]!r}")
    size = rec["size"]
    if (not isinstance(size, list) or len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v <= 0 for v in size)
            or size[0] * size[1] >= 1 << 31):
        raise ValueError(f"{where}: 'size' must be [H, W] with positive integers and H*W < 2^31, got {size!r}")
    for k in MASKS:
        if not isinstance(rec[k], str):
            raise ValueError(f"{where}: {k!r} must be a COCO RLE string, got {type(rec[k]).__name__}")


def load(directory):
    """Every record of DIR/masks.rank*.jsonl (the files of all ranks are one job's predictions), sorted by (index, sentence).
    Raises ValueError on a record whose keys or size are malformed and on a key that occurs twice, FileNotFoundError when the
    directory holds no such file."""
    paths = sorted(glob.glob(os.path.join(os.fspath(directory), "masks.rank*.jsonl")))
    if not paths:
        raise FileNotFoundError(f"{directory}: no masks.rank*.jsonl")
    seen, out = {}, []
    for path in paths:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if not line.strip():
                    continue
                where = f"{path}:{no}"
                try:
                    rec = json.loads(line)
                except json.JSONDecodeError as e:
                    raise ValueError(f"{where}: not JSON ({e})") from None
                _check_record(rec, where)
                key = (rec["index"], rec["sentence"])
                if key in seen:
                    raise ValueError(f"{where}: (index, sentence) = {key} already occurs at {seen[key]}")
                seen[key] = where
                out.append(rec)
    out.sort(key=lambda r: (r["index"], r["sentence"]))
    return out


def _by_key(records):
    return {(r["index"], r["sentence"]): r for r in records}


def _pack(strings, H, W, device):
    from . import ops
    from .sam import rle_counts_from_string
    return ops.rle_pack([rle_counts_from_string(s) for s in strings], H, W, device=device)


def _stack_masks(targets, H, W):
    """mask targets [H,W] bool / uint8 as one uint8 [n,H,W] for ops.rle_encode (a bool tensor is reinterpreted, not converted)"""
    import torch
    return torch.stack([t.reshape(H, W).to(torch.uint8) if t.dtype != torch.bool else t.reshape(H, W).view(torch.uint8) for t in targets])


def _polygon_runs(who, names, entries, sizes, counts, device=None):
    """(slots, table) of polygon targets, rasterised on the device by ONE ops.rle_from_polygons call (sizes, counts: its images);
    ValueError in the name of the caller `who` for the first entry that is refused, which names[k] names"""
    from . import ops
    slots, table, status = ops.rle_from_polygons(entries, sizes, counts, rule="once", device=device)
    code = status.cpu().numpy()[:, 0]
    if (code != 0).any():
        k = int(np.flatnonzero(code != 0)[0])
        raise ValueError(f"{who}: the polygons of {names[k]} are refused (status {int(code[k])})")
    return slots, table


def _batches(keys, by_size_of, batch):
    """keys grouped by image size, at most `batch` per group: [((H, W), [key, ...])]"""
    groups = {}
    for k in keys:
        groups.setdefault(tuple(by_size_of(k)), []).append(k)
    return [(hw, ks[i:i + batch]) for hw, ks in sorted(groups.items()) for i in range(0, len(ks), batch)]


def compare(a, b, device=None, batch=256):
    """Two sets of predictions (loaded records, or directories), mask by mask: for every key in both sets the intersection
    and union of the two `pure` masks and of the two `final` masks (ops.rle_iou).  Returns {"summary": {n_common, only_in_a,
    only_in_b, identical_pure, identical_final, min_iou_pure, min_iou_final, differ_pure, differ_final, size_mismatch},
    "per_key": {(index, sentence): {"pure": (I, U), "final": (I, U)}}}.  Two masks are identical when I == U (two empty masks
    included: their IoU counts as 1); keys whose records state different sizes are listed and not compared."""
    from . import ops
    a = _by_key(load(a) if isinstance(a, (str, os.PathLike)) else a)
    b = _by_key(load(b) if isinstance(b, (str, os.PathLike)) else b)
    common = sorted(set(a) & set(b))
    size_mismatch = [k for k in common if a[k]["size"] != b[k]["size"]]
    usable = [k for k in common if a[k]["size"] == b[k]["size"]]
    per_key = {}
    for (H, W), keys in _batches(usable, lambda k: a[k]["size"], batch):
        sa, ta = _pack([a[k][m] for m in MASKS for k in keys], H, W, device)
        sb, tb = _pack([b[k][m] for m in MASKS for k in keys], H, W, device)
        iu = ops.rle_iou(sa, ta, sb, tb, H, W).cpu().numpy().reshape(len(MASKS), len(keys), 2)
        for i, k in enumerate(keys):
            per_key[k] = {m: (int(iu[j, i, 0]), int(iu[j, i, 1])) for j, m in enumerate(MASKS)}
    summary = {"n_common": len(common), "only_in_a": sorted(set(a) - set(b)), "only_in_b": sorted(set(b) - set(a)),
               "size_mismatch": size_mismatch}
    for m in MASKS:
        differ = [k for k in usable if per_key[k][m][0] != per_key[k][m][1]]
        ious = [per_key[k][m][0] / per_key[k][m][1] if per_key[k][m][1] else 1.0 for k in usable]
        summary[f"identical_{m}"] = len(usable) - len(differ)
        summary[f"min_iou_{m}"] = min(ious) if ious else None
        summary[f"differ_{m}"] = differ
    return {"summary": summary, "per_key": per_key}


def score(records, targets, batch=32):
    """The metric rows of saved predictions against ground truth.  records: a loaded set; targets: an iterable of
    ((index, sentence), target) in any order, a target being a mask [H,W] bool / uint8 device tensor or a
    refer_io.PolygonTarget.  Mask targets are encoded on the device (ops.rle_encode); the polygon targets of a flush are
    rasterised on the device, straight into run lengths, by ONE ops.rle_from_polygons call and never become pixels.  Either
    way they are met by the saved strings' runs in ops.rle_iou: integer counts, exact.  Returns (rows [n,6] int64 =
    dist.ROW_FIELDS sorted by key, missing: target keys without a record, extra: record keys without a target)."""
    import torch
    from . import ops
    from .refer_io import PolygonTarget
    recs = _by_key(records)
    rows, missing, seen = [], [], set()

    def flush(H, W, items):
        keys = [k for k, _ in items]
        n = len(keys)
        if isinstance(items[0][1], PolygonTarget):      # a flush holds one kind of target
            s1, t1 = _polygon_runs("score", keys, [t.polygons for _, t in items], [(H, W)], [n])
            dev = s1.device
            sg, tg = s1.repeat(len(MASKS), 1), t1.repeat(len(MASKS), 1)
        else:
            gt = _stack_masks([t for _, t in items], H, W)
            dev = gt.device
            sel = torch.arange(n, device=dev).repeat(len(MASKS))
            sg, tg = ops.rle_encode(gt, sel)
        sp, tp = _pack([recs[k][m] for m in MASKS for k in keys], H, W, dev)
        iu = ops.rle_iou(sp, tp, sg, tg, H, W).cpu().numpy().reshape(len(MASKS), n, 2)
        if (iu < 0).any():
            raise ValueError(f"score: a saved mask of {keys[int(np.argwhere(iu < 0)[0][1])]} does not decode")
        for i, k in enumerate(keys):
            rows.append([k[0], k[1], iu[0, i, 0], iu[0, i, 1], iu[1, i, 0], iu[1, i, 1]])

    pending = {}
    for key, t in targets:
        key = (int(key[0]), int(key[1]))
        if key in seen:
            raise ValueError(f"score: two targets for {key}")
        seen.add(key)
        if key not in recs:
            missing.append(key)
            continue
        H, W = (int(v) for v in t.shape[-2:])
        if recs[key]["size"] != [H, W]:
            raise ValueError(f"score: the record of {key} states size {recs[key]['size']}, its target is {[H, W]}")
        kind = (H, W, isinstance(t, PolygonTarget))
        q = pending.setdefault(kind, [])
        q.append((key, t))
        if len(q) >= batch:
            flush(H, W, pending.pop(kind))
    for (H, W, _), q in sorted(pending.items()):
        flush(H, W, q)
    rows = np.asarray(sorted(rows), dtype=np.int64).reshape(-1, 6)
    return rows, sorted(missing), sorted(set(recs) - seen)


def ensemble(sets, rule="majority", weights=None, device=None, batch=64):
    """Two or more saved runs voted into one prediction.  sets: loaded record lists or directories; every set must hold the same
    (index, sentence) keys and state the same size for each -- an ensemble over different sentences is not a run (ValueError).
    For every key the `pure` masks of all sets are voted into one mask and the `final` masks into another: rule is a name of
    ops.rle_merge_rule ("majority", "union", "intersect", "at_least:T", "exactly:T") over k = sum(weights) votes; weights: one
    non-negative integer per set (default 1 each), expressed by listing a set's mask that many times.  The strings' runs cross
    the bus (ops.rle_pack), the vote happens on bit planes (ops.rle_merge: one call per `batch` <= 64 image sizes, every size an
    image of the call) and runs come back: no mask becomes pixels, and the output slots hold ceil(H*W/32) words, so no mask is
    ever lost.  Returns records {"index", "sentence", "size", "pure", "final"} (COCO strings) sorted by key; score() fills in
    the counts that save() writes."""
    from . import ops
    from .sam import coco_encode_rle, rle_counts_from_string, rle_from_slot
    sets = [_by_key(load(s) if isinstance(s, (str, os.PathLike)) else s) for s in sets]
    if len(sets) < 2:
        raise ValueError(f"ensemble: {len(sets)} set(s); a vote takes at least two")
    weights = [1] * len(sets) if weights is None else list(weights)
    if len(weights) != len(sets) or any(isinstance(w, bool) or not isinstance(w, int) or w < 0 for w in weights):
        raise ValueError(f"ensemble: weights {weights!r} (one non-negative integer per set, {len(sets)} sets)")
    if not 1 <= int(batch) <= 64:
        raise ValueError(f"ensemble: batch {batch} (1 .. 64 image sizes per call)")
    keys = sorted(sets[0])
    for i, s in enumerate(sets[1:], 1):
        if set(s) != set(keys):
            odd = sorted(set(s) ^ set(keys))[0]
            raise ValueError(f"ensemble: set {i} and set 0 do not hold the same keys (index {odd[0]} sentence {odd[1]} is in one only)")
        for k in keys:
            if s[k]["size"] != sets[0][k]["size"]:
                raise ValueError(f"ensemble: index {k[0]} sentence {k[1]} has size {s[k]['size']} in set {i} and "
                                 f"{sets[0][k]['size']} in set 0")
    votes = int(sum(weights))
    bounds = ops.rle_merge_rule(rule, votes)
    by_size = {}
    for k in keys:
        by_size.setdefault(tuple(sets[0][k]["size"]), []).append(k)
    sizes = sorted(by_size)
    out = {}
    for c in range(0, len(sizes), int(batch)):
        chunk = sizes[c:c + int(batch)]
        strings, members, order = [], [], []
        for hw in chunk:
            for k in by_size[hw]:
                for m in MASKS:
                    first = len(strings)
                    strings += [s[k][m] for s in sets]
                    members.append([first + i for i, w in enumerate(weights) for _ in range(w)])
                    order.append((k, m, hw))
        n_src = [len(by_size[hw]) * len(MASKS) * len(sets) for hw in chunk]
        n_out = [len(by_size[hw]) * len(MASKS) for hw in chunk]
        # one packed set for all sizes of the call: rle_pack's size only guards its own arguments, the table rows carry none
        slots, table = ops.rle_pack([rle_counts_from_string(s) for s in strings], chunk[0][0], chunk[0][1], device=device)
        res = ops.rle_merge(slots, table, chunk, n_src, members, None, [bounds] * len(members), n_out)
        s_out, t_out, status = (x.cpu().numpy() for x in res)
        for e, (k, m, (H, W)) in enumerate(order):
            if status[e, 0] == 2:
                raise ValueError(f"ensemble: a saved {m!r} mask of index {k[0]} sentence {k[1]} does not decode")
            counts = rle_from_slot(s_out[e], int(t_out[e, 0]), int(t_out[e, 1]), H, W)
            out.setdefault(k, {})[m] = coco_encode_rle({"size": [H, W], "counts": counts})["counts"]
    return [{"index": k[0], "sentence": k[1], "size": list(sets[0][k]["size"]), **out[k]} for k in keys]


def save(records, directory, rank=0):
    """DIR/masks.rank{rank}.jsonl, one JSON line per record with the keys load() reads back (KEYS, in that order): what
    main.py --save_masks writes for a run and --ensemble_out for a vote.  Returns the path."""
    records = list(records)
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(os.fspath(directory), f"masks.rank{rank}.jsonl")
    for i, rec in enumerate(records):
        _check_record(rec, f"save: record {i}")
    with open(path, "w") as f:
        for rec in records:
            f.write(json.dumps({k: rec[k] for k in KEYS}) + "\n")
    return path


def _jsonable(report):
    s = dict(report["summary"])
    for k in ("only_in_a", "only_in_b", "size_mismatch", "differ_pure", "differ_final"):
        s[k] = [list(v) for v in s[k]]
    return {"summary": s, "per_key": [{"index": k[0], "sentence": k[1], **{m: list(v[m]) for m in MASKS}}
                                      for k, v in sorted(report["per_key"].items())]}


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m hybridgl_amd.predictions", description="saved predictions (main.py --save_masks)")
    sub = p.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compare", help="two saved sets, mask by mask")
    c.add_argument("dir_a")
    c.add_argument("dir_b")
    c.add_argument("--json", default="", metavar="OUT", help="also write the summary and the per-key counts here")
    args = p.parse_args(argv)
    try:
        a, b = load(args.dir_a), load(args.dir_b)
    except (OSError, ValueError) as e:
        raise SystemExit(f"hybridgl_amd.predictions: {e}")
    report = compare(a, b)
    s = report["summary"]
    print(f"common: {s['n_common']}   only in A: {len(s['only_in_a'])}   only in B: {len(s['only_in_b'])}"
          + (f"   size mismatch: {len(s['size_mismatch'])}" if s["size_mismatch"] else ""))
    for m in MASKS:
        lo = s[f"min_iou_{m}"]
        print(f"{m}: identical {s[f'identical_{m}']}, min IoU {'-' if lo is None else format(lo, '.6f')}")
        for k in s[f"differ_{m}"]:
            i, u = report["per_key"][k][m]
            print(f"  {m} differs at index {k[0]} sentence {k[1]}: I = {i}, U = {u}")
    for name in ("only_in_a", "only_in_b"):
        for k in s[name]:
            print(f"  {name.replace('_', ' ')}: index {k[0]} sentence {k[1]}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(_jsonable(report), f)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
