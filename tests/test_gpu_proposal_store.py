"""The proposal store (hybridgl_amd/proposals.py) in the evaluation loop, on the tiny REFER set and the tiny SAM of
tests/test_gpu_run.py: recording beside a run changes nothing; a run from the store, with no SAM anywhere, reproduces the
run that wrote it bit for bit (grouped and ref by ref); the files are generate()'s coco_rle records; crop layers; the two
driver flags; the errors of a store that does not match its dataset."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dataset(root, n_images=9):
    """REFER directory layout with `n_images` images of different sizes and 1-3 refs per image, the refs in round-robin order
    over the images (first refs of all images, then second refs, ...): images come back after other images"""
    from PIL import Image
    from hybridgl_amd.synth import synth_image
    (root / "refcoco").mkdir(parents=True)
    img_dir = root / "images/mscoco/images/train2014"
    img_dir.mkdir(parents=True)
    images, anns, refs = [], [], []
    rid = 200
    for i in range(n_images):
        h, w = 96 + 16 * (i % 4), 128 + 24 * (i % 3)
        name = f"COCO_train2014_{i:012d}.png"
        Image.fromarray(synth_image(h, w, 70 + i)).save(img_dir / name)
        images.append({"id": 10 + i, "file_name": name, "height": h, "width": w})
        for j in range(1 + i % 3):
            aid = 1000 + rid
            x0 = 8 + 20 * j
            anns.append({"id": aid, "image_id": 10 + i, "category_id": 1,
                         "segmentation": [[x0, 12, x0 + 70, 15, x0 + 60, h - 10, x0 + 5, h - 20]], "bbox": [0, 0, 1, 1]})
            sents = [{"sent_id": 2 * rid, "raw": "the cat on left", "tokens": []}]
            if (i + j) % 2:
                sents.append({"sent_id": 2 * rid + 1, "raw": "a big dog", "tokens": []})
            refs.append({"ref_id": rid, "ann_id": aid, "image_id": 10 + i, "category_id": 1, "split": "val",
                         "sent_ids": [s["sent_id"] for s in sents], "sentences": sents})
            rid += 1
    by_img = {}
    for r in refs:
        by_img.setdefault(r["image_id"], []).append(r)
    refs = [rs[k] for k in range(3) for rs in by_img.values() if k < len(rs)]
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "thing"}]},
              open(root / "refcoco/instances.json", "w"))
    pickle.dump(refs, open(root / "refcoco/refs(unc).p", "wb"))
    parse = {}
    for r in refs:
        parse[str(r["sent_ids"][0])] = {"noun_phrase": "the cat", "other_nouns": ["left"], "dirflag": "left", "relaflag": "left"}
        if len(r["sent_ids"]) > 1:
            parse[str(r["sent_ids"][1])] = {"noun_phrase": "dog", "other_nouns": [], "dirflag": "none", "relaflag": "big"}
    json.dump(parse, open(root / "parse.json", "w"))
    return refs


def _flags(root, golden_dir, *more):
    return ["--real", "--refer_data_root", str(root), "--dataset", "refcoco", "--split", "val",
            "--bpe_vocab", os.path.join(golden_dir, "tiny_bpe_vocab.txt.gz"), "--parse_json", str(root / "parse.json"),
            "--heatmap", "device"] + list(more)


def _sparse_threshold(sam, gen, cuda):
    """random weights give noise logits whose masks at threshold 0 all span the image (one survivor of the NMS): a mask
    threshold at the 99.95 % quantile leaves a handful of pixels per candidate, so the boxes differ and the NMS decides"""
    from hybridgl_amd.sam import SamPredictor
    from hybridgl_amd.synth import synth_image
    pred = SamPredictor(sam)
    pred.set_image(torch.from_numpy(synth_image(96, 128, 70)).to(cuda))
    pts = torch.from_numpy(pred.transform.apply_coords(gen.point_grids[0] * np.array([[128, 96]]), (96, 128)))[:, None, :]
    logits, _, _ = pred.predict_torch(pts, torch.ones((len(pts), 1), dtype=torch.int64), return_logits=True)
    return float(torch.quantile(logits.flatten()[:4_000_000].float(), 0.9995))


def _same(a, b):
    """equal record lists (the stability of an empty mask is NaN on both sides)"""
    return json.dumps(a) == json.dumps(b)


class World:
    pass


@pytest.fixture(scope="module")
def world(cuda, golden_dir, tmp_path_factory):
    """the models, the data set, a plain run, the same run with the recorder (it writes the store the other tests read) and
    SAM's own masks and boxes of every image"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.gem import create_gem_model
    from hybridgl_amd.loader import Prefetcher
    from hybridgl_amd.pipeline import HybridGLPipeline
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, sam_model_registry
    w = World()
    w.model = CLIPViTFM("ViT-B/16", seed=0, device=cuda)
    w.gem = create_gem_model("ViT-B/16", clip=w.model)
    w.sam = sam_model_registry["tiny"](device=cuda)
    w.gen = SamAutomaticMaskGenerator(w.sam, points_per_side=5, pred_iou_thresh=-1.0, stability_score_thresh=0.0, box_nms_thresh=0.7,
                                      min_mask_region_area=2)
    w.sam.mask_threshold = _sparse_threshold(w.sam, w.gen, cuda)
    w.root = tmp_path_factory.mktemp("refer_data")
    w.refs = _dataset(w.root)
    w.args = drv.default_argument_parser().parse_args(_flags(w.root, golden_dir))
    w.rr = drv.RealRefs(w.args, cuda, "unc", 77)
    w.mk = lambda gen: HybridGLPipeline(w.model, fusion_mode="G2L", masking_block=9, mask_generator=gen, use_sam_masks=True, gem_model=w.gem)
    w.loader = lambda: Prefetcher(w.rr.jobs(), w.rr.load, workers=4, depth=12, device=cuda)
    w.plain = w.mk(w.gen)
    assert w.plain.run(w.loader(), group=8) == len(w.refs)
    w.store = str(tmp_path_factory.mktemp("store"))
    w.recorder = P.ProposalRecorder(w.gen, w.store, P.generator_settings(w.gen, sam_model="tiny", precision="f16x3", proposal_cap=0))
    w.recorded = w.mk(w.recorder)
    assert w.recorded.run(w.loader(), group=8) == len(w.refs)
    w.recorder.flush()
    torch.cuda.synchronize()
    w.images, w.sam_out = {}, {}
    for i in w.rr.jobs():
        r = w.rr.load(i)
        if r.image_id not in w.images:
            w.images[r.image_id] = r.sam_img
            m, xywh = w.gen.generate_group([r.sam_img])[0][:2]
            w.sam_out[r.image_id] = (m.clone(), xywh.clone())
    return w


def test_recording_changes_nothing(world):
    """(a) rows and report of the wrapped run are the plain run's; one file per image and meta.json; ragged counts"""
    w = world
    assert np.array_equal(w.plain.partial_rows(), w.recorded.partial_rows())
    assert w.plain.metrics() == w.recorded.metrics()
    assert (w.plain.cache_hits, w.plain.skipped) == (w.recorded.cache_hits, w.recorded.skipped)
    counts = [int(m.shape[0]) for m, _ in w.sam_out.values()]
    assert len(set(counts)) >= 3, f"the proposal counts should be ragged, got {counts}"
    assert sorted(os.listdir(w.store)) == sorted([f"{i}.json" for i in w.images] + ["meta.json"])
    assert w.recorder.written == len(w.images) and not w.recorder._pending
    meta = json.load(open(os.path.join(w.store, "meta.json")))
    assert meta["points_per_side"] == [5] and meta["min_mask_region_area"] == 2 and meta["sam_model"] == "tiny"
    assert meta["mask_threshold"] == w.sam.mask_threshold and meta["box_nms_thresh"] == 0.7 and meta["crop_n_layers"] == 0


def test_a_stored_run_reproduces_it(world, cuda, monkeypatch):
    """(b) StoredProposals in place of the generator, no Sam constructed: the rows of the run that wrote the store, in groups
    of 8 and of 3 and ref by ref through step(); per image SAM's masks and boxes; returning images come from the image cache"""
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world

    def no_sam(*a, **k):
        raise AssertionError("a Sam model was constructed")

    monkeypatch.setattr(hsam.Sam, "__init__", no_sam)
    want = w.plain.partial_rows()
    for group in (8, 3):
        sp = P.StoredProposals(w.store, cuda)
        w.rr.proposals = sp      # files, JSON and packing on the loader threads
        try:
            p = w.mk(sp)
            assert p.run(w.loader(), group=group) == len(w.refs)
        finally:
            w.rr.proposals = None
        torch.cuda.synchronize()
        assert np.array_equal(p.partial_rows(), want), group
        assert p.metrics() == w.plain.metrics() and p.skipped == 0
        assert p.cache_hits > 0 and (group != 8 or p.cache_hits == w.plain.cache_hits)
        assert len(w.images) <= sp.loaded <= len(w.refs)      # parsed when the loader threads met the image, kept for its other refs
    sp = P.StoredProposals(w.store, cuda)
    p = w.mk(sp)
    for i in w.rr.jobs():
        p.step(w.rr.load(i))
    torch.cuda.synchronize()
    assert np.array_equal(p.partial_rows(), want)
    ids = list(w.images)
    out = sp.generate_group([w.images[i] for i in ids], ids)
    for iid, (m, xywh, iou, stab, src) in zip(ids, out):
        assert m.dtype == torch.uint8 and xywh.dtype == torch.int64 and src is None
        assert torch.equal(m, w.sam_out[iid][0]) and torch.equal(xywh, w.sam_out[iid][1]), iid
        recs = sp.records(iid)
        assert np.array_equal(iou.cpu().numpy(), np.array([r["predicted_iou"] for r in recs], np.float32))
        assert np.array_equal(stab.cpu().numpy(), np.array([r["stability_score"] for r in recs], np.float32), equal_nan=True)
    # cap: the first entries
    capped = sp.generate_group([w.images[ids[0]]], ids[:1], cap=2)[0]
    assert torch.equal(capped[0], w.sam_out[ids[0]][0][:2]) and torch.equal(capped[1], w.sam_out[ids[0]][1][:2])
    with pytest.raises(ValueError, match="image_id"):
        sp.generate_device(w.images[ids[0]])


def test_records_are_what_generate_returns(world, tmp_path):
    """(c) records(id) == generate(image) in coco_rle mode, for two images recorded ref by ref through step().

    generate() and step() both take an image through generate_device: Sam.encode of the one image.  The grouped loop encodes
    with Sam.encode_batch, which equals Sam.encode only up to the summation order of split-K (one image's mlp.lin2 runs
    split-K, a batch's does not: tests/test_gpu_group_tail.py::test_group_of_mixed_sizes_equals_image_by_image measures a few
    1e-6 on the embedding and, with it, the last bits of the predicted IoUs).  A store the grouped loop wrote therefore holds the
    grouped loop's predicted_iou bits -- (b) holds it to them -- and the one step() wrote holds generate()'s, every bit."""
    from hybridgl_amd import proposals as P
    w = world
    rec = P.ProposalRecorder(w.gen, tmp_path / "by_step")
    pipe = w.mk(rec)
    ids = []
    for i in w.rr.jobs():
        ref = w.rr.load(i)
        if ref.image_id in ids:
            continue
        pipe.step(ref)
        ids.append(ref.image_id)
        if len(ids) == 2:
            break
    assert rec.flush() == 2
    store = P.ProposalStore(tmp_path / "by_step")
    w.gen.output_mode = "coco_rle"
    try:
        for iid in ids:
            want = w.gen.generate(w.images[iid])
            got = store.records(iid)
            assert len(got) == len(want) > 0 and _same(got, want), iid
    finally:
        w.gen.output_mode = "binary_mask"


def test_crop_layers_round_trip(world, cuda, tmp_path):
    """(d) one image through a generator with a crop layer: recorded from the three calls and from step()'s call, read back"""
    from hybridgl_amd import proposals as P
    from hybridgl_amd.sam import SamAutomaticMaskGenerator
    from hybridgl_amd.synth import synth_image
    w = world
    img = torch.from_numpy(synth_image(150, 200, 11)).to(cuda)
    gen = SamAutomaticMaskGenerator(w.sam, points_per_side=6, points_per_batch=16, pred_iou_thresh=0.0, stability_score_thresh=0.0,
                                    crop_n_layers=1, crop_n_points_downscale_factor=2, min_mask_region_area=10, output_mode="coco_rle")
    rec = P.ProposalRecorder(gen, tmp_path / "crops", P.generator_settings(gen))
    a = rec.group_finish(rec.group_cleanup(rec.group_begin([img], None, None, image_ids=[77])))[0]
    b = rec.generate_device_crops(img, image_id=78)
    assert rec.flush() == 2
    want = gen.generate(img)
    n = a[0].shape[0]
    assert n > 4 and len({tuple(r["crop_box"]) for r in want}) > 1, "the survivors should come from more than one crop"
    sp = P.StoredProposals(tmp_path / "crops", cuda)
    assert _same(sp.records(77), want) and _same(sp.records(78), want)
    assert sp.settings()["crop_n_layers"] == 1 and sp.settings()["points_per_side"] == [6, 3]
    for iid in (77, 78):
        m, xywh, iou, stab, _ = sp.generate_device(img, image_id=iid)
        assert torch.equal(m, a[0]) and torch.equal(xywh, a[1]) and torch.equal(iou, a[2])
        assert torch.equal(torch.nan_to_num(stab, nan=-7.0), torch.nan_to_num(a[3], nan=-7.0))
    assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[1])


def test_the_driver_flags(world, cuda, golden_dir, tmp_path, monkeypatch, capsys):
    """(e) --save_proposals under G2L, then --proposals_dir --fusion_mode L2G with no SAM model built: the report of a full
    L2G run"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    store = str(tmp_path / "props")
    base = _flags(w.root, golden_dir, "--sam_model", "tiny", "--points_per_side", "5", "--pred_iou_thresh", "-1.0",
                  "--stability_score_thresh", "0", "--min_mask_region_area", "2", "--group", "4", "--workers", "2",
                  "--result_dir", str(tmp_path / "log"), "--max_refs", "9")
    parse = drv.default_argument_parser().parse_args
    save = parse(base + ["--fusion_mode", "G2L", "--save_proposals", store, "--save_masks", str(tmp_path / "masks")])
    drv.resolve_defaults(save)
    save.precision = "f16x3"
    m_save, st = drv.evaluate(save, w.model, w.gen, w.gem, cuda)
    assert st["proposals_saved"] == 9 and len(os.listdir(store)) == 10
    assert os.path.exists(tmp_path / "masks" / "masks.rank0.jsonl")

    def no_sam(*a, **k):
        raise AssertionError("a Sam model was constructed")

    monkeypatch.setattr(hsam.Sam, "__init__", no_sam)
    read = parse(base + ["--fusion_mode", "L2G", "--proposals_dir", store])
    model, gen, gem = drv.build_models(read, cuda)
    assert isinstance(gen, P.StoredProposals)
    m_read, st_read = drv.evaluate(read, w.model, gen, w.gem, cuda)
    monkeypatch.undo()
    assert st_read["proposal_store"]["sam_model"] == "tiny" and st_read["proposal_store"]["points_per_side"] == [5]
    assert gen.loaded == 9
    full = parse(base + ["--fusion_mode", "L2G"])
    drv.resolve_defaults(full)
    full.precision = read.precision
    m_full, _ = drv.evaluate(full, w.model, w.gen, w.gem, cuda)
    assert m_read == m_full and m_read["n_sentences"] > 9
    assert drv.report_text(read, m_read, read.precision) == drv.report_text(full, m_full, full.precision)
    assert m_save["n_sentences"] == m_full["n_sentences"]
    both = parse(base + ["--save_proposals", store, "--proposals_dir", store])
    with pytest.raises(SystemExit):
        drv.build_models(both, cuda)


def test_a_store_that_does_not_match_is_refused(world, cuda, tmp_path):
    """(f) a removed file, a wrong size, a corrupted count and a bbox that is not the mask's: ValueError with image and entry"""
    import shutil
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    store = str(tmp_path / "copy")
    shutil.copytree(w.store, store)
    ids = list(w.images)
    iid = next(i for i in ids if w.sam_out[i][0].shape[0] >= 2)
    img = w.images[iid]
    path = os.path.join(store, f"{iid}.json")
    good = json.load(open(path))

    def load_with(recs):
        json.dump(recs, open(path, "w"))
        return P.StoredProposals(store, cuda).generate_group([img], [iid])

    assert torch.equal(load_with(good)[0][0], w.sam_out[iid][0])
    H, W = good[1]["segmentation"]["size"]
    bad = json.loads(json.dumps(good))
    bad[1]["segmentation"]["size"] = [W, H] if H != W else [H, W + 1]
    with pytest.raises(ValueError, match=f"image {iid} entry 1: size"):
        load_with(bad)
    counts = hsam.rle_counts_from_string(good[1]["segmentation"]["counts"]).tolist()
    short = hsam.coco_encode_rle({"size": [H, W], "counts": counts[:-1] + [counts[-1] - 1]})["counts"]
    bad = json.loads(json.dumps(good))
    bad[1]["segmentation"]["counts"] = short      # the counts stop one pixel short of H*W
    with pytest.raises(ValueError, match=f"image {iid} entry 1: its counts do not decode"):
        load_with(bad)
    bad[1]["segmentation"]["counts"] = good[1]["segmentation"]["counts"] + "o"      # a group cut off by the end of the string
    with pytest.raises(ValueError, match=f"image {iid} entry 1: bad counts string"):
        load_with(bad)
    bad = json.loads(json.dumps(good))
    k = next(j for j, r in enumerate(good) if r["area"] > 0)
    bad[k]["bbox"][2] += 1
    with pytest.raises(ValueError, match=f"image {iid} entry {k}: the stored bbox"):
        load_with(bad)
    os.remove(path)
    sp = P.StoredProposals(store, cuda)
    w.rr.proposals = None
    with pytest.raises(ValueError, match=f"image {iid} has no file"):
        w.mk(sp).run((w.rr.load(i) for i in w.rr.jobs()), group=4)
    torch.cuda.synchronize()
