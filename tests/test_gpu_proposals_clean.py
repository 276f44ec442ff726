"""proposals.clean on the GPU: postprocess_small_regions on a store.  (a) A synthetic store written from the connected-component
case masks, cleaned, against the numpy statement of the step: flood fill holes, flood fill islands (tests/rle_clean_cases.py),
the boxes taken again, scores 1.0 / 0.0, the float32 box NMS of tests/nms_cases.py, the kept records in its order, the changed
ones re-encoded.  (b) The tiny SAM generator in coco_rle mode: its records at min_mask_region_area = 0, cleaned at A, are
record for record the records of the same generator at min_mask_region_area = A.  Then the command line and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import nms_cases as NMS
import rle_clean_cases as RC

pytestmark = pytest.mark.gpu

MIN_AREA = 20
SHAPES = {3: (65, 33), 8: (37, 130), 21: (129, 65)}
EMPTY = 11
# (b): the area at which the tiny generator's records split into changed and unchanged ones -- found on the GPU: the noise masks
# of random weights are speckled, so of the 108 + 108 records of the two images below A = 2 (single pixels) changes 108 + 107 and
# leaves one as it was; A = 1 changes none and every A >= 3 all of them
SAM_AREA = 2


def record(m, k):
    from hybridgl_amd import sam as hsam
    H, W = m.shape
    x0, y0, x1, y1 = RC.box_of(m)
    return {"segmentation": hsam.coco_encode_rle({"size": [H, W], "counts": RC.counts_of(m).tolist()}), "area": int(m.sum()),
            "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": 0.5 + k / 1000.0, "point_coords": [[float(k), 1.5]],
            "stability_score": 0.9, "crop_box": [0, 0, W, H]}


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    from hybridgl_amd import proposals as P

    class World:
        pass

    w = World()
    w.src = str(tmp_path_factory.mktemp("src"))
    store = P.ProposalStore(w.src)
    w.masks = {}
    for iid, shape in SHAPES.items():
        seen, masks = set(), []
        for _, m, _ in RC.pairs():
            if m.shape == shape and m.tobytes() not in seen:
                seen.add(m.tobytes())
                masks.append(m)
        w.masks[iid] = masks
        store.write(iid, [record(m, k) for k, m in enumerate(masks)])
    store.write(EMPTY, [])
    store.write_meta({"sam_model": "none", "min_mask_region_area": 0})
    w.dst = str(tmp_path_factory.mktemp("clean") / "a20")
    w.report = P.clean(w.src, w.dst, MIN_AREA, 0.7, group=3, device=cuda)
    return w


def statement(masks, recs, min_area, thr):
    """postprocess_small_regions in numpy -> the records it leaves"""
    from hybridgl_amd import sam as hsam
    wants = [RC.clean(m, min_area, "both") for m in masks]
    boxes = np.asarray([w["box"] for w in wants], np.int32)
    scores = np.asarray([0.0 if w["result"][2] else 1.0 for w in wants], np.float32)
    out = []
    for i in NMS.greedy_nms(boxes, scores, np.ones(len(masks), np.uint8), thr):
        r, w = recs[i], wants[i]
        if w["result"][2]:
            H, W = masks[i].shape
            x0, y0, x1, y1 = w["box"]
            r = dict(r, segmentation=hsam.coco_encode_rle({"size": [H, W], "counts": RC.counts_of(w["mask"]).tolist()}),
                     area=int(w["mask"].sum()), bbox=[x0, y0, x1 - x0, y1 - y0])
        out.append(r)
    return out, wants


def test_a_synthetic_store_against_the_numpy_statement(world, cuda):
    from hybridgl_amd import proposals as P
    w = world
    src, dst = P.ProposalStore(w.src), P.ProposalStore(w.dst)
    assert dst.image_ids() == sorted(list(SHAPES) + [EMPTY]) and dst.records(EMPTY) == [] and w.report["per_image"][EMPTY] == [0, 0, 0]
    changed = unchanged = dropped = 0
    for iid in SHAPES:
        recs = src.records(iid)
        want, wants = statement(w.masks[iid], recs, MIN_AREA, 0.7)
        got = dst.records(iid)
        assert json.dumps(got) == json.dumps(want), iid
        n_changed = sum(1 for r in got if r not in recs)
        assert w.report["per_image"][iid][:2] == [len(recs), len(want)] and w.report["per_image"][iid][2] >= n_changed
        changed, unchanged, dropped = changed + n_changed, unchanged + len(got) - n_changed, dropped + len(recs) - len(got)
        # the unchanged ones come first (score 1.0), each group in stored order; an unchanged record is the stored one, whole
        order = [recs.index(next(r for r in recs if r["point_coords"] == g["point_coords"])) for g in got]
        first = [i for i in order if not wants[i]["result"][2]]
        assert order == first + [i for i in order if wants[i]["result"][2]] and first == sorted(first) and all(got[k] == recs[i] for k, i in enumerate(first))
    assert changed >= 5 and unchanged >= 5 and dropped >= 5      # of the statement's own records: the list exercises all three
    assert dst.meta() == dict(src.meta(), cleaned={"min_area": MIN_AREA, "nms_thresh": 0.7, "source": w.src})
    assert w.report["before"] == sum(len(m) for m in w.masks.values()) and w.report["after"] == w.report["before"] - dropped
    # min_area 0 and 1 change nothing; the NMS at 1.0 drops nothing: the store comes back record for record
    same = P.clean(w.src, os.path.join(os.path.dirname(w.dst), "a1"), 1, 1.0, device=cuda)
    assert same["after"] == same["before"] and same["changed"] == 0
    for iid in SHAPES:
        assert json.dumps(P.ProposalStore(os.path.join(os.path.dirname(w.dst), "a1")).records(iid)) == json.dumps(src.records(iid))


def test_the_tiny_generator_at_area_0_cleaned_equals_the_generator_at_area_a(cuda, tmp_path):
    from hybridgl_amd import proposals as P
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, SamPredictor, sam_model_registry
    from hybridgl_amd.synth import synth_image
    sam = sam_model_registry["tiny"](device=cuda)
    # box_nms_thresh 1.0: no box falls (the noise masks' boxes are nearly the image: any lower threshold leaves one record)
    kw = dict(points_per_side=6, pred_iou_thresh=-1.0, stability_score_thresh=-1.0, box_nms_thresh=1.0, output_mode="coco_rle")
    gen0 = SamAutomaticMaskGenerator(sam, min_mask_region_area=0, **kw)
    genA = SamAutomaticMaskGenerator(sam, min_mask_region_area=SAM_AREA, **kw)
    # random weights give noise logits: at their median a mask covers about half of the image
    pred = SamPredictor(sam)
    pred.set_image(torch.from_numpy(synth_image(96, 128, 70)).to(cuda))
    pts = torch.from_numpy(pred.transform.apply_coords(gen0.point_grids[0] * np.array([[128, 96]]), (96, 128)))[:, None, :]
    logits, _, _ = pred.predict_torch(pts, torch.ones((len(pts), 1), dtype=torch.int64), return_logits=True)
    sam.mask_threshold = float(torch.quantile(logits.flatten()[:4_000_000].float(), 0.5))
    images = {5: synth_image(96, 128, 105), 6: synth_image(150, 200, 106)}
    src = P.ProposalStore(tmp_path / "src")
    for iid, img in images.items():
        recs = gen0.generate(torch.from_numpy(img).to(cuda))
        assert json.dumps(gen0.generate(torch.from_numpy(img).to(cuda))) == json.dumps(recs) and len(recs) > 8      # two calls agree
        src.write(iid, recs)
    src.write_meta(P.generator_settings(gen0, sam_model="tiny"))
    for area in (SAM_AREA, 60):      # single pixels; and regions of a size that every record has
        genA.min_mask_region_area = area
        rep = P.clean(src, tmp_path / f"dst{area}", area, max(genA.box_nms_thresh, genA.crop_nms_thresh), device=cuda)
        dst = P.ProposalStore(tmp_path / f"dst{area}")
        n_same = n_all = 0
        for iid, img in images.items():
            want = genA.generate(torch.from_numpy(img).to(cuda))
            got = dst.records(iid)
            print(f"\narea {area} image {iid}: {rep['per_image'][iid]} (before, after, changed)")
            assert json.dumps(got) == json.dumps(json.loads(json.dumps(want))), (area, iid)
            stored = src.records(iid)
            n_same, n_all = n_same + sum(1 for r in got if r in stored), n_all + len(got)
        if area == SAM_AREA:
            assert 0 < n_same < n_all, (n_same, n_all)      # at least one record changed and one did not


def test_the_command_line_writes_the_same_store_and_the_refusals(world, tmp_path, capsys, cuda):
    from hybridgl_amd import proposals as P
    out = tmp_path / "cli"
    js = tmp_path / "rep.json"
    assert P.main(["clean", world.src, str(out), "--min_area", str(MIN_AREA), "--json", str(js)]) == 0
    assert f"proposals: {world.report['before']} -> {world.report['after']}" in capsys.readouterr().out
    a, b = P.ProposalStore(out), P.ProposalStore(world.dst)
    assert a.image_ids() == b.image_ids() and a.meta() == b.meta()
    for i in a.image_ids():
        assert open(a.path(i)).read() == open(b.path(i)).read()
    rep = json.load(open(js))
    assert rep["before"] == world.report["before"] and rep["after"] == world.report["after"] and len(rep["per_image"]) == len(SHAPES) + 1
    # the cases thin refuses
    with pytest.raises(ValueError):
        P.clean(world.src, world.src, MIN_AREA)
    with pytest.raises(ValueError):
        P.clean(world.src, world.dst, MIN_AREA)                 # already holds a store
    with pytest.raises(ValueError):
        P.clean(tmp_path / "nowhere", tmp_path / "x", MIN_AREA)
    with pytest.raises(ValueError):
        P.clean(world.src, tmp_path / "x", -1)
    with pytest.raises(ValueError):
        P.clean(world.src, tmp_path / "x", MIN_AREA, float("nan"))
    bad = P.ProposalStore(tmp_path / "bad")
    r = record(world.masks[3][5], 0)
    bad.write(1, [r, dict(r, segmentation={"size": [65, 33], "counts": "5"})])      # counts that do not sum to H*W
    with pytest.raises(ValueError, match="image 1 entry 1"):
        P.clean(bad, tmp_path / "y", MIN_AREA, device=cuda)
    with pytest.raises(SystemExit):
        P.main(["clean", world.src, world.src, "--min_area", "5"])
