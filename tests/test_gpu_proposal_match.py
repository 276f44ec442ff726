"""Two proposal stores compared set against set, and the ceiling of a store without CLIP (hybridgl_amd/proposals.py compare /
ceiling over ops.rle_match), on the tiny REFER set and the store of tests/test_gpu_proposal_store.py: a store against itself; a
copy with one record removed, one duplicated and one mask shifted by a pixel; proposals.ceiling and --proposal_ceiling against
ceiling_rows() / sweep_metrics()["ceiling"] of a sweep run fed from the same store with the same cap."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from test_gpu_proposal_store import _flags, world  # noqa: F401  (the module fixture: models, data set, the recorded store)

pytestmark = pytest.mark.gpu


def test_a_store_against_itself(world):
    from hybridgl_amd import proposals as P
    w = world
    assert P.ProposalStore(w.store).image_ids() == sorted(w.images)
    rep = P.compare(w.store, P.ProposalStore(w.store), group=4)
    s = rep["summary"]
    n = sum(int(m.shape[0]) for m, _ in w.sam_out.values())
    nonempty = sum(int((m.flatten(1).sum(1) > 0).sum()) for m, _ in w.sam_out.values())
    assert s["n_images"] == len(w.images) and s["n_a"] == s["n_b"] == n and s["identical"] == nonempty > 0
    assert s["only_in_a"] == s["only_in_b"] == s["size_mismatch"] == []
    assert s["at_iou"] == {0.5: [nonempty, nonempty], 0.75: [nonempty, nonempty], 0.9: [nonempty, nonempty]}
    assert sorted(rep["per_image"]) == sorted(w.images)
    for iid, r in rep["per_image"].items():
        k = int(w.sam_out[iid][0].shape[0])
        assert r["n_a"] == r["n_b"] == k and r["identical"] <= k
        if r["identical"] == k > 0:
            assert r["mean_iou_a"] == r["min_iou_a"] == r["mean_iou_b"] == r["min_iou_b"] == 1.0


def _report(ma, mb, thresholds):
    """what compare says of one image, from the dense count of tests/test_gpu_rle_match.py and its tie rule"""
    from test_gpu_rle_match import expect
    _, wa, wb = expect(ma, np.zeros(len(ma), np.int64), mb, np.zeros(len(mb), np.int64))

    def side(x, other):
        has = x[:, 2] >= 0
        partner = np.array([other[j, 1] if j >= 0 else 0 for j in x[:, 2]], dtype=np.int64)
        iou = np.where(has, x[:, 3] / np.maximum(x[:, 1] + partner - x[:, 3], 1), 0.0)
        return iou, int((has & (x[:, 3] == x[:, 1]) & (x[:, 3] == partner)).sum())

    (ia, same), (ib, _) = side(wa, wb), side(wb, wa)
    return {"n_a": len(ma), "n_b": len(mb), "identical": same,
            "at_iou": {t: [int((ia >= t).sum()), int((ib >= t).sum())] for t in thresholds},
            "mean_iou_a": float(ia.sum()) / len(ia) if len(ia) else None, "min_iou_a": float(ia.min()) if len(ia) else None,
            "mean_iou_b": float(ib.sum()) / len(ib) if len(ib) else None, "min_iou_b": float(ib.min()) if len(ib) else None}


def test_a_changed_copy_is_named_exactly(world, tmp_path, capsys):
    """one record removed, one duplicated, one mask shifted by a pixel, one file missing: the report names exactly those"""
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    copy = str(tmp_path / "copy")
    shutil.copytree(w.store, copy)
    masks = {i: m.cpu().numpy().astype(np.uint8) for i, (m, _) in w.sam_out.items()}
    ids = sorted(masks)
    assert len(ids) >= 4 and all(len(masks[i]) for i in ids)
    shifted = next(i for i in ids if masks[i].reshape(len(masks[i]), -1).any(1).any())
    removed, doubled, gone = [i for i in ids if i != shifted][:3]
    k = int(np.flatnonzero(masks[shifted].reshape(len(masks[shifted]), -1).any(1))[0])      # a mask with a pixel to move
    moved = np.zeros_like(masks[shifted][k])
    moved[:, 1:] = masks[shifted][k][:, :-1]                      # one pixel to the right
    assert not np.array_equal(moved, masks[shifted][k])
    theirs = dict(masks)
    theirs[removed] = masks[removed][1:]
    theirs[doubled] = np.concatenate([masks[doubled], masks[doubled][:1]])
    theirs[shifted] = masks[shifted].copy()
    theirs[shifted][k] = moved

    def edit(iid, fn):
        path = os.path.join(copy, f"{iid}.json")
        recs = json.load(open(path))
        json.dump(fn(recs), open(path, "w"))

    def shift(recs):
        recs[k]["segmentation"] = hsam.coco_encode_rle(hsam.mask_to_rle(moved))
        return recs

    edit(removed, lambda r: r[1:])
    edit(doubled, lambda r: r + [r[0]])
    edit(shifted, shift)
    os.remove(os.path.join(copy, f"{gone}.json"))
    thresholds = (0.5, 1.0)
    rep = P.compare(w.store, copy, thresholds=thresholds)
    s, per = rep["summary"], rep["per_image"]
    assert s["only_in_a"] == [gone] and s["only_in_b"] == [] and s["size_mismatch"] == [] and s["n_images"] == len(ids) - 1
    assert sorted(per) == [i for i in ids if i != gone]
    for iid in per:
        assert per[iid] == _report(masks[iid], theirs[iid], thresholds), iid
    same = P.compare(w.store, w.store, thresholds=thresholds)["per_image"]
    assert sorted(i for i in per if per[i] != same[i]) == sorted([removed, doubled, shifted])
    assert per[removed]["n_b"] == per[removed]["n_a"] - 1 and per[doubled]["n_b"] == per[doubled]["n_a"] + 1
    assert per[shifted]["n_b"] == per[shifted]["n_a"] and per[shifted]["min_iou_b"] < 1.0
    assert s["n_a"] == sum(len(masks[i]) for i in per) and s["n_b"] == sum(len(theirs[i]) for i in per)
    assert s["identical"] == sum(per[i]["identical"] for i in per)
    assert s["min_iou_a"] == min(per[i]["min_iou_a"] for i in per)
    # the command line prints the same report and writes it
    out = tmp_path / "report.json"
    assert P.main(["compare", w.store, copy, "--iou", "0.5,1.0", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert f"image {removed}: A {len(masks[removed])}, B {len(masks[removed]) - 1}" in text and f"image {doubled}:" in text
    assert f"image {shifted}:" in text and f"only in a: image {gone}" in text
    saved = json.load(open(out))
    assert saved["summary"]["identical"] == s["identical"] and len(saved["per_image"]) == len(per)
    # a size that differs is listed, not compared
    edit(shifted, lambda recs: [dict(r, segmentation={"size": [r["segmentation"]["size"][0] + 1, r["segmentation"]["size"][1]],
                                                       "counts": r["segmentation"]["counts"]}) for r in recs])
    assert P.compare(w.store, copy)["summary"]["size_mismatch"] == [shifted]


@pytest.mark.parametrize("cap", [None, 2])
def test_ceiling_equals_the_sweep_runs(world, cuda, golden_dir, tmp_path, cap):
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    from hybridgl_amd.pipeline import HybridGLPipeline
    w = world
    sp = P.StoredProposals(w.store, cuda, cap=cap)
    pipe = HybridGLPipeline(w.model, fusion_mode="G2L", masking_block=9, mask_generator=sp, use_sam_masks=True, gem_model=w.gem,
                            sweep=[(0.5, 0.6, 3, 6)])
    assert pipe.run(w.loader(), group=8) == len(w.refs)
    torch.cuda.synchronize()
    want = pipe.ceiling_rows()
    want = want[np.lexsort((want[:, 1], want[:, 0]))]

    def targets():
        for i in w.rr.jobs():
            ref = w.rr.load(i)
            for j, sent in enumerate(ref.sentences):
                yield (ref.index if ref.index is not None else i, j), ref.image_id, (sent.target if sent.target is not None else ref.target)

    got = P.ceiling(w.store, targets(), cap=cap, group=4)
    assert got.shape == want.shape and got.dtype == np.int64 and len(got) > len(w.refs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (got[:, 4] >= got[:, 3]).all() and (cap is not None or (got[:, 3] > 0).any())
    # the driver flag: the same figures, no model built
    from hybridgl_amd import sam as hsam
    from hybridgl_amd import backbone

    def no_model(*a, **k):
        raise AssertionError("a model was constructed")

    out = tmp_path / "ceiling.json"
    args = drv.default_argument_parser().parse_args(_flags(w.root, golden_dir, "--proposals_dir", w.store, "--proposal_ceiling", str(out),
                                                           "--group", "4", "--proposal_cap", str(cap or 0)))
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(hsam.Sam, "__init__", no_model)
        mp.setattr(backbone.CLIPViTFM, "__init__", no_model)
        c = drv.proposal_ceiling_main(args, cuda)
    finally:
        mp.undo()
    assert json.load(open(out)) == json.loads(json.dumps(c)) == json.loads(json.dumps(pipe.sweep_metrics()["ceiling"]))
    assert set(c) == {"oIoU", "mIoU", "cum", "n_sentences"} and c["n_sentences"] == len(want)
