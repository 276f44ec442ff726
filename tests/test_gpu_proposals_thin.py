"""proposals.thin on the GPU, on a store written from the tiny SAM through the recorder (as tests/test_gpu_proposal_store.py writes
one): it keeps per image exactly what sam.nms_rles keeps of the stored strings, every mask it keeps is a mask of the source,
thr = 1.0 keeps everything, the ceiling of a thinned store never exceeds the source's, and the command line writes the same store."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IDS = [4, 9, 23]
SHAPES = {4: (96, 128), 9: (150, 200), 23: (70, 37)}
EMPTY = 15


class World:
    pass


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    from hybridgl_amd import proposals as P
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, SamPredictor, sam_model_registry
    from hybridgl_amd.synth import synth_image
    w = World()
    sam = sam_model_registry["tiny"](device=cuda)
    # box_nms_thresh 1.0: no box falls, so the list holds the overlapping masks that a mask NMS is for
    gen = SamAutomaticMaskGenerator(sam, points_per_side=6, pred_iou_thresh=-1.0, stability_score_thresh=-1.0, box_nms_thresh=1.0,
                                    min_mask_region_area=0)
    # random weights give noise logits: at their median a mask covers about half of the image
    pred = SamPredictor(sam)
    pred.set_image(torch.from_numpy(synth_image(96, 128, 70)).to(cuda))
    pts = torch.from_numpy(pred.transform.apply_coords(gen.point_grids[0] * np.array([[128, 96]]), (96, 128)))[:, None, :]
    logits, _, _ = pred.predict_torch(pts, torch.ones((len(pts), 1), dtype=torch.int64), return_logits=True)
    sam.mask_threshold = float(torch.quantile(logits.flatten()[:4_000_000].float(), 0.5))
    w.images = {i: torch.from_numpy(synth_image(*SHAPES[i], 100 + i)).to(cuda) for i in IDS}
    w.src = str(tmp_path_factory.mktemp("src"))
    rec = P.ProposalRecorder(gen, w.src, P.generator_settings(gen, sam_model="tiny"))
    for i in IDS:
        rec.group_finish(rec.group_cleanup(rec.group_begin([w.images[i]], None, None, image_ids=[i])))
    assert rec.flush() == len(IDS)
    store = P.ProposalStore(w.src)
    store.write(EMPTY, [])
    w.records = {i: store.records(i) for i in IDS}
    assert all(len(r) > 8 for r in w.records.values())
    w.dst = str(tmp_path_factory.mktemp("thin") / "half")
    w.report = P.thin(w.src, w.dst, 0.5)
    return w


def test_it_keeps_what_nms_rles_keeps(world, cuda):
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    dst = P.ProposalStore(w.dst)
    assert dst.image_ids() == sorted(IDS + [EMPTY]) and dst.records(EMPTY) == []
    before = after = 0
    for i in IDS:
        recs = w.records[i]
        kept = hsam.nms_rles([r["segmentation"] for r in recs], [r["predicted_iou"] for r in recs], 0.5, device=cuda)
        assert len(set(kept)) == len(kept) > 0
        assert json.dumps(dst.records(i)) == json.dumps([recs[k] for k in sorted(kept)]), i
        assert w.report["per_image"][i] == [len(recs), len(kept)]
        # the first of the walk is always kept: the highest predicted IoU, the lowest index on a tie
        assert kept[0] == min(range(len(recs)), key=lambda k: (-np.float32(recs[k]["predicted_iou"]), k))
        before, after = before + len(recs), after + len(kept)
    assert w.report["before"] == before and w.report["after"] == after and w.report["per_image"][EMPTY] == [0, 0]
    assert dst.meta() == dict(P.ProposalStore(w.src).meta(), thinned={"thr": 0.5, "metric": "iou", "score": "predicted_iou", "source": w.src})
    # the stored order without scores is rleNms's; thr 0 leaves masks that do not meet at all
    zero = P.thin(w.src, os.path.join(os.path.dirname(w.dst), "zero"), 0.0, score="stored")
    assert 0 < zero["after"] < zero["before"] == before
    for i in IDS:
        recs = w.records[i]
        assert zero["per_image"][i][1] == len(hsam.nms_rles([r["segmentation"] for r in recs], None, 0.0, device=cuda))


def test_every_kept_mask_is_a_mask_of_the_source(world, cuda):
    from hybridgl_amd import proposals as P
    rep = P.compare(world.dst, world.src, device=cuda)
    s = rep["summary"]
    assert s["n_a"] == world.report["after"] and s["n_b"] == world.report["before"] and s["identical"] == s["n_a"]
    assert s["only_in_a"] == s["only_in_b"] == s["size_mismatch"] == [] and s["n_images"] == len(IDS) + 1


def test_threshold_one_keeps_everything_and_the_ceiling_never_rises(world, cuda, tmp_path):
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    rep = P.thin(w.src, tmp_path / "all", 1.0, metric="containment", score="area")
    assert rep["after"] == rep["before"]
    for i in IDS + [EMPTY]:
        assert json.dumps(P.ProposalStore(tmp_path / "all").records(i)) == json.dumps(P.ProposalStore(w.src).records(i))
    targets, k = [], 0
    rng = np.random.default_rng(3)
    for i in IDS:
        H, W = SHAPES[i]
        for j in range(4):      # two rectangles and two of the image's own proposals
            if j < 2:
                y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
                m = np.zeros((H, W), np.uint8)
                m[y0:y0 + H // 3 + 1, x0:x0 + W // 3 + 1] = 1
            else:
                seg = w.records[i][(7 * j) % len(w.records[i])]["segmentation"]
                m = hsam.rle_to_mask({"size": seg["size"], "counts": hsam.rle_counts(seg)}).astype(np.uint8)
            targets.append(((k, j), i, torch.from_numpy(m).to(cuda)))
        k += 1
    full = P.ceiling(w.src, targets)
    same = P.ceiling(tmp_path / "all", targets)
    less = P.ceiling(w.dst, targets)
    assert len(full) == len(targets) and np.array_equal(full, same)
    assert np.array_equal(less[:, :2], full[:, :2])
    assert (less[:, 3] * full[:, 4] <= full[:, 3] * less[:, 4]).all()      # I / U, compared exactly


def test_the_command_line_writes_the_same_store(world, tmp_path, capsys):
    from hybridgl_amd import proposals as P
    out = tmp_path / "cli"
    assert P.main(["thin", world.src, str(out), "--thr", "0.5"]) == 0
    assert f"proposals: {world.report['before']} -> {world.report['after']}" in capsys.readouterr().out
    a, b = P.ProposalStore(out), P.ProposalStore(world.dst)
    assert a.image_ids() == b.image_ids() and a.meta() == b.meta()
    for i in a.image_ids():
        assert open(a.path(i)).read() == open(b.path(i)).read()
