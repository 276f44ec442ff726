"""StoredProposals(mask_nms_thresh=...) on the GPU: a store thinned by mask overlap as it loads (ops.rle_nms -> ops.rle_select ->
the one ops.rle_decode_group) hands out, tensor for tensor, what a reader of the store that proposals.thin wrote hands out -- for
every image alone and the group of all four, under the second metric and the other orders, with a cap (the first `cap` of the
thinned list), at thr = 1.0 (the store itself); the driver's --mask_nms_thresh gives the metrics of a run from the thinned
directory; the flag's refusals; a record that does not decode.  The store is the one of tests/test_gpu_proposals_thin.py: the tiny
SAM without a box NMS at its median threshold, three images of 96 x 128, 150 x 200 and 70 x 37 plus one without a proposal."""
import collections
import json
import os
import shutil

import numpy as np
import pytest
import torch

from test_gpu_proposals_thin import EMPTY, IDS, SHAPES, world      # noqa: F401  (the fixture that writes the store)

pytestmark = pytest.mark.gpu


def same(a, b):
    """two generate_group results: masks, boxes, IoU, stability of every image (the stability of an empty mask is NaN on both sides)"""
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        for x, y in zip(pa[:4], pb[:4]):
            assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape)
            if x.is_floating_point():
                x, y = torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)
            assert torch.equal(x, y)
        assert pa[4] is None and pb[4] is None


def groups(w, cuda):
    """([images], [ids]) of every image alone and of all four, the one without a proposal in the middle"""
    from hybridgl_amd.synth import synth_image
    blank = torch.from_numpy(synth_image(64, 48, 1)).to(cuda)
    images = dict(w.images)
    images[EMPTY] = blank
    out = [([images[i]], [i]) for i in IDS + [EMPTY]]
    order = [IDS[0], IDS[1], EMPTY, IDS[2]]
    return out + [([images[i] for i in order], order)]


@pytest.mark.parametrize("thr,metric,score", [(0.5, "iou", "predicted_iou"), (0.5, "containment", "area"), (0.3, "iou", "stored"),
                                              (0.6, "containment", "stability_score")])
def test_thinned_on_load_equals_the_thinned_store(world, cuda, tmp_path, monkeypatch, thr, metric, score):
    from hybridgl_amd import proposals as P
    w = world
    dst = w.dst
    if (thr, metric, score) != (0.5, "iou", "predicted_iou"):
        dst = str(tmp_path / "thin")
        P.thin(w.src, dst, thr, metric=metric, score=score)
    total = 0
    for cap in (None, 3):
        live = P.StoredProposals(w.src, cuda, cap=cap, mask_nms_thresh=thr, mask_nms_metric=metric, mask_nms_score=score)
        disk = P.StoredProposals(dst, cuda, cap=cap)
        for images, ids in groups(w, cuda):
            a, b = live.generate_group(images, ids), disk.generate_group(images, ids)
            same(a, b)
            total += sum(int(p[0].shape[0]) for p in a)
            if cap:
                assert all(p[0].shape[0] <= 3 for p in a)
        if cap is None:      # the survivors of the walk, each image once, whatever groups it came by in
            kept = {i: len(P.ProposalStore(dst).records(i)) for i in IDS + [EMPTY]}
            assert live.thinned == [sum(len(w.records[i]) for i in IDS), sum(kept.values())]
            assert 0 < live.thinned[1] < live.thinned[0]
            # a cap of the call, on top: the first two of the thinned list
            same(live.generate_group(*groups(w, cuda)[-1], cap=2), disk.generate_group(*groups(w, cuda)[-1], cap=2))
    assert total > 3 * len(IDS)
    if (thr, metric, score) == (0.5, "iou", "predicted_iou"):
        # the class's contract, counted: one NMS, one compaction and one grouped decode per group that holds an entry
        from hybridgl_amd import ops
        calls = collections.Counter()

        def counted(name, fn):
            def call(*a, **kw):
                calls[name] += 1
                return fn(*a, **kw)
            return call

        for name in ("rle_nms", "rle_select", "rle_decode_group"):
            monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
        four, none = groups(w, cuda)[-1], groups(w, cuda)[len(IDS)]
        assert none[1] == [EMPTY]
        for reader, group, want in ((live, four, (1, 1, 1)), (disk, four, (0, 0, 1)), (live, none, (0, 0, 0)), (disk, none, (0, 0, 0))):
            calls.clear()
            reader.generate_group(*group)
            assert (calls["rle_nms"], calls["rle_select"], calls["rle_decode_group"]) == want


def test_threshold_one_is_the_store_itself_and_none_is_todays_path(world, cuda):
    from hybridgl_amd import proposals as P
    w = world
    plain = P.StoredProposals(w.src, cuda)
    live = P.StoredProposals(w.src, cuda, mask_nms_thresh=1.0)
    for images, ids in groups(w, cuda):
        same(live.generate_group(images, ids), plain.generate_group(images, ids))
    assert live.thinned[0] == live.thinned[1] == sum(len(w.records[i]) for i in IDS)
    assert plain.mask_nms_thresh is None and plain.thinned == [0, 0]
    for bad in (dict(mask_nms_thresh=float("nan")), dict(mask_nms_thresh=0.5, mask_nms_metric="dice"),
                dict(mask_nms_thresh=0.5, mask_nms_score="bbox")):
        with pytest.raises(ValueError):
            P.StoredProposals(w.src, cuda, **bad)


def test_a_record_that_does_not_decode(world, cuda, tmp_path):
    """the store's own errors, by the entry's index in the stored list: a run list one pixel short, whether the walk keeps the
    entry or drops it, and a bbox that is not its mask's"""
    from hybridgl_amd import proposals as P
    from hybridgl_amd import sam as hsam
    w = world
    iid = IDS[0]
    store = str(tmp_path / "copy")
    shutil.copytree(w.src, store)
    path = os.path.join(store, f"{iid}.json")
    good = json.load(open(path))
    kept_idx = [k for k, r in enumerate(good) if r in P.ProposalStore(w.dst).records(iid)]
    dropped = [k for k in range(len(good)) if k not in kept_idx]
    assert kept_idx and dropped

    def load_with(recs):
        json.dump(recs, open(path, "w"))
        return P.StoredProposals(store, cuda, mask_nms_thresh=0.5).generate_group([w.images[iid]], [iid])

    same(load_with(good), P.StoredProposals(w.dst, cuda).generate_group([w.images[iid]], [iid]))
    H, W = good[0]["segmentation"]["size"]
    for k in (kept_idx[-1], dropped[0]):
        counts = hsam.rle_counts_from_string(good[k]["segmentation"]["counts"]).tolist()
        j = max(i for i, c in enumerate(counts) if c > 0)
        counts[j] -= 1      # the counts stop one pixel short of H*W
        bad = json.loads(json.dumps(good))
        bad[k]["segmentation"]["counts"] = hsam.coco_encode_rle({"size": [H, W], "counts": counts})["counts"]
        with pytest.raises(ValueError, match=f"image {iid} entry {k}: its counts do not decode"):
            load_with(bad)
    k = next(j for j in kept_idx if good[j]["area"] > 0)
    bad = json.loads(json.dumps(good))
    bad[k]["bbox"][2] += 1
    with pytest.raises(ValueError, match=f"image {iid} entry {k}: the stored bbox"):
        load_with(bad)


def test_the_flag_is_refused_without_a_store_and_with_the_ceiling():
    from hybridgl_amd import main as drv
    parse = drv.default_argument_parser().parse_args
    for flags in (["--real", "--mask_nms_thresh", "0.5"], ["--mask_nms_thresh", "0.5", "--synthetic", "2"],
                  ["--real", "--mask_nms_thresh", "0.5", "--save_proposals", "d"]):
        with pytest.raises(SystemExit, match="--mask_nms_thresh"):
            drv.check_proposal_flags(parse(flags))
        with pytest.raises(SystemExit, match="--mask_nms_thresh"):
            drv.main(parse(flags))
    with pytest.raises(SystemExit, match="--proposal_ceiling"):
        drv.check_proposal_flags(parse(["--real", "--proposals_dir", "d", "--mask_nms_thresh", "0.5", "--proposal_ceiling", "c.json"]))
    with pytest.raises(SystemExit, match="NaN"):
        drv.check_proposal_flags(parse(["--real", "--proposals_dir", "d", "--mask_nms_thresh", "nan"]))
    drv.check_proposal_flags(parse(["--real", "--proposals_dir", "d", "--mask_nms_thresh", "0.5", "--mask_nms_metric", "containment",
                                    "--mask_nms_score", "stored"]))
    with pytest.raises(SystemExit):
        parse(["--mask_nms_metric", "dice"])


def test_one_evaluation_through_the_driver(world, cuda, golden_dir, tmp_path, monkeypatch, capsys):
    """--proposals_dir SRC --mask_nms_thresh 0.5 against --proposals_dir THIN(SRC, 0.5): the same metrics and report, the banner
    and the totals of --stats_json; the store is written by a run of the same data set with the thin test's generator"""
    from hybridgl_amd import backbone
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    from hybridgl_amd.gem import create_gem_model
    from hybridgl_amd.sam import SamAutomaticMaskGenerator, sam_model_registry
    from test_gpu_proposal_store import _dataset, _flags
    root = tmp_path / "refer_data"
    root.mkdir()
    refs = _dataset(root, n_images=4)
    model = backbone.CLIPViTFM("ViT-B/16", seed=0, device=cuda)
    gem = create_gem_model("ViT-B/16", clip=model)
    sam = sam_model_registry["tiny"](device=cuda)
    sam.mask_threshold = P.ProposalStore(world.src).meta()["mask_threshold"]      # the median of the noise logits: overlapping masks
    sgen = SamAutomaticMaskGenerator(sam, points_per_side=6, pred_iou_thresh=-1.0, stability_score_thresh=-1.0, box_nms_thresh=1.0,
                                     min_mask_region_area=0)
    src, dst = str(tmp_path / "props"), str(tmp_path / "thin")
    base = _flags(root, golden_dir, "--group", "4", "--workers", "2", "--result_dir", str(tmp_path / "log"), "--fusion_mode", "G2L")
    parse = drv.default_argument_parser().parse_args
    save = parse(base + ["--save_proposals", src])
    drv.resolve_defaults(save)
    save.precision = "f16x3"
    drv.evaluate(save, model, sgen, gem, cuda)
    rep = P.thin(src, dst, 0.5)
    assert 0 < rep["after"] < rep["before"]

    class Built:      # build_models constructs the CLIP model from the flags: hand it the one this test holds
        def __init__(self, **kw):
            pass

        def eval(self):
            return model

    monkeypatch.setattr(backbone, "CLIPViTFM", Built)
    live = parse(base + ["--proposals_dir", src, "--mask_nms_thresh", "0.5", "--stats_json", str(tmp_path / "stats.json")])
    capsys.readouterr()
    m_live = drv.main(live)      # flags -> build_models -> StoredProposals(mask_nms_thresh=...) -> the loop -> banner and stats
    monkeypatch.undo()
    out = capsys.readouterr().out
    assert f"thinned on load by mask NMS: thr=0.5 metric=iou score=predicted_iou, {rep['before']} -> {rep['after']} proposals" in out
    st_live = json.load(open(tmp_path / "stats.json"))["stats"]
    disk = parse(base + ["--proposals_dir", dst])
    drv.resolve_defaults(disk)
    disk.precision = live.precision
    m_disk, st_disk = drv.evaluate(disk, model, P.StoredProposals(dst, cuda), gem, cuda)
    assert m_live == m_disk and m_live["n_sentences"] >= len(refs)
    assert drv.report_text(live, m_live, live.precision) == drv.report_text(disk, m_disk, disk.precision)
    assert st_live["proposals_thinned"] == {"thr": 0.5, "metric": "iou", "score": "predicted_iou", "before": rep["before"],
                                            "after": rep["after"]}
    assert "proposals_thinned" not in st_disk
    # the unthinned store gives another run: the thinning reached the scoring
    plain = parse(base + ["--proposals_dir", src])
    drv.resolve_defaults(plain)
    plain.precision = live.precision
    sp = P.StoredProposals(src, cuda)
    drv.evaluate(plain, model, sp, gem, cuda)
    assert sp.thinned == [0, 0]
