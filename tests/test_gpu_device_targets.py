"""`main.py --device_targets`: the two branches that build no model (--score_masks, --proposal_ceiling) take every target's size
and polygons from the REFER annotations alone and rasterise them on the device, straight into run lengths
(ops.rle_from_polygons through predictions.score / proposals.ceiling).  On a small on-disk REFER tree (the layout of
tests/test_gpu_proposal_store.py: multi-polygon objects, polygons that leave the image, one RLE-dict annotation) with a saved
run and a proposal store written as the run's own writers write them, but from seeded masks -- no model is needed to pin what
the flag changes: with the image files DELETED the flag's rows and metrics equal those obtained before the deletion without
it, and without the flag the branches fail."""
import json
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dataset(root):
    """7 images of different sizes, 1-2 refs each, 1-2 sentences per ref: single polygons, overlapping pairs (the rule "covered
    exactly once" matters), polygons that leave the image, a one-point polygon beside a real one, an RLE-dict annotation"""
    from PIL import Image
    (root / "refcoco").mkdir(parents=True)
    img_dir = root / "images/mscoco/images/train2014"
    img_dir.mkdir(parents=True)
    rng = np.random.default_rng(4)
    images, anns, refs = [], [], []
    rid = 300
    for i in range(7):
        h, w = 48 + 9 * (i % 4), 64 + 11 * (i % 3)
        name = f"COCO_train2014_{i:012d}.png"
        Image.fromarray(rng.integers(0, 255, size=(h, w, 3), dtype=np.uint8)).save(img_dir / name)
        images.append({"id": 20 + i, "file_name": name, "height": h, "width": w})
        for j in range(1 + i % 2):
            aid = 2000 + rid
            x0 = 6.5 + 14 * j
            seg = [[x0, 7.25, x0 + 40, 9, x0 + 33.5, h - 8, x0 + 4, h - 15.75]]
            if i % 3 == 1:
                seg.append([x0 + 20, 20, w + 7.5, 18.5, w + 3, h + 4, x0 + 25, h - 12])      # overlaps the first, leaves the image
            if i % 3 == 2:
                seg += [[-6.0, -4.5, 30.25, 12, 10, h + 5.5], [3.0, 3.0]]
            if i == 6 and j == 0:
                m = np.zeros((h, w), np.uint8)
                m[5:30, 8:41] = 1
                flat, counts, cur, run = m.T.ravel(), [], 0, 0
                for v in flat:
                    if v == cur:
                        run += 1
                    else:
                        counts.append(run)
                        cur, run = v, 1
                counts.append(run)
                seg = {"size": [h, w], "counts": counts}
            anns.append({"id": aid, "image_id": 20 + i, "category_id": 1, "segmentation": seg, "bbox": [0, 0, 1, 1]})
            sents = [{"sent_id": 2 * rid, "raw": "the cat on left", "tokens": []}]
            if (i + j) % 2:
                sents.append({"sent_id": 2 * rid + 1, "raw": "a big dog", "tokens": []})
            refs.append({"ref_id": rid, "ann_id": aid, "image_id": 20 + i, "category_id": 1, "split": "val",
                         "sent_ids": [s["sent_id"] for s in sents], "sentences": sents})
            rid += 1
    refs = refs[::2] + refs[1::2]      # images come back after other images
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "thing"}]}, open(root / "refcoco/instances.json", "w"))
    pickle.dump(refs, open(root / "refcoco/refs(unc).p", "wb"))
    json.dump({}, open(root / "parse.json", "w"))
    return refs


def _flags(root, golden_dir, *more):
    return ["--real", "--refer_data_root", str(root), "--dataset", "refcoco", "--split", "val", "--bpe_vocab",
            os.path.join(golden_dir, "tiny_bpe_vocab.txt.gz"), "--parse_json", str(root / "parse.json"), "--heatmap", "given",
            "--workers", "1", "--result_dir", str(root / "log")] + list(more)


class World:
    pass


@pytest.fixture(scope="module")
def world(cuda, golden_dir, tmp_path_factory):
    """the tree, a saved run and a proposal store over it, the two branches' results WITHOUT the flag -- and then no image file"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    from hybridgl_amd import refer_io
    from hybridgl_amd import sam as hsam
    w = World()
    w.root = tmp_path_factory.mktemp("refer_data")
    w.refs = _dataset(w.root)
    ds = refer_io.ReferDataset(str(w.root), "refcoco", "unc", "val")
    rng = np.random.default_rng(9)
    string = lambda m: hsam.coco_encode_rle(hsam.mask_to_rle(m.astype(bool)))["counts"]
    # the saved run: per sentence two masks near the target, with the counts a run would have stored
    w.out = w.root / "out"
    w.out.mkdir()
    lines = []
    for i in range(len(ds)):
        gt = ds.target(i).astype(bool)
        H, W = gt.shape
        for j in range(len(ds.sentence_raws[i])):
            pure = np.roll(gt, int(rng.integers(-5, 6)), axis=1)
            final = gt & (rng.random((H, W)) < 0.9)
            lines.append({"index": i, "sentence": j, "size": [H, W], "pure": string(pure), "final": string(final),
                          "I": int((pure & gt).sum()), "U": int((pure | gt).sum()), "I_final": int((final & gt).sum()),
                          "U_final": int((final | gt).sum())})
    with open(w.out / "masks.rank0.jsonl", "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
    w.lines = lines
    w.tampered = w.root / "tampered"
    w.tampered.mkdir()
    changed = [dict(r) for r in lines]
    changed[3]["final"] = changed[3]["pure"]
    assert lines[3]["final"] != lines[3]["pure"]
    with open(w.tampered / "masks.rank0.jsonl", "w") as f:
        for r in changed:
            f.write(json.dumps(r) + "\n")
    # the store: three box proposals per image, as ProposalRecorder writes them
    w.store = w.root / "store"
    store = P.ProposalStore(w.store)
    for img in ds.refer.data["images"]:
        H, W = img["height"], img["width"]
        masks = np.zeros((3, H, W), bool)
        masks[0, 5:H - 10, 8:50] = True
        masks[1, 10:H - 5, 20:W - 4] = True
        masks[2, 0:20, 0:30] = True
        counts = [hsam.mask_to_rle(m)["counts"] for m in masks]
        store.write(img["id"], P.build_records(H, W, counts, [int(m.sum()) for m in masks], np.zeros((3, 4), np.int64), np.ones(3),
                                               np.ones(3), np.zeros((3, 2)), np.asarray([[0, 0, W, H]] * 3)))
    store.write_meta({})
    parse = drv.default_argument_parser().parse_args
    w.score_args = lambda d, *more: parse(_flags(w.root, golden_dir, "--score_masks", str(d), *more))
    w.ceiling_args = lambda *more: parse(_flags(w.root, golden_dir, "--proposals_dir", str(w.store), "--proposal_ceiling",
                                                str(w.root / "ceiling.json"), *more))
    w.golden_dir = golden_dir
    w.score = drv.score_masks(w.score_args(w.out), cuda)
    w.ceiling = drv.proposal_ceiling(w.ceiling_args(), cuda)
    assert w.score[1]["mismatches"] == [] and len(w.score[1]["rows"]) == len(lines) and len(w.ceiling[1]) == len(lines)
    assert (w.ceiling[1][:, 3] > 0).all()
    img_dir = w.root / "images/mscoco/images/train2014"
    for name in os.listdir(img_dir):
        os.remove(img_dir / name)
    assert os.listdir(img_dir) == []
    return w


def test_score_masks_from_the_annotations_alone(cuda, world):
    from hybridgl_amd import main as drv
    m, rep = drv.score_masks(world.score_args(world.out, "--device_targets"), cuda)
    m0, rep0 = world.score
    assert m == m0 and np.array_equal(rep["rows"], rep0["rows"]) and rep["rows"].dtype == np.int64
    assert rep["mismatches"] == [] and rep["missing"] == [] and rep["extra"] == []
    want = sorted([r["index"], r["sentence"], r["I"], r["U"], r["I_final"], r["U_final"]] for r in world.lines)
    assert rep["rows"].tolist() == want


def test_proposal_ceiling_from_the_annotations_alone(cuda, world):
    from hybridgl_amd import main as drv
    c, rows = drv.proposal_ceiling(world.ceiling_args("--device_targets", "--group", "3"), cuda)
    c0, rows0 = world.ceiling
    assert c == c0 and np.array_equal(rows, rows0)


def test_without_the_flag_the_branches_need_the_image_files(cuda, world):
    """what cannot pass before the flag existed: no image file is left"""
    from hybridgl_amd import main as drv
    with pytest.raises(FileNotFoundError):
        drv.score_masks(world.score_args(world.out), cuda)
    with pytest.raises(FileNotFoundError):
        drv.proposal_ceiling(world.ceiling_args(), cuda)


def test_a_tampered_record_is_still_reported(cuda, world):
    from hybridgl_amd import main as drv
    m, rep = drv.score_masks(world.score_args(world.tampered, "--device_targets"), cuda)
    assert rep["mismatches"] == [(world.lines[3]["index"], world.lines[3]["sentence"])] and rep["missing"] == [] and rep["extra"] == []
    with pytest.raises(SystemExit) as e:
        drv.score_masks_main(world.score_args(world.tampered, "--device_targets"), cuda)
    assert e.value.code == 1


def test_the_flag_where_it_does_not_apply(cuda, world):
    from hybridgl_amd import main as drv
    parse = drv.default_argument_parser().parse_args
    cases = [(["--synthetic", "2", "--score_masks", str(world.out), "--device_targets"], "needs --real REFER data"),
             (_flags(world.root, world.golden_dir, "--score_masks", str(world.out), "--device_targets")[:3] +
              ["--dataset", "phrasecut", "--score_masks", str(world.out), "--device_targets"], "needs --real REFER data"),
             (["--synthetic", "2", "--proposals_dir", str(world.store), "--proposal_ceiling", str(world.root / "c.json"),
               "--device_targets"], "needs --real REFER data"),
             (_flags(world.root, world.golden_dir, "--device_targets"), "applies to --score_masks and --proposal_ceiling only")]
    for argv, message in cases:
        with pytest.raises(SystemExit) as e:
            drv.main(parse(argv))
        assert message in str(e.value), (argv, str(e.value))


def test_a_polygon_the_host_codec_refuses_raises(cuda):
    from hybridgl_amd import predictions as P
    from hybridgl_amd.refer_io import PolygonTarget
    rec = {"index": 4, "sentence": 1, "size": [8, 9], "pure": "", "final": "", "I": 0, "U": 0, "I_final": 0, "U_final": 0}
    with pytest.raises(ValueError, match="NaN"):
        P.score([rec], [((4, 1), PolygonTarget(8, 9, [[1.0, float("nan"), 3.0, 3.0]]))])
