"""Pictures from what is on disk, on the GPU: main.py --save_masks then --render_masks over the synthetic refs -- every PNG is
the numpy contract (tests/paint_cases.py) applied to the record's decoded string over the dataset's image; --render_which both
paints pure then final; a record with a wrong size is refused with its key named; --render_limit stops; and
`python -m hybridgl_amd.proposals render` over a small hand-written store equals the contract with the entries ordered by area,
largest first, ties by stored order."""
import json
import os

import numpy as np
import pytest

import paint_cases as PC

pytestmark = pytest.mark.gpu

FLAGS = ["--synthetic", "3", "--proposals", "6", "--heatmap", "given", "--group", "2", "--workers", "1"]


@pytest.fixture(scope="module")
def saved(cuda, tmp_path_factory):
    from hybridgl_amd import main as drv
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.pipeline import synthetic_ref
    out = tmp_path_factory.mktemp("render") / "saved"
    args = drv.default_argument_parser().parse_args(FLAGS + ["--save_masks", str(out)])
    drv.evaluate(args, CLIPViTFM("ViT-B/16", seed=0, device=cuda), None, None, cuda)
    records = {(r["index"], r["sentence"]): r for r in map(json.loads, open(out / "masks.rank0.jsonl"))}
    images = {i: synthetic_ref(i, cuda, N=6, device_blur=True)[0].sam_img.cpu().numpy() for i in range(3)}
    return out, records, images


def contract(image, strings, styles):
    """the strings' masks painted over image in order, by the numpy contract"""
    from hybridgl_amd import refer_io
    H, W = image.shape[:2]
    masks = [refer_io.gt_mask_from_rle({"size": [H, W], "counts": s})[0].astype(bool) for s in strings]
    slots, table = PC.encode_set(masks, max(len(PC.counts_of(m)) for m in masks), [0] * len(masks))
    out = np.zeros((H * W, 3), np.uint8)
    PC.paint(slots, table, [[H, W, 0, 0, 0]], np.arange(len(masks), dtype=np.int32), np.stack(styles), image.reshape(-1, 3), out, None,
             np.zeros((len(masks), 4), np.int32))
    return out.reshape(H, W, 3)


@pytest.mark.parametrize("which", ["final", "pure", "both"])
def test_render_masks_equals_the_contract(cuda, saved, tmp_path, which):
    from PIL import Image
    from hybridgl_amd import main as drv
    from hybridgl_amd import render
    directory, records, images = saved
    out = tmp_path / "png"
    args = drv.default_argument_parser().parse_args(FLAGS + ["--render_masks", str(directory), "--render_out", str(out), "--render_which", which])
    paths = drv.main(args)
    assert sorted(os.listdir(out)) == sorted(f"{i:06d}_{j}.png" for i, j in records) == sorted(os.path.basename(p) for p in paths)
    blue, red = PC.style_row(**render.DEMO_STYLE), PC.style_row(**render.PURE_STYLE)
    for (i, j), rec in records.items():
        strings, styles = {"final": ([rec["final"]], [blue]), "pure": ([rec["pure"]], [blue]),
                           "both": ([rec["pure"], rec["final"]], [red, blue])}[which]
        assert np.array_equal(np.array(Image.open(out / f"{i:06d}_{j}.png")), contract(images[i], strings, styles)), (i, j)


def test_render_limit_and_a_record_of_the_wrong_size(cuda, saved, tmp_path):
    from hybridgl_amd import main as drv
    directory, records, _ = saved
    out = tmp_path / "few"
    args = drv.default_argument_parser().parse_args(FLAGS + ["--render_masks", str(directory), "--render_out", str(out), "--render_limit", "4"])
    assert len(drv.main(args)) == 4 and len(os.listdir(out)) == 4
    bad = tmp_path / "bad"
    bad.mkdir()
    with open(bad / "masks.rank0.jsonl", "w") as f:
        for key, rec in records.items():
            f.write(json.dumps(dict(rec, size=[640, 639]) if key == (1, 2) else rec) + "\n")
    args = drv.default_argument_parser().parse_args(FLAGS + ["--render_masks", str(bad), "--render_out", str(tmp_path / "none")])
    with pytest.raises(SystemExit) as e:
        drv.main(args)
    assert "index 1 sentence 2" in str(e.value) and "[640, 639]" in str(e.value)
    with pytest.raises(SystemExit):
        drv.main(drv.default_argument_parser().parse_args(FLAGS + ["--render_masks", str(directory)]))      # no --render_out


def test_proposals_render_equals_the_contract(cuda, tmp_path):
    from PIL import Image
    from hybridgl_amd import proposals as P
    from hybridgl_amd import render
    from hybridgl_amd.sam import coco_encode_rle
    from hybridgl_amd.synth import synth_image
    rng = np.random.default_rng(12)
    store, root, out = P.ProposalStore(tmp_path / "store"), tmp_path / "images", tmp_path / "out"
    root.mkdir()
    want = {}
    for iid, (H, W), n in ((7, (40, 50), 5), (11, (33, 65), 0), (12, (65, 70), 4)):
        image = synth_image(H, W, iid)
        Image.fromarray(image).save(root / f"{iid}.png")
        masks = [PC.blob(rng, H, W, kind) for kind in ("box", "disc", "box", "noise", "cross")[:n]]
        if n >= 3:
            masks[2] = masks[0].copy()      # a tie in area: the stored order decides
        recs = [{"segmentation": coco_encode_rle({"size": [H, W], "counts": PC.counts_of(m)}), "area": int(m.sum()), "bbox": [0, 0, 1, 1],
                 "predicted_iou": 0.9, "point_coords": [[0.0, 0.0]], "stability_score": 0.9, "crop_box": [0, 0, W, H]} for m in masks]
        store.write(iid, recs)
        order = sorted(range(n), key=lambda k: (-int(masks[k].sum()), k))
        canvas = np.zeros((H * W, 3), np.uint8)
        if n:
            slots, table = PC.encode_set(masks, max(len(PC.counts_of(m)) for m in masks), [0] * n)
            PC.paint(slots, table, [[H, W, 0, 0, 0]], np.asarray(order, np.int32), render.proposal_styles(n), image.reshape(-1, 3), canvas,
                     None, np.zeros((n, 4), np.int32))
        else:
            canvas[:] = image.reshape(-1, 3)
        want[iid] = canvas.reshape(H, W, 3)
    assert P.main(["render", str(store.directory), str(out), "--images", str(root)]) == 0
    assert sorted(os.listdir(out)) == ["11.png", "12.png", "7.png"]
    for iid, pic in want.items():
        assert np.array_equal(np.array(Image.open(out / f"{iid}.png")), pic), iid
    assert len(P.render(store, tmp_path / "one", str(root), limit=1)) == 1
    os.remove(root / "12.png")
    with pytest.raises(SystemExit) as e:
        P.main(["render", str(store.directory), str(tmp_path / "out2"), "--images", str(root)])
    assert "image 12" in str(e.value)
