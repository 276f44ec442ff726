"""hybridgl_amd.demo on the GPU: the one-call surface against the evaluator it mirrors.  CLIP ViT-B/16 with seeded weights, the
tiny SAM and the GEM model that shares CLIP's weights, the generator's filters open -- as tests/test_gpu_driver.py builds them.
The RefBatch of HybridGL.segment equals, tensor for tensor, the one RealRefs.load builds for the same image and sentences of a
synthetic REFER tree (the ground truth aside); its indices are winning_indices() of a hand-driven pipeline.step; rle_final
decodes to the winning proposal; .overlay() is the numpy contract (tests/paint_cases.py) on that mask; a second call on the same
image runs no proposal stage; the CLI writes the PNG that Pillow reads back equal to .overlay(), and exits with 2 when the
filters keep nothing."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import paint_cases as PC

pytestmark = pytest.mark.gpu

SENTENCES = ["the cat on left", "a big dog"]
PARSE = [{"noun_phrase": "the cat", "other_nouns": ["left"], "dirflag": "left", "relaflag": "none"},
         {"noun_phrase": "dog", "other_nouns": [], "dirflag": "none", "relaflag": "big"}]
# the filters open and the box NMS off (nothing has IoU > 1): the tiny SAM's noise masks all have image-sized boxes
AMG = dict(points_per_side=4, pred_iou_thresh=-1.0, stability_score_thresh=0.0, min_mask_region_area=20, box_nms_thresh=1.0)
AMG_FLAGS = ["--points_per_side", "4", "--pred_iou_thresh", "-1", "--stability_score_thresh", "0", "--min_mask_region_area", "20",
             "--box_nms_thresh", "1"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """one image, one ref with two sentences, in the reference's directory layout"""
    from PIL import Image
    from hybridgl_amd.synth import synth_image
    root = tmp_path_factory.mktemp("demo_refer")
    (root / "refcoco").mkdir(parents=True)
    img_dir = root / "images/mscoco/images/train2014"
    img_dir.mkdir(parents=True)
    name = f"COCO_train2014_{0:012d}.png"
    Image.fromarray(synth_image(120, 163, 50)).save(img_dir / name)
    json.dump({"images": [{"id": 10, "file_name": name, "height": 120, "width": 163}],
               "annotations": [{"id": 100, "image_id": 10, "category_id": 1, "segmentation": [[10, 12, 90, 15, 80, 100, 15, 90]],
                                "bbox": [0, 0, 1, 1]}], "categories": [{"id": 1, "name": "thing"}]}, open(root / "refcoco/instances.json", "w"))
    refs = [{"ref_id": 200, "ann_id": 100, "image_id": 10, "category_id": 1, "split": "val", "sent_ids": [400, 401],
             "sentences": [{"sent_id": 400 + k, "raw": s, "tokens": []} for k, s in enumerate(SENTENCES)]}]
    pickle.dump(refs, open(root / "refcoco/refs(unc).p", "wb"))
    json.dump({"400": PARSE[0], "401": PARSE[1]}, open(root / "parse.json", "w"))
    return root, str(img_dir / name)


@pytest.fixture(scope="module")
def vocab(golden_dir):
    return os.path.join(golden_dir, "tiny_bpe_vocab.txt.gz")


@pytest.fixture(scope="module")
def hgl(cuda, vocab):
    from hybridgl_amd.demo import HybridGL
    return HybridGL(sam_model="tiny", bpe_vocab=vocab, amg=AMG, device=cuda)


@pytest.fixture(scope="module")
def segs(hgl, tree):
    return hgl.segment(tree[1], SENTENCES, PARSE)


def test_the_ref_batch_is_the_loaders(cuda, hgl, tree, vocab):
    from hybridgl_amd import main as drv
    from hybridgl_amd.weights import CLIP_CONFIGS
    root, path = tree
    args = drv.default_argument_parser().parse_args(["--real", "--refer_data_root", str(root), "--dataset", "refcoco", "--split", "val",
                                                     "--bpe_vocab", vocab, "--parse_json", str(root / "parse.json")])
    rr = drv.RealRefs(args, cuda, "unc", CLIP_CONFIGS["ViT-B/16"]["context_length"])
    want = rr.load(0)
    got = hgl.ref_batch(path, SENTENCES, PARSE)
    for name in ("sam_img", "image_norm", "tensor_img", "tokens", "masks", "boxes"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert got.token_len == want.token_len and got.blurred is None and got.sam_resized is None
    assert got.target.shape == want.target.shape and not got.target.any()      # the ground truth aside
    assert len(got.sentences) == len(want.sentences) == 2
    for a, b in zip(got.sentences, want.sentences):
        assert (a.sentence_row, a.noun_phrase_row, a.other_noun_rows, a.dirflag, a.relaflag, a.n_nouns, a.gem_row) == \
               (b.sentence_row, b.noun_phrase_row, b.other_noun_rows, b.dirflag, b.relaflag, b.n_nouns, b.gem_row)
        assert a.imgattn is None and b.imgattn is None
    # the defaults of a missing record are the loader's too: the noun phrase is the sentence, no other nouns, flags "none"
    bare = hgl.ref_batch(path, SENTENCES[0])
    s = bare.sentences[0]
    assert (s.sentence_row, s.noun_phrase_row, s.other_noun_rows, s.dirflag, s.relaflag, s.n_nouns, s.gem_row) == (0, 1, [], "none", "none", 0, 2)
    assert torch.equal(bare.tokens[0], bare.tokens[1])
    with pytest.raises(ValueError):
        hgl.ref_batch(path, SENTENCES, PARSE[:1])
    with pytest.raises(ValueError):
        hgl.ref_batch(path, SENTENCES[0], {"nouns": []})


def test_the_indices_are_a_hand_driven_steps(cuda, hgl, segs, tree):
    from hybridgl_amd.pipeline import HybridGLPipeline
    pipe = HybridGLPipeline(hgl.model, mask_generator=hgl.generator, use_sam_masks=True, gem_model=hgl.gem_model, k_clamp="per_ref")
    pipe.step(hgl.ref_batch(tree[1], SENTENCES, PARSE))
    win = pipe.winning_indices()
    assert win.shape == (2, 2)
    assert [(s.index_pure, s.index_final) for s in segs] == [tuple(int(v) for v in w) for w in win]
    assert all(s.n_proposals == pipe.last_proposals[0].shape[0] >= 2 and s.text == t for s, t in zip(segs, SENTENCES))


def test_the_strings_decode_to_the_winners_and_the_overlay_is_the_contract(cuda, segs, tree):
    from PIL import Image
    from hybridgl_amd import refer_io, render
    image = np.array(Image.open(tree[1]).convert("RGB"))
    H, W = image.shape[:2]
    for s in segs:
        for which, rle, index in (("pure", s.rle_pure, s.index_pure), ("final", s.rle_final, s.index_final)):
            assert rle["size"] == [H, W] and isinstance(rle["counts"], str)
            m, area = refer_io.gt_mask_from_rle(rle)
            mask = s.mask(which).cpu().numpy()
            assert mask.dtype == bool and np.array_equal(m.astype(bool), mask) and area == mask.sum() > 0
            assert torch.equal(s.mask(which), s.proposals[index])
            # the numpy contract on that mask, in the demo's style
            c = PC.counts_of(mask)
            slots = np.asarray([c], np.uint32)
            out = np.zeros((H * W, 3), np.uint8)
            status = np.zeros((1, 4), np.int32)
            PC.paint(slots, np.array([[len(c), 0, 0, 0]], np.int32), [[H, W, 0, 0, 0]], np.zeros(1, np.int32),
                     PC.style_row(**render.DEMO_STYLE)[None], image.reshape(-1, 3), out, None, status)
            got = s.overlay(which=which)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), out.reshape(H, W, 3))
            blue = image.copy()
            blue[mask, 2] = np.clip(np.rint(image[mask, 2].astype(np.float32) + np.float32(178.5)), 0, 255)
            assert np.array_equal(got.cpu().numpy(), blue)
    red = segs[0].overlay(style=dict(fill=(255, 0, 0), a=0.5, b=0.5, outline=(255, 255, 255)))
    assert not torch.equal(red, segs[0].overlay())
    with pytest.raises(ValueError):
        segs[0].overlay(which="best")


def test_a_second_call_on_the_same_image_runs_no_proposal_stage(cuda, hgl, segs, tree):
    again = hgl.segment(tree[1], SENTENCES, PARSE)      # the same path: the same image
    first = hgl._pipe.last_proposals
    hits = (hgl._pipe.last_image()[0], hgl._image[1])
    other = hgl.segment(tree[1], "a big dog", PARSE[1])
    assert hgl._pipe.last_proposals is first and (hgl._pipe.last_image()[0], hgl._image[1]) == hits
    assert other[0].proposals.data_ptr() == again[0].proposals.data_ptr()
    assert [(s.index_pure, s.index_final, s.rle_final) for s in again] == [(s.index_pure, s.index_final, s.rle_final) for s in segs]
    assert (other[0].index_pure, other[0].index_final, other[0].rle_pure) == (segs[1].index_pure, segs[1].index_final, segs[1].rle_pure)
    # another object is another image: the proposal stage runs again
    from PIL import Image
    arr = np.array(Image.open(tree[1]).convert("RGB"))
    third = hgl.segment(arr, SENTENCES[1], PARSE[1])
    assert hgl._pipe.last_proposals is not first and hgl._image[1] == hits[1] + 1
    assert (third[0].index_final, third[0].rle_final) == (segs[1].index_final, segs[1].rle_final)
    assert hgl.segment(arr, SENTENCES[1], PARSE[1])[0].proposals.data_ptr() == third[0].proposals.data_ptr()


def test_the_cli_writes_the_overlay_and_all_proposals(cuda, hgl, segs, tree, vocab, tmp_path, capsys):
    from PIL import Image
    from hybridgl_amd import demo, render
    out, out2 = tmp_path / "result.png", tmp_path / "all.png"
    rec = tmp_path / "parse.json"
    json.dump({SENTENCES[0]: PARSE[0], SENTENCES[1]: PARSE[1]}, open(rec, "w"))
    rc = demo.main(["--image", tree[1], "--text", SENTENCES[1], "--out", str(out), "--parse_json", str(rec), "--all_proposals", str(out2),
                    "--sam_model", "tiny", "--bpe_vocab", vocab] + AMG_FLAGS)
    assert rc == 0 and f"proposal {segs[1].index_final} of {segs[1].n_proposals}" in capsys.readouterr().out
    assert np.array_equal(np.array(Image.open(out)), segs[1].overlay().cpu().numpy())
    # every proposal, largest first (ties in stored order), in the palette with outlines: the contract on the decoded proposals
    masks = segs[1].proposals.cpu().numpy()
    N, H, W = masks.shape
    order = sorted(range(N), key=lambda k: (-int(masks[k].sum()), k))
    need = max(len(PC.counts_of(m)) for m in masks)
    slots, table = PC.encode_set(list(masks), need, [0] * N)
    want = np.zeros((H * W, 3), np.uint8)
    PC.paint(slots, table, [[H, W, 0, 0, 0]], np.asarray(order, np.int32), render.proposal_styles(N),
             np.array(Image.open(tree[1]).convert("RGB")).reshape(-1, 3), want, None, np.zeros((N, 4), np.int32))
    assert np.array_equal(np.array(Image.open(out2)), want.reshape(H, W, 3))
    assert np.array_equal(hgl.all_proposals(segs[1]).cpu().numpy(), want.reshape(H, W, 3))


def test_exit_code_2_when_the_filters_keep_nothing(cuda, hgl, tree, vocab, tmp_path, capsys, monkeypatch):
    from hybridgl_amd import demo
    from hybridgl_amd.pipeline import EmptyProposals
    out = tmp_path / "never.png"
    rc = demo.main(["--image", tree[1], "--text", SENTENCES[0], "--out", str(out), "--noun_phrase", "the cat", "--dirflag", "left",
                    "--sam_model", "tiny", "--bpe_vocab", vocab, "--points_per_side", "4", "--pred_iou_thresh", "2"])
    assert rc == 2 and not out.exists() and "no proposal survives" in capsys.readouterr().err
    # the library surface lets the exception through: the same models behind a generator whose filter keeps nothing, on an
    # image object the cache has not seen
    from PIL import Image
    from hybridgl_amd.sam import SamAutomaticMaskGenerator
    monkeypatch.setattr(hgl._pipe, "mask_generator", SamAutomaticMaskGenerator(hgl.generator.model, points_per_side=4, pred_iou_thresh=2.0))
    with pytest.raises(EmptyProposals):
        hgl.segment(np.array(Image.open(tree[1]).convert("RGB")), SENTENCES[0])
