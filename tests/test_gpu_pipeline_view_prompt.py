"""HybridGLPipeline(view_prompt=...) on the tiny model: None and the "hybridgl" preset are the same pipeline (features and
winners bit for bit, step and run); with "red_circle", and with fusion_mode="crop" + "masked_crop", the hybrid features the
pipeline collects are model(*ops.synthesize_views_prompt(...)) on the same proposals, bit for bit; a box window refuses every
fusion mode but "crop"; the demo's --view_prompt red_circle writes its PNG (the demo is built for 224-pixel views: seeded CLIP
ViT-B/16 and the tiny SAM, as tests/test_gpu_demo.py builds them)."""
import os

import numpy as np
import pytest
import torch

from hybridgl_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(cuda):
    from hybridgl_amd import weights
    from hybridgl_amd.backbone import CLIPViTFM
    return CLIPViTFM("tiny", state_dict=weights.clip_state_dict("tiny", 0), device=cuda)


@pytest.fixture(scope="module")
def refs(cuda):
    from hybridgl_amd.pipeline import synthetic_ref
    return [synthetic_ref(i, cuda, N=n, H=96, W=128, context=16, vocab=512)[0] for i, n in enumerate((12, 7, 9, 12))]


def _pipe(model, **kw):
    from hybridgl_amd.pipeline import HybridGLPipeline
    return HybridGLPipeline(model, masking_block=9, res=64, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_none_and_the_default_preset_are_one_pipeline(model, refs):
    a, b, c = _pipe(model), _pipe(model, view_prompt="hybridgl"), _pipe(model, view_prompt=ops.view_prompt())
    assert a.view_prompt is None and b.view_prompt is None and c.view_prompt is None      # the old op serves all three
    for r in refs:
        ha, hb = a.step(r)[0], b.step(r)[0]
        assert _same_bits(ha, hb)
    assert np.array_equal(a.winning_indices(), b.winning_indices()) and np.array_equal(a.partial_rows(), b.partial_rows())
    a, b = _pipe(model), _pipe(model, view_prompt="hybridgl")
    assert a.run(iter(refs), group=2, collect=True) == len(refs) == b.run(iter(refs), group=2, collect=True)
    for (h1, _, _), (h2, _, _) in zip(a.collected, b.collected):
        assert _same_bits(h1, h2)
    assert np.array_equal(a.winning_indices(), b.winning_indices()) and a.metrics() == b.metrics()


@pytest.mark.parametrize("fusion,name", [("G2L", "red_circle"), ("crop", "masked_crop"), ("crop", "crop,pad_permille=250")])
def test_collected_features_are_the_models_on_the_prompted_views(model, refs, fusion, name):
    prompt = ops.parse_view_prompt(name)

    def views(r, out=None):
        blurred = (r.blurred if r.blurred is not None else ops.gaussian_blur_u8(r.sam_img, 15)) if prompt.global_bg == 0 else None
        return ops.synthesize_views_prompt(r.sam_img, blurred, r.image_norm, r.masks, prompt, boxes=ops.xywh_to_view_boxes(r.boxes), res=64,
                                           out=out)
    # step: one ref, one forward
    p = _pipe(model, fusion_mode=fusion, view_prompt=name)
    assert p.view_prompt is not None
    plain = _pipe(model, fusion_mode=fusion)
    for r in refs[:2]:
        got = p.step(r)[0]
        want = model(*views(r), r.masks, masking_block=9, fusion_mode=fusion)
        assert _same_bits(got, want)
        assert not torch.equal(got, plain.step(r)[0])      # the prompt reaches CLIP
    # the XYWH boxes of the records are the masks' own boxes: the op computes the same ones when given none
    r = refs[0]
    assert torch.equal(ops.synthesize_views_prompt(r.sam_img, None, r.image_norm, r.masks, ops.view_prompt("crop", global_bg="keep"), res=64)[0],
                       ops.synthesize_views_prompt(r.sam_img, None, r.image_norm, r.masks, ops.view_prompt("crop", global_bg="keep"),
                                                   boxes=ops.xywh_to_view_boxes(r.boxes), res=64)[0])
    # run: groups of two refs, one forward per group over both refs' rows (hgl_clip_hybrid_forward_segments)
    p = _pipe(model, fusion_mode=fusion, view_prompt=prompt)
    assert p.run(iter(refs), group=2, collect=True) == len(refs)
    assert len(p.collected) == len(refs)
    for g in range(0, len(refs), 2):
        pair = refs[g:g + 2]
        n = [r.masks.shape[0] for r in pair]
        loc = torch.empty((sum(n), 3, 64, 64), device=model.device)
        glo = torch.empty_like(loc)
        for r, o in zip(pair, (0, n[0])):
            views(r, out=(loc[o:o + r.masks.shape[0]], glo[o:o + r.masks.shape[0]]))
        want = model(loc, glo, [r.masks for r in pair], masking_block=9, fusion_mode=fusion)
        assert _same_bits(p.collected[g][0], want[:n[0]]) and _same_bits(p.collected[g + 1][0], want[n[0]:])


def test_a_box_window_takes_the_crop_mode_only(model):
    for mode in ("G2L", "L2G", "G2L&L2G"):
        for spec in ("masked_crop", "crop", "window=box"):
            with pytest.raises(ValueError, match="fusion_mode='crop'"):
                _pipe(model, fusion_mode=mode, view_prompt=spec)
    _pipe(model, fusion_mode="crop", view_prompt="masked_crop")
    for spec in ("red_circle", "black", "gray", "keep", "marker=box,grow=3"):      # markers and backgrounds go with every mode
        for mode in ("G2L", "L2G", "G2L&L2G", "crop"):
            _pipe(model, fusion_mode=mode, view_prompt=spec)
    with pytest.raises(ValueError, match="thickness"):
        _pipe(model, view_prompt="red_circle,thickness=99")


def test_the_demo_writes_its_png_under_a_red_circle(cuda, golden_dir, tmp_path):
    from PIL import Image
    from hybridgl_amd import demo
    from hybridgl_amd.synth import synth_image
    img = tmp_path / "in.png"
    Image.fromarray(synth_image(120, 163, 50)).save(img)
    out = tmp_path / "out.png"
    rc = demo.main(["--image", str(img), "--text", "the cat on left", "--out", str(out), "--noun_phrase", "the cat", "--dirflag", "left",
                    "--sam_model", "tiny", "--bpe_vocab", os.path.join(golden_dir, "tiny_bpe_vocab.txt.gz"),
                    "--view_prompt", "red_circle", "--points_per_side", "4", "--pred_iou_thresh", "-1", "--stability_score_thresh", "0",
                    "--min_mask_region_area", "20", "--box_nms_thresh", "1"])
    assert rc == 0
    assert np.asarray(Image.open(out)).shape == (120, 163, 3)
