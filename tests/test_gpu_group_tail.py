"""The SAM proposal tail of a GROUP of images -- one decoder call, one post-processing call and one NMS launch per size class
(SamAutomaticMaskGenerator._propose_classes / group_cleanup / group_finish) -- against the per-image calls it replaces, bit
for bit, at the ViT-H decoder size."""
import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import sam as hsam
from hybridgl_amd import weights

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _vit_h_d2(cuda):
    """SAM with the full ViT-H width, grid and decoder but two encoder blocks (the decoder is the published size).  Built and
    dropped by every test itself (no fixture keeps it): its registered fp16 splits have to be gone when the test returns."""
    name = "vit_h_d2"
    return hsam.Sam(weights.sam_state_dict(name, 0), weights.SAM_CONFIGS[name], cuda)


def _release():
    import gc
    torch.cuda.synchronize()
    gc.collect()
    ops._ws_cache.clear()       # (the decoder workspace of 1024 prompts)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ppi", [64, 192])
@pytest.mark.parametrize("n_img", [2, 3, 16])
def test_batched_decode_equals_the_single_image_calls(cuda, n_img, ppi):
    """The prompts of n_img images in ONE decoder call give, prompt by prompt, the bits of each image's own call: 64 prompts
    per image is the regime of eight key ranges per prompt in the token -> image attention (the split follows the prompts
    per image, not the launch's 128 .. 1024), 192 the regime of one; plain and with the IoU gate."""
    m = _vit_h_d2(cuda)
    try:
        _batched_decode(cuda, m, n_img, ppi)
    finally:
        del m
        _release()


def _batched_decode(cuda, m, n_img, ppi):
    g = m.grid
    rng = np.random.default_rng(100 * n_img + ppi)
    emb = T(rng.standard_normal((n_img, g * g, 256)).astype(np.float32), cuda)
    p01 = T(rng.random((n_img * ppi, 2)).astype(np.float32), cuda)
    low, iou = m.decode_points_multi(emb, p01, n_img)
    assert torch.isfinite(low).all() and torch.isfinite(iou).all()
    thr = float(torch.quantile(iou.max(dim=1).values, 0.5))      # the gate skips about half of the prompts
    lowg, ioug = m.decode_points_multi(emb, p01, n_img, iou_gate=thr)
    assert torch.equal(iou, ioug)
    for i in range(n_img):
        sl = slice(i * ppi, (i + 1) * ppi)
        l1, i1 = m.decode_points(emb[i], p01[sl].contiguous())
        assert torch.equal(i1, iou[sl]), (i, "iou")
        assert torch.equal(l1, low[sl]), (i, "low_res")
        l2, i2 = m.decode_points(emb[i], p01[sl].contiguous(), iou_gate=thr)
        assert torch.equal(i2, iou[sl]), (i, "gated iou")
        live = (i2 > thr).any(dim=1)                              # (the skipped prompts' rows are unwritten memory)
        assert torch.equal(l2[live], lowg[sl][live]) and torch.equal(l2[live], l1[live]), (i, "gated low_res")


def _nms_case(rng, K, nan=False):
    xy = rng.integers(0, 600, size=(K, 2))
    wh = rng.integers(1, 200, size=(K, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.int32)
    scores = rng.random(K).astype(np.float32)
    keep = (rng.random(K) > 0.2).astype(np.uint8)
    if K:
        boxes[K // 2] = boxes[0]                     # duplicates
        keep[0] = keep[K - 1] = 1
    if K > 3:
        scores[3] = scores[1]                        # score tie -> lower index first
    if nan and K:
        scores[rng.choice(K, size=min(K // 2, 7), replace=False)] = np.nan
        scores[0] = np.nan
    return boxes, scores, keep


@pytest.mark.parametrize("nan", [False, True])
def test_segmented_nms_equals_nms_per_segment(cuda, nan):
    """hgl_nms_segments on the candidate lists of test_nms_vs_oracle / test_nms_with_nan_scores side by side -- an empty
    list, lists for the bit-matrix kernel (<= 512) and for the serial one (513 .. 1024) in one call -- against hgl_nms on
    every list alone and against the oracle."""
    from oracle import sam_oracle as S
    rng = np.random.default_rng(12 if nan else 2)
    for lens in ([1, 7, 64, 192, 0, 512, 513, 700, 5], [192] * 16, [64, 0, 0, 33], [0], [1024, 3]):
        cases = [_nms_case(rng, K, nan) for K in lens]
        boxes = np.concatenate([c[0] for c in cases]).reshape(-1, 4)
        scores = np.concatenate([c[1] for c in cases])
        keep = np.concatenate([c[2] for c in cases])
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        if boxes.shape[0] == 0:      # (a call needs memory to point at)
            boxes, scores, keep = np.zeros((1, 4), np.int32), np.zeros(1, np.float32), np.zeros(1, np.uint8)
        idx, n = hsam.nms_segments(T(boxes, cuda), T(scores, cuda), T(keep, cuda), T(offs, cuda), max(lens), 0.7)
        idx, n = idx.cpu().numpy(), n.cpu().numpy()
        assert n.shape == (len(lens),)
        for s, (K, (b, sc, kp)) in enumerate(zip(lens, cases)):
            got = idx[offs[s]:offs[s] + n[s]].tolist()
            if K == 0:
                assert n[s] == 0
                continue
            i1, n1 = hsam.nms(T(b, cuda), T(sc, cuda), T(kp, cuda), 0.7)
            assert got == i1.cpu().numpy()[: int(n1.item())].tolist(), (lens, s)
            sel = np.nonzero(kp)[0]
            assert got == sel[S.nms(b[sel].astype(np.int64), sc[sel], 0.7)].tolist(), (lens, s)


def test_group_of_mixed_sizes_equals_image_by_image(cuda):
    """generate_group on five images of two sizes, interleaved (so a class's embeddings are gathered), with thresholds that
    decide and leave one image without a single survivor: per image the tensors of generate_device on that image alone.

    The image alone starts from the embedding the group's encoder pass gave it.  Sam.encode_batch equals Sam.encode only
    "up to the summation order of split-K" (its docstring: one image's mlp.lin2 runs split-K, a batch's does not), which
    moves the embedding by a few 1e-6 (printed below; measured 5.2e-6 .. 6.4e-6 at max |emb| = 5 on these images) and with it
    the last bits of the predicted IoUs, whichever tail runs behind it.  What this test pins is the
    tail: decoder, post-processing, both NMS passes, clean-up and gathers, bit for bit."""
    m = _vit_h_d2(cuda)
    try:
        _mixed_group(cuda, m)
    finally:
        del m
        _release()


def _mixed_group(cuda, m):
    from hybridgl_amd.synth import synth_image
    shapes = [(480, 640), (333, 500), (480, 640), (333, 500), (480, 640)]
    imgs = [torch.from_numpy(synth_image(h, w, 20 + i)).to(cuda) for i, (h, w) in enumerate(shapes)]
    resized = [hsam.resize_longest_side(im.contiguous(), m.img_size) for im in imgs]
    emb = m.encode_batch(resized)
    for i, r in enumerate(resized):
        d = (m.encode(r) - emb[i]).abs().max()
        print(f"image {i}: max |encode - encode_batch| = {float(d):.3e} (max |emb| {float(emb[i].abs().max()):.3e})")
    current = [None]
    m.encode_batch = lambda res: emb              # (this model dies with the test)
    m.encode = lambda r: emb[current[0]]
    probe = hsam.SamAutomaticMaskGenerator(m, points_per_side=8, pred_iou_thresh=-1e30, stability_score_thresh=0.0, box_nms_thresh=2.0)
    tops = []
    for i, im in enumerate(imgs):
        current[0] = i
        tops.append(float(probe.propose(im)[2].max()))
    order = np.argsort(tops)
    thr = tops[order[0]]                      # nothing of the image with the lowest best prediction exceeds it
    assert tops[order[1]] > thr, "two images share the lowest best prediction: choose other seeds"
    for area in (100, 0):
        gen = hsam.SamAutomaticMaskGenerator(m, points_per_side=8, pred_iou_thresh=thr, stability_score_thresh=0.5, box_nms_thresh=0.7,
                                             min_mask_region_area=area)
        got = gen.generate_group(imgs)
        assert len(got) == len(imgs)
        assert got[order[0]][0].shape[0] == 0 and sum(int(o[0].shape[0]) for o in got) > 0
        for i, (im, out) in enumerate(zip(imgs, got)):
            current[0] = i
            alone = gen.generate_device(im)
            for a, b in zip(alone, out):
                assert a.shape == b.shape and a.dtype == b.dtype, (area, i, a.shape, b.shape)
                assert torch.equal(a, b), (area, i)
