"""GPU: the opt-in fp16 precision mode ('f16': fp16 GEMM operands, one MFMA per product, fp32 accumulation).

The GEMMs are pinned EXACTLY: with both operands rounded to fp16 on the host (the weight after its power-of-two pre-scale),
the result equals the float64 product of the rounded operands within fp32-accumulation error.  The models are compared
with the f32 mode within bounds derived from the fp16 operand error (2^-11 relative per operand), and
against the f16x3 mode to show that the mode really multiplies hi halves only."""
import numpy as np
import pytest
import torch

from abi_ref import gemm_f16_reference
from hybridgl_amd import ops, weights

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


GEMM_CASES = [
    # M, N, K, bias, residual, act, tiling
    (600, 768, 768, True, False, "none", "auto"),       # CLIP qkv-like, ragged M
    (1000, 3072, 768, True, False, "gelu", "auto"),     # CLIP fc1 + GELU
    (391, 768, 3072, True, True, "none", "v1"),         # CLIP fc2 + residual, register-staged tiling
    (1300, 1280, 5120, True, True, "none", "P"),        # SAM lin2 + residual, ping-pong tiling
    (517, 3840, 1280, True, False, "none", "P"),        # SAM qkv
]


@pytest.mark.parametrize("M,N,K,has_b,has_r,act,tiling", GEMM_CASES)
def test_gemm_f16_is_the_fp16_operand_product(cuda, M, N, K, has_b, has_r, act, tiling):
    rng = np.random.default_rng(M + N + K)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) if has_b else None
    r = rng.standard_normal((M, N)).astype(np.float32) if has_r else None
    ref, bound = gemm_f16_reference(a, w, b, r, act)
    W = T(w, cuda)
    args = (T(a, cuda), W, T(b, cuda) if has_b else None, T(r, cuda) if has_r else None, act)
    try:
        ops.select_x3_kernel(tiling)
        ops.set_precision("f16")
        y16 = ops.gemm_f16x3(*args).cpu().numpy().astype(np.float64)
        ops.set_precision("f16x3")
        y3 = ops.gemm_f16x3(*args).cpu().numpy().astype(np.float64)
    finally:
        ops.select_x3_kernel("auto")
    assert ops.split_overflow_count() == 0
    ratio = np.abs(y16 - ref) / bound
    assert ratio.max() <= 1.0, (ratio.max(), np.abs(y16 - ref).max())
    # the three-term result is NOT the fp16-operand product (it carries the lo halves): far further from it than the f16 one
    assert 20.0 * np.abs(y16 - ref).max() < np.abs(y3 - ref).max()


def test_gemm_f16_row_balanced_split_k_tail(cuda):
    """The row-balanced launch (whole rounds of the persistent tiling + a split-K tail over the last row tiles): the tail rows
    and main rows both equal the fp16-operand product (the tail sums K slices in a fixed order: same bound)."""
    M, N, K = 66000, 768, 3072         # 258 x 3 tiles = 774 on 256 CUs: three full rounds and a six-tile tail
    rng = np.random.default_rng(7)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32)
    ops.set_precision("f16")
    y = ops.gemm_f16x3(T(a, cuda), T(w, cuda), T(b, cuda), T(r, cuda), balanced=True).cpu().numpy().astype(np.float64)
    assert ops.split_overflow_count() == 0
    rows = np.r_[0:300, M - 1100:M]
    ref, bound = gemm_f16_reference(a, w, b, r, "none", rows=rows)
    ratio = np.abs(y[rows] - ref) / bound
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("M,N,K,has_r", [(77, 512, 512, False), (300, 768, 768, True), (5, 1024, 3072, True)])
def test_skinny_gemm_f16(cuda, M, N, K, has_r):
    """Small-M GEMMs through ops.gemm with a registered weight take the skinny kernel: A rounded in registers, W_hi only."""
    rng = np.random.default_rng(M * 3 + K)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32) if has_r else None
    W = T(w, cuda)
    ops.register_split_weight(W)
    ops.set_precision("f16")
    y = ops.gemm(T(a, cuda), W, T(b, cuda), T(r, cuda) if has_r else None).cpu().numpy().astype(np.float64)
    ref, bound = gemm_f16_reference(a, w, b, r, "none")
    assert (np.abs(y - ref) / bound).max() <= 1.0
    ops.set_precision("f16x3")
    y3 = ops.gemm(T(a, cuda), W, T(b, cuda), T(r, cuda) if has_r else None).cpu().numpy().astype(np.float64)
    assert 20.0 * np.abs(y - ref).max() < np.abs(y3 - ref).max()


# ---- models: f16 against f32 on the same weights --------------------------------------------------------------------------

CLIP_MODES = ["G2L", "L2G", "G2L&L2G", "token_masking", "attn_masking", "crop"]


@pytest.fixture(scope="module")
def clip_models(cuda):
    """seeded ViT-B/16 in the three modes (the tiny geometry's width of 128 keeps every GEMM on the fp32 path)"""
    from hybridgl_amd.backbone import CLIPViTFM
    sd = weights.clip_state_dict("ViT-B/16", 0)
    return {p: CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision=p) for p in ("f32", "f16x3", "f16")}


def _clip_inputs(cuda):
    from oracle.cases import views_for_case
    loc, glo, masks = views_for_case(4, 224, 160, 200)
    return T(loc, cuda), T(glo, cuda), T(masks, cuda)


@pytest.mark.parametrize("mode", CLIP_MODES)
def test_clip_f16_against_f32(cuda, clip_models, mode):
    """Hybrid features of ViT-B/16 (12 blocks): f16 within 3e-3 relative of f32 and measurably different from f16x3 (which
    sits at 1e-5 of f32).  Derivation: every GEMM / attention product rounds both operands to fp16 (2 x 2^-11 = 1e-3
    relative per layer input); 12 blocks of residual updates add these incoherently (sqrt(24) x 1e-3 / a residual damping
    of ~2 = 2.4e-3 worst case).  Measured 2.7e-4 with the one-term GEMMs."""
    x = _clip_inputs(cuda)
    y = {p: m(*x, masking_block=9, fusion_mode=mode).cpu().numpy().astype(np.float64) for p, m in clip_models.items()}
    scale = np.abs(y["f32"]).max()
    e16 = np.abs(y["f16"] - y["f32"]).max() / scale
    e3 = np.abs(y["f16x3"] - y["f32"]).max() / scale
    assert np.isfinite(y["f16"]).all()
    assert e16 < 3e-3, e16
    assert e3 < 1e-4, e3
    assert e16 > 10 * e3, (e16, e3)
    assert ops.split_overflow_count() == 0


def test_clip_b16_stressed_weights_f16_cosine(cuda):
    """ViT-B/16 G2L with trained-checkpoint statistics (tests/stress_weights.py: LayerNorm gains up to 10, massive residual
    channels): the hybrid features of f16 keep a cosine above 0.995 with those of f32 for every proposal (measured on MI355X:
    min 0.9980, median 0.9998 -- the outlier channels cost fp16 operands more than seeded weights do)."""
    from hybridgl_amd.backbone import CLIPViTFM
    from oracle.cases import views_for_case
    from stress_weights import stress_clip_state_dict
    sd = stress_clip_state_dict(weights.clip_state_dict("ViT-B/16", 0))
    loc, glo, masks = views_for_case(6, 224, 160, 200)
    x = (T(loc, cuda), T(glo, cuda), T(masks, cuda))
    ys = {}
    for p in ("f32", "f16"):
        m = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision=p)
        ys[p] = m(*x, masking_block=9, fusion_mode="G2L").cpu().numpy().astype(np.float64)
        del m
    assert ops.split_overflow_count() == 0
    a, b = ys["f32"], ys["f16"]
    cos = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    assert cos.min() > 0.995, cos.min()


def test_sam_vit_h_d2_embedding_f16(cuda):
    """SAM ViT-H (two blocks, one windowed + one global) image embedding: f16 within 5e-3 relative (rms) of f32 (fp16
    operands: ~1e-3 per GEMM / attention input, a few incoherent terms per block; measured 8.7e-4 over all 32 blocks); the
    decoder of an f16 model runs its f16x3 arithmetic: on the same embedding it equals the f16x3 model's decoder bit for
    bit."""
    from hybridgl_amd import sam as hsam
    from hybridgl_amd.synth import synth_image
    cfg = weights.SAM_CONFIGS["vit_h_d2"]
    sd = weights.sam_state_dict("vit_h_d2", 0)
    img = T(synth_image(683, 1024, 5), cuda)
    embs, models = {}, {}
    for p in ("f32", "f16x3", "f16"):
        models[p] = hsam.Sam(sd, cfg, cuda, precision=p)
        embs[p] = models[p].encode(img)
    assert ops.split_overflow_count() == 0
    e32 = embs["f32"].double()
    rms = lambda t: float(t.pow(2).mean().sqrt())  # noqa: E731
    r16 = rms(embs["f16"].double() - e32) / rms(e32)
    r3 = rms(embs["f16x3"].double() - e32) / rms(e32)
    assert torch.isfinite(embs["f16"]).all()
    assert r16 < 5e-3, r16
    assert r16 > 10 * r3, (r16, r3)
    pts = T(np.random.default_rng(3).uniform(0.05, 0.95, (16, 2)).astype(np.float32), cuda)
    e = embs["f16x3"]
    low3, iou3 = models["f16x3"].decode_points(e, pts)
    low16, iou16 = models["f16"].decode_points(e, pts)
    assert torch.equal(low3, low16) and torch.equal(iou3, iou16)


def test_gem_heatmap_f16(cuda, clip_models):
    """GEM heat-map of ViT-B/16: f16 within 1e-2 of f32 (heat-maps are min-max normalised to [0, 1]; the tower's features
    carry the ~1e-3 relative fp16-operand error, the min-max normalisation can magnify it a few times)."""
    from hybridgl_amd import gem as G
    gimg = T(np.random.default_rng(5).standard_normal((3, 224, 224)).astype(np.float32), cuda)
    gtxt = T(np.random.default_rng(6).standard_normal((2, 512)).astype(np.float32), cuda)
    heat = {}
    for p in ("f32", "f16"):
        gm = G.create_gem_model("ViT-B/16", clip=clip_models[p])
        heat[p] = gm.heatmap(gm.image_features(gimg), gtxt, 224).cpu().numpy().astype(np.float64)
    assert np.isfinite(heat["f16"]).all()
    err = np.abs(heat["f16"] - heat["f32"]).max()
    print(f"GEM heat-map f16 vs f32: {err:.2e}")
    assert err < 1e-2, err


def test_activation_beyond_fp16_range_is_reported_in_f16_mode(cuda):
    """The fp16 range guard holds in f16 mode: an MLP unit driven past 65504 is counted and raised as SplitOverflow."""
    from hybridgl_amd.backbone import CLIPViTFM
    from oracle.cases import views_for_case
    sd = {k: np.array(v, copy=True) for k, v in weights.clip_state_dict("ViT-B/16", 0).items()}
    sd["visual.transformer.resblocks.3.mlp.c_fc.weight"][:8] *= np.float32(3.0e4)
    sd["visual.transformer.resblocks.3.mlp.c_fc.bias"][:8] = np.float32(1.0e5)
    loc, glo, masks = views_for_case(4, 224, 160, 200)
    ops.split_overflow_count()
    m = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision="f16")
    m(T(loc, cuda), T(glo, cuda), T(masks, cuda), masking_block=9, fusion_mode="G2L")
    with pytest.raises(ops.SplitOverflow, match="fp16 range"):
        ops.check_split_overflow()


_FRESH_F16X3 = """
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[2])
sys.path.insert(0, sys.argv[2] + '/tests')
from hybridgl_amd import weights
from hybridgl_amd.backbone import CLIPViTFM
from oracle.cases import views_for_case
dev = torch.device('cuda:0')
loc, glo, masks = views_for_case(4, 224, 160, 200)
m = CLIPViTFM('ViT-B/16', state_dict=weights.clip_state_dict('ViT-B/16', 1), device=dev, precision='f16x3')
y = m(torch.from_numpy(loc).to(dev), torch.from_numpy(glo).to(dev), torch.from_numpy(masks).to(dev), masking_block=9,
      fusion_mode='G2L')
np.save(sys.argv[1], y.cpu().numpy())
"""


def test_f16_and_f16x3_models_share_a_process(cuda, tmp_path):
    """Each model re-asserts its own mode on entry: an f16x3 model built AFTER an f16 model in this process gives, bit for
    bit, what the same model gives in a fresh process that never saw f16 (weights registered while f16 was current are
    the same split), before and after the f16 model runs again; the f16 model's outputs are not those of f16x3."""
    import os
    import subprocess
    import sys
    from hybridgl_amd.backbone import CLIPViTFM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sd = weights.clip_state_dict("ViT-B/16", 1)
    x = _clip_inputs(cuda)
    m16_first = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision="f16")
    m16_first(*x, masking_block=9, fusion_mode="G2L")
    m3 = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision="f16x3")
    y_before = m3(*x, masking_block=9, fusion_mode="G2L").clone()
    m16 = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision="f16")
    y16 = m16(*x, masking_block=9, fusion_mode="G2L").clone()
    y_after = m3(*x, masking_block=9, fusion_mode="G2L").clone()
    assert torch.equal(y_before, y_after)
    assert not torch.equal(y16, y_after)
    assert ops._lib.load().hgl_get_precision() == 1
    out = tmp_path / "fresh.npy"
    subprocess.run([sys.executable, "-c", _FRESH_F16X3, str(out), root], check=True, timeout=600)
    assert np.array_equal(np.load(out), y_after.cpu().numpy())


def test_driver_precision_flag(cuda, tmp_path):
    """hybridgl_amd.main --precision f16 --synthetic 4: runs and records the mode in the stats JSON and the result log."""
    import json
    from hybridgl_amd import main as drv
    stats = tmp_path / "stats.json"
    args = drv.default_argument_parser().parse_args([
        "--precision", "f16", "--synthetic", "4", "--stats_json", str(stats), "--result_dir", str(tmp_path / "log")])
    m = drv.main(args)
    assert m["n_sentences"] > 0
    assert json.load(open(stats))["stats"]["precision"] == "f16"
    log = open(next((tmp_path / "log").iterdir())).read()
    assert "precision: f16" in log


# ---- whole refs: the product loop in f16 against f32 ----------------------------------------------------------------------

def _one_sentence_refs(cuda):
    """the sentences of the whole-ref fixture's three images (oracle/gen_cases_e2e.py), one ref per sentence so that step()
    hands back every sentence's proposal scores; 12 given proposals per image, ViT-B/16 at 224 (the tiny geometry never
    leaves the fp32 path)"""
    from hybridgl_amd import synth
    from hybridgl_amd.pipeline import RefBatch, Sentence
    from oracle.gen_cases_e2e import E2E_CASES
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    refs = []
    for ci, (iseed, H, W, tseed, sents, gseed) in enumerate(E2E_CASES):
        img = synth.synth_image(H, W, iseed)
        masks = synth.synth_masks(12, H, W, 500 + ci)
        boxes = np.zeros((12, 4), np.int64)
        for i, m in enumerate(masks):
            ys, xs = np.nonzero(m)
            boxes[i] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) if len(xs) else 0
        gt = synth.synth_masks(1, H, W, gseed)[0]
        for j, (dirflag, rela, n_other) in enumerate(sents):
            tok = synth.synth_tokens(2 + n_other, 77, 49408, tseed + 31 * j)
            s = Sentence(0, 1, list(range(2, 2 + n_other)), dirflag, rela, n_other, t(synth.synth_heatmap(H, W, 6000 + 10 * ci + j)))
            refs.append(RefBatch(t(img), None, t(synth.imagenet_normalize(img)), t(masks), t(boxes), t(tok), t(gt), [s],
                                 token_len=int(tok.argmax(axis=1).max()) + 1, index=len(refs)))
    return refs


def test_whole_refs_f16_pick_the_f32_winners(cuda):
    """The product loop (views -> hybrid forward -> text encoder -> scoring tail -> IoU) in f16 against f32 on the same
    refs.  SCORE_BOUND bounds |score_f16 - score_f32| for every proposal (checked here); wherever the f32 top-2 margin
    exceeds twice that bound the winner cannot move and must be the same; flips below it are reported, not failed.  The
    IoU counts of the refs whose winners agree are identical."""
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.pipeline import HybridGLPipeline
    sd = weights.clip_state_dict("ViT-B/16", 0)
    out = {}
    for p in ("f32", "f16"):
        model = CLIPViTFM("ViT-B/16", state_dict=sd, device=cuda, precision=p)
        pipe = HybridGLPipeline(model, fusion_mode="G2L", masking_block=9, res=224)
        scores = []
        for r in _one_sentence_refs(cuda):
            _, _, last = pipe.step(r)
            scores.append(last[1].double().cpu().numpy().reshape(-1))
        torch.cuda.synchronize()
        out[p] = (np.concatenate([np.asarray(pipe.winning_indices())], 0), np.asarray(pipe.partial_rows()), scores)
        del pipe, model
    assert ops.split_overflow_count() == 0
    idx32, rows32, sc32 = out["f32"]
    idx16, rows16, sc16 = out["f16"]
    scale = max(np.abs(s).max() for s in sc32)
    SCORE_BOUND = 5e-3 * scale          # ~1e-3 relative feature error through a cosine and the fusion: measured below
    dmax = max(np.abs(a - b).max() for a, b in zip(sc16, sc32))
    print(f"whole refs: max |score f16 - f32| = {dmax:.3e} (bound {SCORE_BOUND:.3e}, score scale {scale:.3e})")
    assert dmax <= SCORE_BOUND, (dmax, SCORE_BOUND)
    flips = 0
    for i, s in enumerate(sc32):
        top = np.sort(s)[::-1]
        margin = top[0] - top[1] if len(top) > 1 else np.inf
        same = idx16[i][0] == idx32[i][0]      # the pure winner: the arg-max of these scores
        if margin > 2 * SCORE_BOUND:
            assert same, (i, idx16[i].tolist(), idx32[i].tolist(), margin)
        elif not same:
            flips += 1
        for k in (0, 1):                        # IoU counts (I, U) of the pure / spatially guided winner where they agree
            if idx16[i][k] == idx32[i][k]:
                assert np.array_equal(rows16[i, 2 + 2 * k:4 + 2 * k], rows32[i, 2 + 2 * k:4 + 2 * k]), (i, k)
    print(f"whole refs: {flips} of {len(sc32)} sentences flip inside the bound")


# ---- attention: the one-term flavours against float64 on fp16-rounded operands ---------------------------------------------

ATTN_CASES = [
    # B, heads, S, hd, rel (kh = kw), what it exercises
    (24, 12, 197, 64, 0),      # CLIP sequences: two query tiles per wave (attn_x3q_kernel)
    (6, 16, 196, 80, 14),      # SAM 14 x 14 windows, rel-pos terms on the matrix cores (attn_x3_kernel<80, 14>)
    (6, 2, 196, 64, 14),       # windows at head dim 64 (ViT-B geometry)
    (1, 2, 4096, 80, 64),      # SAM global block, rel-pos tensors (ping-pong attn_x3pp_kernel)
]


@pytest.mark.parametrize("B,H,S,hd,rel", ATTN_CASES)
def test_attention_f16_is_the_fp16_operand_attention(cuda, B, H, S, hd, rel):
    """softmax(fp16(q * scale) fp16(k)^T + bias) fp16(v) in float64 is what the f16 flavours compute, up to the fp16
    rounding of P (round to nearest, <= 2^-11 relative per probability: <= 2^-11 max|v| on the output; bound 2^-10 max|v|)
    and fp32 accumulation; the f16x3 kernels (unrounded operands) sit further from it."""
    rng = np.random.default_rng(S + hd + rel)
    D = H * hd
    q = rng.standard_normal((B, S, D)).astype(np.float32)
    k = rng.standard_normal((B, S, D)).astype(np.float32)
    v = rng.standard_normal((B, S, D)).astype(np.float32)
    scale = hd ** -0.5
    rh = rw = None
    if rel:
        rh = (0.5 * rng.standard_normal((B * H, S, rel))).astype(np.float32)
        rw = (0.5 * rng.standard_normal((B * H, S, rel))).astype(np.float32)
    args = dict(scale=scale, rel_h=T(rh, cuda) if rel else None, rel_w=T(rw, cuda) if rel else None)
    ops.set_precision("f16")
    y16 = ops.attention(T(q, cuda), T(k, cuda), T(v, cuda), H, **args).cpu().numpy().astype(np.float64)
    ops.set_precision("f16x3")
    y3 = ops.attention(T(q, cuda), T(k, cuda), T(v, cuda), H, **args).cpu().numpy().astype(np.float64)
    r16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
    qs = r16(q * np.float32(scale)).reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    ks = r16(k).reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    vs = r16(v).reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    sc = qs @ ks.transpose(0, 1, 3, 2)
    if rel:
        key = np.arange(S)
        sc = sc + rh.reshape(B, H, S, rel).astype(np.float64)[..., key // rel] + rw.reshape(B, H, S, rel).astype(np.float64)[..., key % rel]
    p = np.exp(sc - sc.max(-1, keepdims=True))
    ref = ((p / p.sum(-1, keepdims=True)) @ vs).transpose(0, 2, 1, 3).reshape(B, S, D)
    bound = 2.0 ** -10 * np.abs(v).max() + 1e-5
    e16 = np.abs(y16 - ref).max()
    e3 = np.abs(y3 - ref).max()
    print(f"attention {B}x{H}x{S}x{hd} rel {rel}: f16 {e16:.2e}, f16x3 {e3:.2e} (bound {bound:.2e})")
    assert np.isfinite(y16).all() and e16 <= bound, (e16, bound)
    assert np.sqrt(((y16 - ref) ** 2).mean()) < np.sqrt(((y3 - ref) ** 2).mean())
