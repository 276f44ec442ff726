"""Host-only checks of tests/decoder_cases.py: the float64 reference of the SAM prompt encoder + mask decoder against
oracle/sam_oracle.py (which tests/golden pins to the reference project), the stress knob, and the case table against the
restated route.

The bar between the two references is 1e-4 * max(1, |ref|): about twenty times the fp32 / float64 gap measured on the CPU
(5.4e-6 on the logits, 5.7e-7 on the IoU head at 24 x 24).  It is a check of two references against each other, not of a kernel.
"""
import numpy as np
import pytest

import decoder_cases as D
from hybridgl_amd import weights
from oracle import sam_oracle as S
from oracle.cases import sam_tiny_case

G = 16          # the tiny golden geometry: 16 x 16 tokens, a 256-pixel input
SIZE = 256


@pytest.fixture(scope="module")
def sd():
    return weights.sam_state_dict("tiny", 0)


@pytest.fixture(scope="module")
def emb():
    return np.random.default_rng(7).standard_normal((G, G, 256)).astype(np.float32)


def _close(got, ref, what):
    err = float(np.abs(got - ref).max())
    bar = 1e-4 * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: max |float64 - oracle| {err:.3e} (bar {bar:.3e})")
    assert np.isfinite(got).all() and err <= bar, (what, err, bar)


def test_prompt_encoder_equals_the_oracle(sd):
    pts = sam_tiny_case()["points_in"]
    _close(D.embed_points(sd, pts, SIZE), S.embed_points(sd, pts, SIZE), "embed_points")
    rng = np.random.default_rng(1)
    co = np.floor(rng.random((4, 3, 2)) * SIZE)
    lab = np.array([[1, 0, -1], [0, 2, 3], [1, 1, -1], [2, 3, -1]])
    _close(D.embed_prompts(sd, co, lab, SIZE), S.embed_prompts(sd, co, lab, SIZE), "embed_prompts")
    _close(D.embed_prompts(sd, co.astype(np.float32), lab, SIZE), S.embed_prompts(sd, co.astype(np.float32), lab, SIZE),
           "embed_prompts (fp32 coordinates)")
    _close(D.dense_pe(sd, 12, 12), S.dense_pe(sd, 12, 12), "dense_pe")
    mask_in = (4.0 * rng.standard_normal((2, 1, 4 * G, 4 * G))).astype(np.float32)
    _close(D.embed_masks(sd, mask_in), S.embed_masks(sd, mask_in), "embed_masks")


def test_mask_decoder_equals_the_oracle_on_points(sd, emb):
    pts = sam_tiny_case()["points_in"]
    low, iou = D.mask_decoder(sd, emb, D.embed_points(sd, pts, SIZE))
    rlow, riou = S.mask_decoder(sd, emb, S.embed_points(sd, pts, SIZE))
    assert low.dtype == np.float64 and low.shape == rlow.shape == (len(pts), 3, 64, 64) and iou.shape == riou.shape
    _close(low, rlow, "points: logits")
    _close(iou, riou, "points: iou")
    # a list of prompts gives those prompts' rows and nothing else enters them
    inter = {}
    low2, iou2 = D.mask_decoder(sd, emb, D.embed_points(sd, pts, SIZE), prompts=[3, 1], inter=inter)
    assert np.abs(low2 - low[[3, 1]]).max() < 1e-12 and np.abs(iou2 - iou[[3, 1]]).max() < 1e-12
    assert inter["keys_l1"].shape == (2, G * G, 256) and inter["queries_final"].shape == (2, 7, 256)
    assert inter["upscaled"].shape == (2, 4 * G, 4 * G, 32) and inter["hyper"].shape == (2, 4, 32)


def test_mask_decoder_equals_the_oracle_on_three_token_prompts_and_single_mask(sd, emb):
    rng = np.random.default_rng(2)
    co = np.floor(rng.random((4, 3, 2)) * SIZE)
    co[:, 2] = 0.0
    lab = np.array([[1, 0, -1], [0, 0, -1], [1, 1, -1], [0, 1, -1]])
    for mm in (True, False):
        low, iou = D.mask_decoder(sd, emb, D.embed_prompts(sd, co, lab, SIZE), multimask=mm)
        rlow, riou = S.mask_decoder(sd, emb, S.embed_prompts(sd, co, lab, SIZE), multimask=mm)
        assert low.shape == rlow.shape == (4, 3 if mm else 1, 64, 64)
        _close(low, rlow, f"three tokens, multimask {mm}: logits")
        _close(iou, riou, f"three tokens, multimask {mm}: iou")


def test_mask_decoder_equals_the_oracle_on_a_box_with_a_mask_input(sd, emb):
    rng = np.random.default_rng(3)
    co = np.sort(np.floor(rng.random((3, 2, 2)) * SIZE), axis=1)
    lab = np.tile(np.array([2, 3]), (3, 1))
    mask_in = (4.0 * rng.standard_normal((3, 1, 4 * G, 4 * G))).astype(np.float32)
    low, iou = D.mask_decoder(sd, emb, D.embed_prompts(sd, co, lab, SIZE), dense=D.embed_masks(sd, mask_in))
    rlow, riou = S.mask_decoder(sd, emb, S.embed_prompts(sd, co, lab, SIZE), dense=S.embed_masks(sd, mask_in))
    _close(low, rlow, "box + mask input: logits")
    _close(iou, riou, "box + mask input: iou")


def test_stress_knob_sharpens_the_soft_max_and_both_references_hold(sd, emb, monkeypatch):
    """stress_decoder(sd, 16): the ORACLE stays finite, the widest score range of one of its token -> image rows exceeds 150 and
    its peak probability 0.999 (measured on the oracle's own soft-max calls), and the two references still agree"""
    hot = D.stress_decoder(sd, 16)
    for a in D.T2I_ATTENTIONS:
        assert np.array_equal(hot[f"{a}.q_proj.weight"], sd[f"{a}.q_proj.weight"] * np.float32(16))
        assert np.array_equal(hot[f"{a}.k_proj.weight"], sd[f"{a}.k_proj.weight"])
    assert np.array_equal(hot["mask_decoder.transformer.layers.0.self_attn.q_proj.weight"],
                          sd["mask_decoder.transformer.layers.0.self_attn.q_proj.weight"])
    assert D.stress_decoder(sd, 1)["mask_decoder.transformer.final_attn_token_to_image.q_proj.bias"].tobytes() == \
        sd["mask_decoder.transformer.final_attn_token_to_image.q_proj.bias"].tobytes()
    seen = [0.0, 0.0]
    plain = S.softmax

    def watched(x, axis=-1):
        out = plain(x, axis=axis)
        if x.shape[-1] == G * G:        # keys = the image tokens: a token -> image attention
            seen[0] = max(seen[0], float((x.max(-1) - x.min(-1)).max()))
            seen[1] = max(seen[1], float(out.max()))
        return out

    monkeypatch.setattr(S, "softmax", watched)
    pts = sam_tiny_case()["points_in"]
    rlow, riou = S.mask_decoder(hot, emb, S.embed_points(hot, pts, SIZE))
    inter = {}
    low, iou = D.mask_decoder(hot, emb, D.embed_points(hot, pts, SIZE), inter=inter)
    print(f"temp 16: oracle score range {seen[0]:.1f}, peak probability {seen[1]:.6f}; float64 {inter['score_range']:.1f}, "
          f"{inter['peak_probability']:.6f}")
    assert np.isfinite(rlow).all() and np.isfinite(riou).all()
    assert seen[0] > 150 and seen[1] > 0.999
    assert inter["score_range"] > 150 and inter["peak_probability"] > 0.999
    _close(low, rlow, "temp 16: logits")
    _close(iou, riou, "temp 16: iou")
    calm = {}
    D.mask_decoder(sd, emb, D.embed_points(sd, pts, SIZE), inter=calm)
    assert calm["score_range"] < 40 and calm["peak_probability"] < 0.9     # the seeded weights alone never push the soft-max


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_case_is_well_formed(c):
    """the route fields a case names and the kernels it lists, both written by hand, against the restated dec_route"""
    assert c.kind in D.N_SPARSE and c.precision in ("f16x3", "f32") and c.temp in (1, 4, 16) and c.first_mask in (0, 1)
    assert c.P >= 1 and c.n_img >= 1 and (c.n_img == 1) == (c.kind != "multi")
    assert c.kernels <= set(D.KERNELS)
    r = D.case_route(c)
    for field, want in c.route.items():
        assert getattr(r, field) == want, (c.name, field, getattr(r, field), want)
    assert D.route_kernels(r, c.kind == "dense") == c.kernels, (c.name, sorted(D.route_kernels(r, c.kind == "dense")), sorted(c.kernels))
    inp = D.case_inputs(c)
    assert inp["emb"].shape == (c.n_img, c.grid, c.grid, 256)
    pts = inp["pts"] if "pts" in inp else inp["co"][:, 0]
    assert pts.min() >= 0 and pts.max() <= inp["size"] - 1
    if c.kind != "dense":      # (a box's corners are sorted)
        for img in range(c.n_img):
            assert tuple(pts[img * c.P]) == (0.0, 0.0) and tuple(pts[(img + 1) * c.P - 1]) == (inp["size"] - 1.0,) * 2
            assert {0, c.P - 1} <= set(D.checked_prompts(c.P))


def test_names_are_unique_and_the_table_covers_every_route_value():
    """every value of every DecRoute field that the decoder geometry can produce occurs in some case's route"""
    names = [c.name for c in D.CASES]
    assert len(set(names)) == len(names)
    routes = [D.case_route(c) for c in D.CASES]
    for field in ("x3", "merged", "raw_t2i", "fused_tail", "multi"):
        assert {getattr(r, field) for r in routes} == {True, False}, field
    assert {r.ns for r in routes if r.raw_t2i} == {1, 8}
    assert {r.shared for r in routes} == {(True, False), (False, False)}
    assert {r.plain for r in routes} == {(False, False), (True, False)}
    assert {r.fuse_i2t for r in routes} == {(True, True), (False, True), (False, False)}      # (True, False) cannot occur
    assert {r.chunked for r in routes} == {(True,) * 3, (False,) * 3}                           # one condition for all three
    # the capacity facts of the module docstring
    assert not D.dec_route(16, 5).raw_t2i and not D.dec_route(16, 129).raw_t2i and not D.dec_route(32, 5).raw_t2i
    assert D.dec_route(32, 129).raw_t2i and D.dec_route(48, 5).raw_t2i and D.dec_route(128, 2).raw_t2i
    assert not any(D.dec_route(g, 5).raw_t2i for g in range(1, 48))


def test_kernel_id_tells_the_two_image_to_token_kernels_apart():
    assert D.kernel_id("void (anonymous namespace)::dec_i2t_fold_kernel((anonymous namespace)::I2TFArgs)") == "dec_i2t_fold_kernel"
    assert D.kernel_id("_ZN12_GLOBAL__N_114dec_i2t_kernelENS_7I2TArgsE") == "dec_i2t_kernel"
    assert D.kernel_id("_ZN12_GLOBAL__N_119t2i_raw_attn_kernelENS_7T2IArgsE") == "t2i_raw_attn_kernel"
    assert D.kernel_id("attn_kernel") == "t2i_raw_attn_kernel" and D.kernel_id("attn_x3_kernel<16,0,4,3>") is None
    assert D.kernel_id("attn_fewq_chunk_kernel") == "attn_fewq_chunk_kernel" and D.kernel_id("attn_fewq_combine_kernel") is None
    assert D.kernel_id("i2t_prep_kernel(float const*)") == "i2t_prep_kernel" and D.kernel_id("gemm_x3_kernel<1>") is None
