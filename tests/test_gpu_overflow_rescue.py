"""GPU: HybridGLPipeline(on_overflow="rescue") -- an activation beyond the fp16 range makes run() do the groups that were in
flight again in f32 instead of raising -- with its two building blocks, ops.split_overflow_snapshot (all three range counters
in stream order) and ops.forced_precision (a model built in f16x3 / f16 run in f32 gives the f32-built model's bits).

The geometry is that of test_overflow_stops_the_loop_at_the_offending_group_not_at_the_end (tests/test_gpu_precision.py):
ViT-B/16 seed 0 with eight units of resblocks.3.mlp.c_fc driven past 65504 (that test shows that this unit is counted), the
tiny SAM with open filters, refs of 96 x 128 with 4 proposals, groups of 2.  The yardstick of a rescued run is a pipeline
whose models are BUILT with precision="f32" from the same weights: equality is bit for bit."""
import numpy as np
import pytest
import torch

from hybridgl_amd import ops, weights

pytestmark = pytest.mark.gpu

CLIP_MODES = ["G2L", "L2G", "G2L&L2G", "token_masking", "attn_masking", "crop"]
SWEEP = [(0.5, 0.6, 3, 6), (0.3, 0.4, 2, 4)]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def world(cuda):
    """the models of every loop test, built once: poisoned and clean ViT-B/16 and the tiny SAM's generator, in f16x3 and f32"""
    from hybridgl_amd import sam as hsam
    from hybridgl_amd.backbone import CLIPViTFM
    from hybridgl_amd.pipeline import synthetic_ref
    ok = weights.clip_state_dict("ViT-B/16", 0)
    bad = {k: np.array(v, copy=True) for k, v in ok.items()}
    bad["visual.transformer.resblocks.3.mlp.c_fc.weight"][:8] *= np.float32(3.0e4)
    bad["visual.transformer.resblocks.3.mlp.c_fc.bias"][:8] = np.float32(1.0e5)
    w = {"refs": [synthetic_ref(i, cuda, N=4, H=96, W=128)[0] for i in range(12)]}
    ssd = weights.sam_state_dict("tiny", 0)
    for p in ("f16x3", "f32"):
        w["bad", p] = CLIPViTFM("ViT-B/16", state_dict=bad, device=cuda, precision=p)
        w["ok", p] = CLIPViTFM("ViT-B/16", state_dict=ok, device=cuda, precision=p)
        tiny = hsam.Sam(ssd, weights.SAM_CONFIGS["tiny"], cuda, precision=p)
        w["gen", p] = hsam.SamAutomaticMaskGenerator(tiny, points_per_side=3, pred_iou_thresh=-1e30, stability_score_thresh=0.0,
                                                     box_nms_thresh=2.0, min_mask_region_area=0)
    torch.cuda.synchronize()
    ops.split_overflow_count()
    return w


def outputs(pipe, first=0):
    """what a run leaves behind, from row / collected entry `first` on"""
    rows = pipe.partial_rows()
    n = len(rows) - first if first else len(rows)
    return dict(rows=rows[-n:], win=pipe.winning_indices()[-n:], hybrid=[c[0] for c in pipe.collected])


def same(a, b):
    assert np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["win"], b["win"])
    assert len(a["hybrid"]) == len(b["hybrid"])
    for x, y in zip(a["hybrid"], b["hybrid"]):
        assert torch.equal(x, y)


def run_reference(world, clip, prec, n, sam=True, **kw):
    """the all-`prec` pipeline: models built in that precision, serial, groups of 2"""
    from hybridgl_amd.pipeline import HybridGLPipeline
    pipe = HybridGLPipeline(world[clip, prec], mask_generator=world["gen", prec] if sam else None, use_sam_masks=sam, **kw)
    assert pipe.run(iter(world["refs"][:n]), group=2, proposal_cap=4 if sam else None, serial=True, collect=True) == n
    torch.cuda.synchronize()
    ops.split_overflow_count()      # (the f16x3 reference of the poisoned model is never asked for; a clean one counts nothing)
    return pipe


@pytest.fixture(scope="module")
def f32_bad(world):
    pipe = run_reference(world, "bad", "f32", 10)
    return pipe, outputs(pipe), pipe.metrics()


@pytest.mark.parametrize("serial", [True, False])
def test_every_group_overflows_and_the_run_equals_the_f32_pipeline(cuda, world, f32_bad, serial):
    from hybridgl_amd.pipeline import HybridGLPipeline
    _, want, want_metrics = f32_bad
    ops.split_overflow_count()
    pipe = HybridGLPipeline(world["bad", "f16x3"], mask_generator=world["gen", "f16x3"], use_sam_masks=True, on_overflow="rescue")
    assert pipe.run(iter(world["refs"][:10]), group=2, proposal_cap=4, serial=serial, collect=True) == 10
    st = pipe.rescue_stats
    print("rescue_stats", st)
    assert st["refs"] == 10 and st["groups"] == 5 and sorted(st["positions"]) == list(range(10)) and st["events"] >= 2
    assert pipe.groups_run == 5                       # the loop's groups, not the re-runs
    got = outputs(pipe)
    same(got, want)
    assert pipe.metrics() == want_metrics             # (does not raise: the counters are zero after a rescued run)
    assert ops.split_overflow_count() == 0
    assert world["gen", "f16x3"].overflow_snapshot is False      # the generator is as run() found it
    # a second run of the same pipeline: the same bits again
    events = st["events"]
    assert pipe.run(iter(world["refs"][:10]), group=2, proposal_cap=4, serial=serial, collect=True) == 10
    same(outputs(pipe, first=len(want["rows"])), want)
    assert pipe.rescue_stats["refs"] == 20 and pipe.rescue_stats["events"] == 2 * events
    assert ops.split_overflow_count() == 0


def test_predictions_and_sweep_of_a_rescued_run_equal_the_f32_pipeline(cuda, world):
    from hybridgl_amd.pipeline import HybridGLPipeline
    ref = run_reference(world, "bad", "f32", 10, record_predictions=True, sweep=SWEEP)
    pipe = HybridGLPipeline(world["bad", "f16x3"], mask_generator=world["gen", "f16x3"], use_sam_masks=True, on_overflow="rescue",
                            record_predictions=True, sweep=SWEEP)
    assert pipe.run(iter(world["refs"][:10]), group=2, proposal_cap=4, collect=True) == 10
    assert pipe.rescue_stats["refs"] == 10
    same(outputs(pipe), outputs(ref))
    assert pipe.predictions() == ref.predictions()
    assert np.array_equal(pipe.sweep_rows(), ref.sweep_rows())
    assert np.array_equal(pipe.sweep_indices(), ref.sweep_indices())
    assert np.array_equal(pipe.ceiling_rows(), ref.ceiling_rows())
    assert torch.equal(pipe.sweep_cum, ref.sweep_cum) and torch.equal(pipe.sweep_cum_ceiling, ref.sweep_cum_ceiling)
    assert torch.equal(pipe.cum, ref.cum)
    assert ops.split_overflow_count() == 0


def test_mixed_run_only_the_groups_in_flight_are_done_again(cuda, world):
    """Clean models; the loader provokes one counted overflow (the GEMM of test_split_overflow_is_counted_and_raised) just before
    it yields ref 4.  The refs done again carry the f32 pipeline's features, every other ref the f16x3 pipeline's."""
    from hybridgl_amd.pipeline import HybridGLPipeline
    f32 = outputs(run_reference(world, "ok", "f32", 12))["hybrid"]
    x3 = outputs(run_reference(world, "ok", "f16x3", 12))["hybrid"]
    assert len(f32) == len(x3) == 12
    for a, b in zip(f32, x3):
        assert a.shape != b.shape or not torch.equal(a, b)      # or the test below shows nothing
    rng = np.random.default_rng(3)
    a2 = rng.standard_normal((256, 128)).astype(np.float32)
    w = T((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32), cuda)
    a2[3, 5] = 1.0e6
    a2[7, 9] = -3.0e5
    a2 = T(a2, cuda)

    def loader():
        for i, r in enumerate(world["refs"]):
            if i == 4:
                ops.gemm_f16x3(a2, w)
            yield r

    ops.split_overflow_count()
    pipe = HybridGLPipeline(world["ok", "f16x3"], mask_generator=world["gen", "f16x3"], use_sam_masks=True, on_overflow="rescue")
    assert pipe.run(loader(), group=2, proposal_cap=4, collect=True) == 12
    st = pipe.rescue_stats
    print("rescue_stats", st)
    assert st["events"] == 1
    pos = st["positions"]
    assert pos == list(range(pos[0], pos[0] + len(pos))) and pos[0] % 2 == 0 and len(pos) % 2 == 0      # whole consecutive groups
    assert 1 <= len(pos) // 2 <= 3 and st["groups"] == len(pos) // 2 and st["refs"] == len(pos)
    assert not set(pos) & {8, 9, 10, 11}
    got = [c[0] for c in pipe.collected]
    assert len(got) == 12
    for i in range(12):
        assert torch.equal(got[i], f32[i] if i in pos else x3[i]), i
    assert [int(r[0]) for r in pipe.partial_rows()[::3]] == list(range(12))      # every ref once, in the loader's order
    assert pipe.groups_run == 6
    pipe.metrics()
    assert ops.split_overflow_count() == 0


def test_given_proposals_without_a_generator_are_rescued_in_the_loop(cuda, world):
    """no count read-back exists in this configuration: before, nothing was noticed until metrics()"""
    from hybridgl_amd.pipeline import HybridGLPipeline
    ref = run_reference(world, "bad", "f32", 10, sam=False)
    ops.split_overflow_count()
    pipe = HybridGLPipeline(world["bad", "f16x3"], mask_generator=None, use_sam_masks=False, on_overflow="rescue")
    assert pipe.run(iter(world["refs"][:10]), group=2, collect=True) == 10
    assert pipe.rescue_stats["refs"] == 10 and pipe.rescue_stats["events"] >= 2
    same(outputs(pipe), outputs(ref))
    assert pipe.metrics() == ref.metrics()
    assert ops.split_overflow_count() == 0
    # the same with a generator whose proposals nobody consumes (the synthetic benchmark's configuration): its kernels run
    # beside the CLIP stage, and the stage-end snapshot is taken behind them
    pipe = HybridGLPipeline(world["bad", "f16x3"], mask_generator=world["gen", "f16x3"], use_sam_masks=False, on_overflow="rescue")
    assert pipe.run(iter(world["refs"][:10]), group=2, collect=True) == 10
    assert pipe.rescue_stats["refs"] == 10
    same(outputs(pipe), outputs(ref))
    assert pipe.metrics() == ref.metrics()
    assert ops.split_overflow_count() == 0


# ---- the image cache across a roll-back ---------------------------------------------------------------------------------------

CACHE_IMAGES = [0, 1, 3, 4, 0, 2, 5, 2, 6, 7, 2, 1]      # the image of the ref at every position; groups of 2


def _cache_refs(world):
    import dataclasses
    return [dataclasses.replace(world["refs"][img], image_id=100 + img, index=pos) for pos, img in enumerate(CACHE_IMAGES)]


def _cache_run(world, prec, loader=None, **kw):
    from hybridgl_amd.pipeline import HybridGLPipeline
    pipe = HybridGLPipeline(world["ok", prec], mask_generator=world["gen", prec], use_sam_masks=True, **kw)
    refs = _cache_refs(world)
    assert pipe.run(loader(refs) if loader else iter(refs), group=2, proposal_cap=4, collect=True) == 12
    torch.cuda.synchronize()
    return pipe


def test_image_cache_entries_of_rolled_back_groups_leave_and_those_of_committed_groups_stay(cuda, world):
    """Refs that share images across the commit boundary, on two streams, one counted overflow provoked just before ref 8 is
    yielded: the loop is then pulling the group of refs 6, 7 and has committed the group of refs 0, 1 (it has read that group's
    snapshot), so the groups done again are those of refs 2..7 or 4..9 (the other stream decides which, as in the mixed run).
    An image's features are those of the pass that filed its cache entry and was not rolled back.  Positions 4 and 11 find images
    0 and 1 as the committed first group filed them (f16x3, although ref 4 is done again in f32).  Image 2 was filed at position 5
    by a pass that is rolled back: the entry is evicted and filed again by the f32 re-run, and position 7 (the first time a
    look-up in the pending group, in the re-run one in the cache) and position 10, in a later group that runs in f16x3, take
    the f32 entry like any other."""
    ops.split_overflow_count()
    f32 = [c[0] for c in _cache_run(world, "f32").collected]
    ref = _cache_run(world, "f16x3")
    x3 = [c[0] for c in ref.collected]
    assert ref.cache_hits == 4
    for a, b in zip(f32, x3):
        assert a.shape != b.shape or not torch.equal(a, b)
    rng = np.random.default_rng(3)
    a2 = rng.standard_normal((256, 128)).astype(np.float32)
    a2[3, 5] = 1.0e6
    a2 = T(a2, cuda)
    w = T((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32), cuda)

    def loader(refs):
        for i, r in enumerate(refs):
            if i == 8:
                ops.gemm_f16x3(a2, w)
            yield r

    pipe = _cache_run(world, "f16x3", loader, on_overflow="rescue")
    st = pipe.rescue_stats
    print("rescue_stats", st)
    pos = st["positions"]
    assert st["events"] == 1 and pos == list(range(pos[0], pos[0] + len(pos))) and pos[0] % 2 == 0 and len(pos) % 2 == 0
    assert 0 not in pos and {4, 5, 6, 7} <= set(pos) and 10 not in pos
    filed, want = {}, []
    for p, img in enumerate(CACHE_IMAGES):      # the cache holds all eight images: nothing is evicted for room
        filed.setdefault(img, "f32" if p in pos else "f16x3")
        want.append(filed[img])
    print("features expected", want)
    assert [want[p] for p in (4, 5, 7, 10, 11)] == ["f16x3", "f32", "f32", "f32", "f16x3"]
    got = [c[0] for c in pipe.collected]
    for p in range(12):
        assert torch.equal(got[p], f32[p] if want[p] == "f32" else x3[p]), p
    assert pipe.cache_hits == ref.cache_hits and list(pipe._img_cache) == list(ref._img_cache)
    assert [int(r[0]) for r in pipe.partial_rows()[::3]] == list(range(12))
    pipe.metrics()
    assert ops.split_overflow_count() == 0


# ---- a generator behind a wrapper ---------------------------------------------------------------------------------------------

class _Through:
    """a wrapper that hands every attribute it does not have on to its generator, as ProposalRecorder does"""

    def __init__(self, generator):
        self.generator = generator

    def __getattr__(self, name):
        if name == "generator":
            raise AttributeError(name)
        return getattr(self.generator, name)


def test_wrapped_generator_keeps_its_two_word_read_back_and_the_run_is_rescued(cuda, world, f32_bad):
    """the three-word read-back is switched on only at the object that makes it; behind a wrapper the stage-end snapshots alone
    decide, and neither the wrapper nor the generator is left with a changed attribute"""
    from hybridgl_amd.pipeline import HybridGLPipeline
    _, want, want_metrics = f32_bad
    ops.split_overflow_count()
    gen = _Through(world["gen", "f16x3"])
    pipe = HybridGLPipeline(world["bad", "f16x3"], mask_generator=gen, use_sam_masks=True, on_overflow="rescue")
    assert pipe.run(iter(world["refs"][:10]), group=2, proposal_cap=4, collect=True) == 10
    assert pipe.rescue_stats["refs"] == 10
    same(outputs(pipe), want)
    assert pipe.metrics() == want_metrics
    assert "overflow_snapshot" not in vars(gen) and world["gen", "f16x3"].overflow_snapshot is False
    assert ops.split_overflow_count() == 0


def test_recorder_and_rescue_exclude_each_other(cuda, world, tmp_path):
    """a ProposalRecorder's files are no part of the roll-back: run() refuses before anything is enqueued or written"""
    import os
    from hybridgl_amd.pipeline import HybridGLPipeline
    from hybridgl_amd.proposals import ProposalRecorder
    rec = ProposalRecorder(world["gen", "f16x3"], tmp_path / "store")
    pipe = HybridGLPipeline(world["ok", "f16x3"], mask_generator=rec, use_sam_masks=True, on_overflow="rescue")
    with pytest.raises(ValueError, match="ProposalRecorder"):
        pipe.run(iter(_cache_refs(world)), group=2, proposal_cap=4)
    assert rec.flush() == 0 and not os.path.exists(tmp_path / "store")
    assert "overflow_snapshot" not in vars(rec) and world["gen", "f16x3"].overflow_snapshot is False
    # the default mode records as before
    pipe = HybridGLPipeline(world["ok", "f16x3"], mask_generator=rec, use_sam_masks=True)
    assert pipe.run(iter(_cache_refs(world)[:4]), group=2, proposal_cap=4) == 4
    assert rec.flush() == 4
    assert ops.split_overflow_count() == 0


def test_null_pointer_is_refused_with_a_device(cuda):
    from hybridgl_amd import _lib
    lib = _lib.load()
    assert lib.hgl_split_overflow_snapshot_async(None, None) == -1      # HGL_EINVAL
    assert ops.split_overflow_count() == 0


# ---- ops.forced_precision -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_models(cuda):
    from hybridgl_amd import gem as G
    from hybridgl_amd import sam as hsam
    from hybridgl_amd.backbone import CLIPViTFM
    csd, ssd = weights.clip_state_dict("tiny", 0), weights.sam_state_dict("tiny", 0)
    out = {}
    for p in ("f32", "f16x3", "f16"):
        clip = CLIPViTFM("tiny", state_dict=csd, device=cuda, precision=p)
        out[p] = (clip, hsam.Sam(ssd, weights.SAM_CONFIGS["tiny"], cuda, precision=p), G.create_gem_model("tiny", clip=clip))
    return out


def _bits(t):
    """float tensors as their bit patterns: an empty mask's stability score is 0 / 0, and a NaN equals no NaN"""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _tiny_outputs(cuda, models):
    """every output of the three tiny models on fixed inputs, as a flat list of tensors"""
    from hybridgl_amd import gem as G
    from oracle.cases import sam_tiny_case, views_for_case
    clip, sam, gm = models
    loc, glo, masks = views_for_case(3, 64, 97, 130)
    x = (T(loc, cuda), T(glo, cuda), T(masks, cuda))
    outs = [clip(*x, masking_block=9, fusion_mode=mode) for mode in CLIP_MODES]
    tok = T(np.random.default_rng(2).integers(1, 400, (3, clip.model.context_length)).astype(np.int32), cuda)
    outs.append(clip.model.encode_text(tok))
    c = sam_tiny_case()
    emb = sam.encode(T(c["resized"], cuda))
    pts = T(np.random.default_rng(4).uniform(0.05, 0.95, (9, 2)).astype(np.float32), cuda)
    low, iou = sam.decode_points(emb, pts)
    outs += [emb, low, iou]
    outs += [t for t in sam.postprocess(low.flatten(0, 1), iou.flatten(), c["input_size"], c["orig_size"], -1e30, 0.0, 1.0)[:4]]
    gimg = T(np.random.default_rng(5).standard_normal((3, 128, 128)).astype(np.float32), cuda)
    gtxt = T(np.random.default_rng(6).standard_normal((2, 32)).astype(np.float32), cuda)
    feat = gm.image_features(gimg)
    outs += [feat, G.resize_antialias(gm.heatmap(feat, gtxt, 128), (97, 130))]
    return outs


@pytest.mark.parametrize("built", ["f16x3", "f16"])
def test_forced_precision_gives_the_f32_built_models_bits_and_leaves_nothing_behind(cuda, tiny_models, built):
    want = _tiny_outputs(cuda, tiny_models["f32"])
    own = _tiny_outputs(cuda, tiny_models[built])
    with ops.forced_precision("f32"):
        assert ops.effective_precision(built) == "f32"
        forced = _tiny_outputs(cuda, tiny_models[built])
    assert ops.effective_precision(built) == built
    again = _tiny_outputs(cuda, tiny_models[built])
    assert len(want) == len(own) == len(forced) == len(again)
    for i, (a, b) in enumerate(zip(forced, want)):
        assert torch.equal(_bits(a), _bits(b)), f"output {i}: forced f32 of a {built}-built model differs from the f32-built model"
    for i, (a, b) in enumerate(zip(again, own)):
        assert torch.equal(_bits(a), _bits(b)), f"output {i}: the {built} model does not give its own bits after the forced run"
    assert ops.split_overflow_count() == 0


@pytest.mark.parametrize("built", ["f16x3"])
def test_forced_precision_on_the_matrix_core_path_of_vit_b16(cuda, world, built):
    """the same at a width whose GEMMs and attention do take the split path (768): the split-built model's own bits differ
    from the f32-built model's, its forced ones do not"""
    from oracle.cases import views_for_case
    loc, glo, masks = views_for_case(4, 224, 160, 200)
    x = (T(loc, cuda), T(glo, cuda), T(masks, cuda))
    want = world["ok", "f32"](*x, masking_block=9, fusion_mode="G2L")
    own = world["ok", built](*x, masking_block=9, fusion_mode="G2L")
    assert not torch.equal(own, want)
    with ops.forced_precision("f32"):
        forced = world["ok", built](*x, masking_block=9, fusion_mode="G2L")
    assert torch.equal(forced, want)
    assert torch.equal(world["ok", built](*x, masking_block=9, fusion_mode="G2L"), own)
    assert ops.split_overflow_count() == 0


def test_forced_precision_nests_and_restores(cuda):
    ops.use_precision("f16x3")
    with ops.forced_precision("f32"):
        ops.use_precision("f16x3")
        assert ops._precision_now == "f32"
        with ops.forced_precision("f16"):
            ops.use_precision("f16x3")
            assert ops._precision_now == "f16"
        assert ops._precision_now == "f32"
    assert ops._precision_now == "f16x3"      # back in the mode of the entry: a bare ops.* call here runs as one before it did
    ops.use_precision("f16")
    with ops.forced_precision("f32"):
        pass
    assert ops._precision_now == "f16"
    ops.use_precision("f16x3")
    assert ops._precision_now == "f16x3"


# ---- ops.split_overflow_snapshot ------------------------------------------------------------------------------------------------

def test_snapshot_holds_all_three_counters(cuda):
    """The words sum to the blocking count after a GEMM overflow; the third word is the SAM decoder's: Sam.decode_points of the
    standard-geometry decoder (vit_b_d2: 64 x 64 image tokens, 256 channels) with 2 prompts runs i2t_prep_kernel for layer 1
    (2 prompts is the issue's count: every capacity of that route grows with the number of prompts, so the smallest count
    serves), whose guarded split meets U = v W_o^T with W_o scaled by 1e6.  The two-word peek does not see it."""
    from hybridgl_amd import sam as hsam
    ops.split_overflow_count()
    rng = np.random.default_rng(3)
    a2 = rng.standard_normal((256, 128)).astype(np.float32)
    w = (rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32)
    a2[3, 5] = 1.0e6
    a2[7, 9] = -3.0e5
    ops.gemm_f16x3(T(a2, cuda), T(w, cuda))
    buf = torch.zeros(3, dtype=torch.int32).pin_memory()
    ops.split_overflow_snapshot(buf)
    torch.cuda.synchronize()
    words = [int(v) for v in buf.tolist()]
    print("snapshot after the GEMM", words)
    assert words == [2, 0, 0]
    assert sum(words) == ops.split_overflow_count(reset=False) == 2      # no reset by the snapshot
    assert ops.split_overflow_count() == 2

    sd = {k: np.array(v, copy=True) for k, v in weights.sam_state_dict("vit_b_d2", 0).items()}
    sd["mask_decoder.transformer.layers.1.cross_attn_image_to_token.out_proj.weight"] *= np.float32(1.0e6)
    m = hsam.Sam(sd, weights.SAM_CONFIGS["vit_b_d2"], cuda, precision="f16x3")
    emb = T(np.random.default_rng(8).standard_normal((4096, 256)).astype(np.float32), cuda)
    pts = T(np.array([[0.3, 0.4], [0.7, 0.2]], dtype=np.float32), cuda)
    m.decode_points(emb, pts)
    two = torch.zeros(2, dtype=torch.int32).pin_memory()
    ops.split_overflow_snapshot(buf)
    ops.split_overflow_peek(two)
    torch.cuda.synchronize()
    words = [int(v) for v in buf.tolist()]
    print("snapshot after the decoder", words, "peek", two.tolist())
    assert words[2] > 0
    assert [int(v) for v in two.tolist()] == words[:2]
    assert sum(words) == ops.split_overflow_count(reset=False)
    assert ops.split_overflow_count() == sum(words) and ops.split_overflow_count() == 0


# ---- the option --------------------------------------------------------------------------------------------------------------

def test_option_validation_and_f32_models_make_rescue_a_no_op(cuda, world):
    from hybridgl_amd.pipeline import HybridGLPipeline
    with pytest.raises(ValueError, match="on_overflow"):
        HybridGLPipeline(world["ok", "f32"], on_overflow="nonsense")
    assert HybridGLPipeline(world["ok", "f32"]).on_overflow == "raise"
    pipe = HybridGLPipeline(world["bad", "f32"], mask_generator=world["gen", "f32"], use_sam_masks=True, on_overflow="rescue")
    assert pipe._rescue_wanted() is False
    assert pipe.run(iter(world["refs"][:4]), group=2, proposal_cap=4, collect=True) == 4
    assert pipe.rescue_stats == {"events": 0, "groups": 0, "refs": 0, "positions": []}
    pipe.metrics()
    # the default mode still raises at the offending group, with the message it had
    bad = HybridGLPipeline(world["bad", "f16x3"], mask_generator=world["gen", "f16x3"], use_sam_masks=True)
    with pytest.raises(ops.SplitOverflow, match="rerun with HYBRIDGL_PRECISION=f32"):
        bad.run(iter(world["refs"][:10]), group=2, proposal_cap=4, serial=True)
    torch.cuda.synchronize()
    assert ops.split_overflow_count() == 0
