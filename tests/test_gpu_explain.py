"""HybridGL(explain=True) on the GPU, with the tiny models as tests/test_gpu_demo.py builds them: what a Segmentation's Explanation
holds against what the tail computes from it -- gem_score is ops.coherence_scores of the kept heat-map bit for bit, index_pure is
the argmax of score_clip, index_final lies in its top k1 -- heat_overlay against the numpy contract (tests/heat_cases.py) on the
read-back map, topk_overlay's order, the flag off, the per-sentence tail in a fresh child process, and the CLI's three outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heat_cases as HC
import paint_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTENCES = ["the cat on left", "a big dog"]
PARSE = [{"noun_phrase": "the cat", "other_nouns": ["left"], "dirflag": "left", "relaflag": "none"},
         {"noun_phrase": "dog", "other_nouns": [], "dirflag": "none", "relaflag": "big"}]
# the filters open and the box NMS off (nothing has IoU > 1): the tiny SAM's noise masks all have image-sized boxes
AMG = dict(points_per_side=4, pred_iou_thresh=-1.0, stability_score_thresh=0.0, min_mask_region_area=20, box_nms_thresh=1.0)
AMG_FLAGS = ["--points_per_side", "4", "--pred_iou_thresh", "-1", "--stability_score_thresh", "0", "--min_mask_region_area", "20",
             "--box_nms_thresh", "1"]


@pytest.fixture(scope="module")
def image_path(tmp_path_factory):
    from PIL import Image
    from hybridgl_amd.synth import synth_image
    path = tmp_path_factory.mktemp("explain") / "image.png"
    Image.fromarray(synth_image(120, 163, 50)).save(path)
    return str(path)


@pytest.fixture(scope="module")
def vocab(golden_dir):
    return os.path.join(golden_dir, "tiny_bpe_vocab.txt.gz")


@pytest.fixture(scope="module")
def hgl(cuda, vocab):
    from hybridgl_amd.demo import HybridGL
    return HybridGL(sam_model="tiny", bpe_vocab=vocab, amg=AMG, device=cuda, explain=True)


@pytest.fixture(scope="module")
def segs(hgl, image_path):
    return hgl.segment(image_path, SENTENCES, PARSE)


def test_the_explanation_is_what_the_tail_computed(cuda, hgl, segs):
    from hybridgl_amd import ops
    from hybridgl_amd.pipeline import black_for
    for s, rec in zip(segs, PARSE):
        ex = s.explanation
        N, H, W = s.proposals.shape
        assert ex.dirflag == rec["dirflag"] and ex.black == black_for(rec["relaflag"])
        assert ex.heat.shape == (H, W) and ex.heat.dtype == torch.float32 and ex.heat.is_cuda
        assert all(t.shape == (N,) and t.dtype == torch.float32 and t.is_cuda for t in (ex.score_clip, ex.score_neg, ex.gem_score))
        again = ops.coherence_scores(ex.heat.contiguous(), s.proposals, ex.dirflag, ex.black)
        assert torch.equal(again.view(torch.int32), ex.gem_score.view(torch.int32))      # bit for bit
        assert int(torch.argmax(ex.score_clip)) == s.index_pure
        k1 = min(hgl._pipe._k0[0], N)
        top = torch.argsort(ex.score_clip, descending=True, stable=True)[:k1].tolist()
        assert s.index_final in top
    assert not torch.equal(segs[0].explanation.heat, segs[1].explanation.heat)      # a map per noun phrase


def test_heat_overlay_is_the_contract_on_the_read_back_map(cuda, segs):
    from hybridgl_amd import render
    for s in segs:
        ex = s.explanation
        x = ex.heat.cpu().numpy()
        image = s.image.cpu().numpy()
        H, W = x.shape
        call = dict(heat=x.reshape(-1), maps=np.array([[H, W, HC.DIRS.index(ex.dirflag), 0, 0, 0]]), ramp=render.ramp("heat"),
                    base=image.reshape(-1, 3), canvas=H * W)
        want, _, status = HC.expect(call)
        assert status[0, 0] == 0
        got, g_status = s.heat_overlay(outline=False, with_status=True)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want.reshape(H, W, 3)) and np.array_equal(g_status.cpu().numpy(), status)
        # the outline: the edge of the final winner in the ink, every other pixel as without it
        lined = s.heat_overlay().cpu().numpy()
        edge = PC.edge_of(s.mask("final").cpu().numpy())
        assert edge.any() and np.all(lined[edge] == 255) and np.array_equal(lined[~edge], want.reshape(H, W, 3)[~edge])
        grey = s.heat_overlay(ramp="grey", outline=False).cpu().numpy()
        assert np.array_equal(grey[..., 0], HC.levels_of(x, HC.DIRS.index(ex.dirflag))[4])


def test_topk_overlay_paints_the_stable_descending_order_best_last(cuda, segs):
    from hybridgl_amd import render
    s = segs[0]
    sc = s.explanation.score_clip.cpu().numpy()
    N = len(sc)
    for k in (1, 3, N + 5):
        kk = min(k, N)
        order = sorted(range(N), key=lambda i: (-sc[i], i))[:kk][::-1]      # best last
        assert s.topk_order(k).tolist() == order and (k < 1 or order[-1] == s.index_pure)
        masks = s.proposals.cpu().numpy()
        H, W = masks.shape[1:]
        need = max(len(PC.counts_of(m)) for m in masks)
        slots, table = PC.encode_set(list(masks), need, [0] * N)
        want = np.zeros((H * W, 3), np.uint8)
        PC.paint(slots, table, [[H, W, 0, 0, 0]], np.asarray(order, np.int32), render.proposal_styles(kk)[::-1].copy(),
                 s.image.cpu().numpy().reshape(-1, 3), want, None, np.zeros((kk, 4), np.int32))
        assert np.array_equal(s.topk_overlay(k).cpu().numpy(), want.reshape(H, W, 3))


def test_the_flag_off_keeps_nothing_and_chooses_the_same(cuda, hgl, segs, image_path):
    from hybridgl_amd.pipeline import HybridGLPipeline
    pipe = HybridGLPipeline(hgl.model, mask_generator=hgl.generator, use_sam_masks=True, gem_model=hgl.gem_model, k_clamp="per_ref")
    assert pipe.keep_explain is False
    pipe.step(hgl.ref_batch(image_path, SENTENCES, PARSE))
    assert pipe.explained() == []
    assert [tuple(int(v) for v in w) for w in pipe.winning_indices()] == [(s.index_pure, s.index_final) for s in segs]
    kept = hgl._pipe.explained()
    assert [(e["index"] is not None, e["sentence"]) for e in kept] == [(True, 0), (True, 1)]
    # without the flag a Segmentation carries none and says so
    import dataclasses
    bare = dataclasses.replace(segs[0], explanation=None)
    with pytest.raises(RuntimeError):
        bare.heat_overlay()


def test_run_keeps_the_sentences_of_the_group(cuda, hgl, image_path):
    import dataclasses
    from hybridgl_amd.pipeline import HybridGLPipeline
    pipe = HybridGLPipeline(hgl.model, mask_generator=hgl.generator, use_sam_masks=True, gem_model=hgl.gem_model, k_clamp="per_ref",
                            keep_explain=True)
    refs = [dataclasses.replace(hgl.ref_batch(image_path, SENTENCES, PARSE), index=0),
            dataclasses.replace(hgl.ref_batch(image_path, SENTENCES[1], PARSE[1]), index=1)]
    assert pipe.run(refs) == 2
    kept = pipe.explained()
    assert [(e["index"], e["sentence"]) for e in kept] == [(0, 0), (0, 1), (1, 0)] == [tuple(o) for o in pipe.iu_owner]
    assert [e["dirflag"] for e in kept] == ["left", "none", "none"] and [e["black"] for e in kept] == [1.8, 1.95, 1.95]
    win = pipe.winning_indices()
    for e, w in zip(kept, win):
        assert e["heat"].shape == tuple(refs[0].sam_img.shape[:2]) and e["score_clip"].shape == e["gem_score"].shape == e["score_neg"].shape
        assert int(torch.argmax(e["score_clip"])) == int(w[0])
    # the next group starts afresh
    assert pipe.run(refs[1:]) == 1 and [(e["index"], e["sentence"]) for e in pipe.explained()] == [(1, 0)]


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import torch
from hybridgl_amd.demo import HybridGL
hgl = HybridGL(sam_model="tiny", bpe_vocab=sys.argv[3], amg=%r, device=torch.device("cuda:0"), explain=True)
assert hgl._pipe.fused_tail is False
segs = hgl.segment(sys.argv[4], %r, %r)
out = {}
for j, s in enumerate(segs):
    ex = s.explanation
    out.update({f"idx{j}": np.array([s.index_pure, s.index_final]), f"heat{j}": ex.heat.cpu().numpy(), f"black{j}": np.array(ex.black),
                f"sc{j}": ex.score_clip.cpu().numpy(), f"sn{j}": ex.score_neg.cpu().numpy(), f"gm{j}": ex.gem_score.cpu().numpy()})
    out[f"dir{j}"] = np.array(ex.dirflag)
np.savez(sys.argv[1], **out)
""" % (AMG, SENTENCES, PARSE)


def test_the_per_sentence_tail_fills_the_same_values(cuda, hgl, segs, image_path, vocab, tmp_path):
    assert hgl._pipe.fused_tail is True
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, out, ROOT, vocab, image_path], env=dict(os.environ, HYBRIDGL_FUSED_TAIL="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    g = np.load(out)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    for j, s in enumerate(segs):
        ex = s.explanation
        assert g[f"idx{j}"].tolist() == [s.index_pure, s.index_final] and str(g[f"dir{j}"]) == ex.dirflag and float(g[f"black{j}"]) == ex.black
        assert same(g[f"heat{j}"], ex.heat.cpu().numpy())
        for name, t in (("sc", ex.score_clip), ("sn", ex.score_neg), ("gm", ex.gem_score)):
            assert same(g[name + str(j)], t.cpu().numpy()), (j, name)


def test_the_cli_writes_both_pictures_and_the_scores(cuda, segs, image_path, vocab, tmp_path, capsys):
    from PIL import Image
    from hybridgl_amd import demo
    out, heat, topk, scores = (tmp_path / n for n in ("result.png", "heat.png", "topk.png", "scores.json"))
    rec = tmp_path / "parse.json"
    json.dump({SENTENCES[0]: PARSE[0], SENTENCES[1]: PARSE[1]}, open(rec, "w"))
    rc = demo.main(["--image", image_path, "--text", SENTENCES[0], "--out", str(out), "--parse_json", str(rec), "--heat_out", str(heat),
                    "--topk_out", str(topk), "--topk", "2", "--scores_json", str(scores), "--sam_model", "tiny", "--bpe_vocab", vocab] + AMG_FLAGS)
    s = segs[0]
    assert rc == 0 and f"proposal {s.index_final} of {s.n_proposals}" in capsys.readouterr().out
    assert np.array_equal(np.array(Image.open(heat)), s.heat_overlay().cpu().numpy())
    assert np.array_equal(np.array(Image.open(topk)), s.topk_overlay(2).cpu().numpy())
    doc = json.load(open(scores))
    assert len(doc) == 1 and doc[0]["text"] == SENTENCES[0]
    assert (doc[0]["index_pure"], doc[0]["index_final"]) == (s.index_pure, s.index_final)
    ex = s.explanation
    for name, t in (("score_clip", ex.score_clip), ("score_neg", ex.score_neg), ("gem_score", ex.gem_score)):
        assert np.array_equal(np.asarray(doc[0][name], np.float32), t.cpu().numpy(), equal_nan=True), name      # a full-image mask has no outside
    x = ex.heat.cpu().numpy()
    _, mn, mx, peak, _ = HC.levels_of(x, HC.DIRS.index(ex.dirflag))
    assert doc[0]["status"] == {"code": 0, "mn": float(mn), "mx": float(mx), "peak": float(peak)}
