"""The evaluator's winning masks as predictions: HybridGLPipeline(record_predictions=True) / predictions() on every tail
path of step() and run(), and the driver's --save_masks file -- against the host codec on the refs' own masks and against
the metric rows the same run produced."""
import json

import numpy as np
import pytest
import torch

from hybridgl_amd import sam as hsam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(cuda):
    from hybridgl_amd.backbone import CLIPViTFM
    return CLIPViTFM("ViT-B/16", seed=0, device=cuda)


@pytest.fixture(scope="module")
def world(cuda, model):
    """five refs with 6 .. 10 proposals of 120 x 160, scored ref by ref with the option on: (refs, pipeline, predictions)"""
    from hybridgl_amd.pipeline import HybridGLPipeline, synthetic_ref
    refs = [synthetic_ref(i, cuda, N=6 + i, H=120, W=160)[0] for i in range(5)]
    a = HybridGLPipeline(model, record_predictions=True)
    for r in refs:
        a.step(r)
    return refs, a, a.predictions()


def test_step_and_run_record_the_same_predictions(cuda, model, world):
    from hybridgl_amd.pipeline import HybridGLPipeline
    refs, a, want = world
    assert len(want) == 15 and [(p["index"], p["sentence"]) for p in want] == [(i, j) for i in range(5) for j in range(3)]
    b = HybridGLPipeline(model, record_predictions=True)
    assert b.run(iter(refs), group=4) == 5
    assert b.predictions() == want
    assert b.predictions() == want      # asking twice changes nothing
    # the other tail paths: one hgl_score_ref per ref inside run(), and the per-sentence launches
    c = HybridGLPipeline(model, record_predictions=True)
    c.group_tail = False
    c.run(iter(refs), group=4)
    assert c.predictions() == want
    d = HybridGLPipeline(model, record_predictions=True)
    d.fused_tail = False
    for r in refs:
        d.step(r)
    assert d.predictions() == want
    e = HybridGLPipeline(model, record_predictions=True)
    e.fused_tail = False
    e.run(iter(refs), group=2)
    assert e.predictions() == want
    for p in (b, c, d, e):
        assert np.array_equal(p.partial_rows(), a.partial_rows())


def test_predictions_are_the_winning_masks(cuda, world):
    refs, a, preds = world
    win = a.winning_indices()
    rows = a.partial_rows()
    assert len(preds) == len(win) == len(rows)
    for p, w, row in zip(preds, win, rows):
        assert (p["index"], p["sentence"], p["pure_index"], p["final_index"]) == (int(row[0]), int(row[1]), int(w[0]), int(w[1]))
        ref = refs[p["index"]]
        masks = ref.masks.cpu().numpy()
        assert p["size"] == [120, 160]
        assert p["pure"] == hsam.mask_to_rle(masks[w[0]])["counts"]
        assert p["final"] == hsam.mask_to_rle(masks[w[1]])["counts"]
        # the IoU counts of the metric row, recomputed from the decoded runs
        target = ref.target.cpu().numpy().astype(bool)
        got = []
        for key in ("pure", "final"):
            m = hsam.rle_to_mask({"size": p["size"], "counts": p[key]})
            got += [int((m & target).sum()), int((m | target).sum())]
        assert got == [int(v) for v in row[2:6]]


def test_the_option_changes_no_metric_row_and_is_off_by_default(cuda, model, world):
    from hybridgl_amd.pipeline import HybridGLPipeline
    refs, a, _ = world
    off = HybridGLPipeline(model)
    off.run(iter(refs), group=4)
    assert np.array_equal(off.partial_rows(), a.partial_rows())
    assert np.array_equal(off.winning_indices(), a.winning_indices())
    assert not off._pred_pending and not off._pred_done and not off._pred_free
    with pytest.raises(RuntimeError, match="record_predictions"):
        off.predictions()


def test_prepare_keeps_the_records_and_the_staging_buffers(cuda, model, world):
    """prepare() rehearses the loop with the option on: its own records are dropped, the pinned buffers stay for the run"""
    from hybridgl_amd.pipeline import HybridGLPipeline
    refs, a, want = world
    p = HybridGLPipeline(model, record_predictions=True)
    p.step(refs[0])
    p.prepare(group=2, H=120, W=160, proposals=8, slack=0)
    assert len(p._pred_free) >= 1 and not p._pred_pending
    pool = {b.data_ptr() for b in p._pred_free}
    p.run(iter(refs[1:]), group=2)
    assert p.predictions() == want
    assert {b.data_ptr() for b in p._pred_free} >= pool


def test_driver_save_masks(cuda, model, tmp_path):
    """--save_masks: one line per sentence; every string decodes to a mask of the stated size whose IoU counts against the
    ref's target are the metric row's"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import refer_io
    from hybridgl_amd.pipeline import synthetic_ref
    out = tmp_path / "out"
    args = drv.default_argument_parser().parse_args(["--synthetic", "3", "--proposals", "6", "--heatmap", "given", "--group", "2",
                                                     "--workers", "1", "--save_masks", str(out)])
    drv.evaluate(args, model, None, None, cuda)
    lines = [json.loads(s) for s in open(out / "masks.rank0.jsonl")]
    assert sorted((r["index"], r["sentence"]) for r in lines) == [(i, j) for i in range(3) for j in range(3)]
    targets = {i: synthetic_ref(i, cuda, N=6, device_blur=True)[1]["gt"].astype(bool) for i in range(3)}
    for r in lines:
        assert set(r) == {"index", "sentence", "size", "pure", "final", "I", "U", "I_final", "U_final"}
        assert r["size"] == [640, 640]
        got = []
        for key in ("pure", "final"):
            assert isinstance(r[key], str)
            m, area = refer_io.gt_mask_from_rle({"size": r["size"], "counts": r[key]})
            assert m.shape == (640, 640) and int(m.sum()) == area and m.max() <= 1
            got += [int((m.astype(bool) & targets[r["index"]]).sum()), int((m.astype(bool) | targets[r["index"]]).sum())]
        assert got == [r["I"], r["U"], r["I_final"], r["U_final"]]
