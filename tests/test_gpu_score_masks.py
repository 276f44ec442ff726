"""Saved predictions scored and compared offline: `main.py --score_masks DIR` (no model, no checkpoint: the files and the
dataset's ground truth through ops.rle_iou) reproduces the metrics and the rows of the run that wrote DIR, reports a tampered
record, and predictions.compare meets two saved sets mask by mask."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hybridgl_amd import refer_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--synthetic", "3", "--proposals", "6", "--heatmap", "given", "--group", "2", "--workers", "1"]


@pytest.fixture(scope="module")
def model(cuda):
    from hybridgl_amd.backbone import CLIPViTFM
    return CLIPViTFM("ViT-B/16", seed=0, device=cuda)


@pytest.fixture(scope="module")
def saved(cuda, model, tmp_path_factory):
    """one run with --save_masks: (directory, its metrics, its lines); and a copy with one `final` string replaced by that of
    another record of the same size whose string differs: (directory, key, the two strings)"""
    from hybridgl_amd import main as drv
    base = tmp_path_factory.mktemp("score")
    out = base / "out"
    args = drv.default_argument_parser().parse_args(FLAGS + ["--save_masks", str(out), "--result_dir", str(base / "log")])
    m, _ = drv.evaluate(args, model, None, None, cuda)
    lines = [json.loads(s) for s in open(out / "masks.rank0.jsonl")]
    assert len(lines) == 9
    pair = next((i, j) for i in range(9) for j in range(9)
                if lines[i]["size"] == lines[j]["size"] and lines[i]["final"] != lines[j]["final"])
    tampered = base / "tampered"
    tampered.mkdir()
    changed = [dict(r) for r in lines]
    changed[pair[0]]["final"] = lines[pair[1]]["final"]
    with open(tampered / "masks.rank0.jsonl", "w") as f:
        for r in changed:
            f.write(json.dumps(r) + "\n")
    key = (lines[pair[0]]["index"], lines[pair[0]]["sentence"])
    return {"out": out, "metrics": m, "lines": lines, "tampered": tampered, "key": key,
            "strings": (lines[pair[0]]["final"], lines[pair[1]]["final"]), "base": base}


def score_args(directory, base):
    from hybridgl_amd import main as drv
    return drv.default_argument_parser().parse_args(FLAGS + ["--score_masks", str(directory), "--result_dir", str(base / "log")])


def test_score_masks_reproduces_the_run(cuda, saved):
    """no model anywhere in the call; metrics, rows and report equal the run's"""
    from hybridgl_amd import main as drv
    m, rep = drv.score_masks(score_args(saved["out"], saved["base"]), cuda)
    assert set(m) == set(saved["metrics"])
    for k in m:
        assert m[k] == saved["metrics"][k], k
    want = sorted([r["index"], r["sentence"], r["I"], r["U"], r["I_final"], r["U_final"]] for r in saved["lines"])
    assert rep["rows"].dtype == np.int64 and rep["rows"].tolist() == want and len(want) == 9
    assert rep["mismatches"] == [] and rep["missing"] == [] and rep["extra"] == []


def test_score_masks_reports_a_tampered_record(cuda, saved):
    from hybridgl_amd import main as drv
    m, rep = drv.score_masks(score_args(saved["tampered"], saved["base"]), cuda)
    assert rep["mismatches"] == [saved["key"]] and rep["missing"] == [] and rep["extra"] == []
    # the recomputed row is the truth about the mask that the file now holds
    from hybridgl_amd.pipeline import synthetic_ref
    gt = synthetic_ref(saved["key"][0], cuda, N=6, device_blur=True)[1]["gt"].astype(bool)
    size = saved["lines"][0]["size"]
    pred = refer_io.gt_mask_from_rle({"size": size, "counts": saved["strings"][1]})[0].astype(bool)
    row = next(r for r in rep["rows"].tolist() if (r[0], r[1]) == saved["key"])
    assert row[4:6] == [int((pred & gt).sum()), int((pred | gt).sum())]


def test_score_masks_reports_missing_and_extra_records(cuda, saved, tmp_path):
    from hybridgl_amd import main as drv
    recs = [dict(r) for r in saved["lines"]]
    gone = recs.pop(4)
    recs.append(dict(recs[0], index=7, sentence=1))
    with open(tmp_path / "masks.rank0.jsonl", "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    m, rep = drv.score_masks(score_args(tmp_path, saved["base"]), cuda)
    assert rep["missing"] == [(gone["index"], gone["sentence"])] and rep["extra"] == [(7, 1)] and rep["mismatches"] == []
    assert len(rep["rows"]) == 8 and m["n_sentences"] == 8


def test_module_entry_point_exit_status(saved):
    """python -m hybridgl_amd.main --score_masks on the tampered copy, in a fresh child process: the report is written, the key is
    named and the exit status is non-zero"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "hybridgl_amd.main"] + FLAGS + ["--score_masks", str(saved["tampered"]),
                                                                 "--result_dir", str(saved["base"] / "log_child")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "pure hybridgl:" in r.stdout
    assert f"stored counts differ from the recomputed ones: index {saved['key'][0]} sentence {saved['key'][1]}" in r.stdout
    log = (saved["base"] / "log_child" / "result_log_refcoco_val.txt").read_text()
    assert log.count("Overall IoU / mean IoU") == 1


def test_compare(cuda, saved, tmp_path):
    from hybridgl_amd import predictions as P
    same = P.compare(saved["out"], saved["out"])
    s = same["summary"]
    assert s["n_common"] == 9 and s["only_in_a"] == [] and s["only_in_b"] == []
    assert s["identical_pure"] == 9 and s["identical_final"] == 9 and s["min_iou_pure"] == 1.0 and s["min_iou_final"] == 1.0
    assert s["differ_pure"] == [] and s["differ_final"] == []
    for r in saved["lines"]:
        area = {k: int(refer_io.gt_mask_from_rle({"size": r["size"], "counts": r[k]})[0].sum()) for k in ("pure", "final")}
        assert same["per_key"][(r["index"], r["sentence"])] == {k: (area[k], area[k]) for k in area}
    diff = P.compare(P.load(saved["out"]), P.load(saved["tampered"]))
    s = diff["summary"]
    assert s["identical_pure"] == 9 and s["identical_final"] == 8 and s["differ_final"] == [saved["key"]] and s["differ_pure"] == []
    size = saved["lines"][0]["size"]
    a, b = (refer_io.gt_mask_from_rle({"size": size, "counts": c})[0].astype(bool) for c in saved["strings"])
    assert diff["per_key"][saved["key"]]["final"] == (int((a & b).sum()), int((a | b).sum()))
    assert s["min_iou_final"] == (a & b).sum() / (a | b).sum() and s["min_iou_pure"] == 1.0
    # one record removed from the second set
    recs = [r for r in saved["lines"] if (r["index"], r["sentence"]) != saved["key"]]
    with open(tmp_path / "masks.rank0.jsonl", "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    less = P.compare(saved["out"], tmp_path)["summary"]
    assert less["only_in_a"] == [saved["key"]] and less["only_in_b"] == [] and less["n_common"] == 8 and less["identical_final"] == 8


def test_compare_command(saved, tmp_path):
    """python -m hybridgl_amd.predictions compare: exit 0 when the command ran (differences included), non-zero on unreadable input"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out_json = tmp_path / "cmp.json"
    r = subprocess.run([sys.executable, "-m", "hybridgl_amd.predictions", "compare", str(saved["out"]), str(saved["tampered"]),
                        "--json", str(out_json)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "final: identical 8" in r.stdout and "pure: identical 9" in r.stdout
    rep = json.load(open(out_json))
    assert rep["summary"]["differ_final"] == [list(saved["key"])] and len(rep["per_key"]) == 9
    r = subprocess.run([sys.executable, "-m", "hybridgl_amd.predictions", "compare", str(saved["out"]), str(tmp_path / "none")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode != 0 and "masks.rank" in r.stderr
