"""Saved runs voted into one prediction: predictions.ensemble (ops.rle_merge on the strings' runs) against the numpy vote, mask
for mask, and `main.py --ensemble_masks DIR DIR DIR --ensemble_out OUT` -- no model anywhere: three record directories are
written by the test from seeded shapes at the sizes of the `--synthetic 3` refs, the branch writes OUT, and --score_masks on OUT
finds nothing to complain about and reports the metrics the branch printed."""
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


def parse(extra, base):
    from hybridgl_amd import main as drv
    return drv.default_argument_parser().parse_args(FLAGS + list(extra) + ["--result_dir", str(base / "log")])


def shape(H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx, ry, rx = rng.random() * H, rng.random() * W, (0.1 + 0.4 * rng.random()) * H, (0.1 + 0.4 * rng.random()) * W
    m = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1)
    return (m ^ (rng.random((H, W)) < 0.02)).astype(np.uint8)      # speckled: runs in plenty


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    """three directories of seeded records over the keys and sizes of the synthetic refs; the dense masks beside them"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import predictions as P
    from hybridgl_amd import sam as hsam
    base = tmp_path_factory.mktemp("ensemble")
    args = parse([], base)
    drv.resolve_defaults(args)
    targets = {key: t for key, _, t in drv.offline_targets(args, cuda)}
    keys = sorted(targets)
    assert len(keys) == 9
    rng = np.random.default_rng(77)
    dirs, dense = [], []
    for r in range(3):
        recs, d = [], {}
        for k in keys:
            H, W = (int(v) for v in targets[k].shape[-2:])
            d[k] = {m: shape(H, W, rng) for m in P.MASKS}
            enc = lambda mask: hsam.coco_encode_rle(hsam.mask_to_rle(mask))["counts"]
            recs.append({"index": k[0], "sentence": k[1], "size": [H, W], "pure": enc(d[k]["pure"]), "final": enc(d[k]["final"]),
                         "I": 0, "U": 0, "I_final": 0, "U_final": 0})
        P.save(recs, base / f"run{r}")
        dirs.append(base / f"run{r}")
        dense.append(d)
    return {"base": base, "dirs": dirs, "dense": dense, "keys": keys, "targets": targets}


def decode(rec, m):
    return refer_io.gt_mask_from_rle({"size": rec["size"], "counts": rec[m]})[0].astype(np.uint8)


@pytest.mark.parametrize("rule,weights", [("majority", None), ("union", None), ("intersect", None), ("majority", [2, 1, 1]),
                                          ("at_least:3", [2, 1, 1]), ("exactly:1", None)])
def test_ensemble_equals_the_numpy_vote(cuda, runs, rule, weights):
    from hybridgl_amd import ops
    from hybridgl_amd import predictions as P
    out = P.ensemble(runs["dirs"], rule=rule, weights=weights, device=cuda)
    assert [(r["index"], r["sentence"]) for r in out] == runs["keys"]
    w = weights or [1, 1, 1]
    lo, hi = ops.rle_merge_rule(rule, sum(w))
    for rec in out:
        k = (rec["index"], rec["sentence"])
        assert sorted(rec) == ["final", "index", "pure", "sentence", "size"]
        for m in P.MASKS:
            count = sum(wi * runs["dense"][i][k][m].astype(np.int64) for i, wi in enumerate(w))
            want = ((count >= lo) & (count <= hi)).astype(np.uint8)
            assert (decode(rec, m) == want).all(), (k, m)


def test_a_run_voted_with_itself_is_itself(cuda, runs):
    from hybridgl_amd import predictions as P
    a = P.load(runs["dirs"][0])
    for sets, rule in (([a, a, a], "majority"), ([a, a], "union"), ([a, a], "intersect")):
        out = P.ensemble(sets, rule=rule, device=cuda)
        for rec, src in zip(out, a):
            assert (rec["index"], rec["sentence"], rec["size"]) == (src["index"], src["sentence"], src["size"])
            assert rec["pure"] == src["pure"] and rec["final"] == src["final"]      # the strings, byte for byte


def test_sets_that_are_not_one_run_are_refused(cuda, runs):
    from hybridgl_amd import predictions as P
    a, b = P.load(runs["dirs"][0]), P.load(runs["dirs"][1])
    with pytest.raises(ValueError, match="do not hold the same keys"):
        P.ensemble([a, b[:-1]], device=cuda)
    with pytest.raises(ValueError, match="do not hold the same keys"):
        P.ensemble([a, b[:-1] + [dict(b[-1], index=99)]], device=cuda)
    odd = [dict(r) for r in b]
    odd[4]["size"] = [odd[4]["size"][0] + 1, odd[4]["size"][1]]
    with pytest.raises(ValueError, match=f"index {odd[4]['index']} sentence {odd[4]['sentence']} has size"):
        P.ensemble([a, odd], device=cuda)
    with pytest.raises(ValueError, match="at least two"):
        P.ensemble([a], device=cuda)
    with pytest.raises(ValueError, match="weights"):
        P.ensemble([a, b], weights=[1], device=cuda)
    with pytest.raises(ValueError, match="weights"):
        P.ensemble([a, b], weights=[1, -1], device=cuda)
    with pytest.raises(ValueError, match="rule"):
        P.ensemble([a, b], rule="most", device=cuda)


def test_the_branch_writes_what_score_masks_confirms(cuda, runs, capsys):
    from hybridgl_amd import main as drv
    from hybridgl_amd import predictions as P
    out = runs["base"] / "voted"
    dirs = [str(d) for d in runs["dirs"]]
    m = drv.ensemble_masks_main(parse(["--ensemble_masks"] + dirs + ["--ensemble_rule", "majority", "--ensemble_out", str(out)],
                                      runs["base"]), cuda)
    said = capsys.readouterr().out
    assert "ensemble of 3 saved runs by majority" in said and all(d in said for d in dirs) and "pure hybridgl:" in said
    recs = P.load(out)
    assert [(r["index"], r["sentence"]) for r in recs] == runs["keys"]
    want = P.ensemble(runs["dirs"], rule="majority", device=cuda)
    for rec, w in zip(recs, want):
        assert rec["pure"] == w["pure"] and rec["final"] == w["final"]
        gt = runs["targets"][(rec["index"], rec["sentence"])].cpu().numpy().astype(bool)
        for m_, (i, u) in (("pure", ("I", "U")), ("final", ("I_final", "U_final"))):
            p = decode(rec, m_).astype(bool)
            assert (rec[i], rec[u]) == (int((p & gt).sum()), int((p | gt).sum()))
    m2, rep = drv.score_masks(parse(["--score_masks", str(out)], runs["base"]), cuda)
    assert rep["mismatches"] == [] and rep["missing"] == [] and rep["extra"] == [] and len(rep["rows"]) == 9
    assert set(m2) == set(m)
    for k in m:
        assert m2[k] == m[k], k
    # weights ride along
    out_w = runs["base"] / "voted_w"
    drv.ensemble_masks_main(parse(["--ensemble_masks"] + dirs + ["--ensemble_weights", "2", "1", "1", "--ensemble_out", str(out_w)],
                                  runs["base"]), cuda)
    assert "with weights 2 1 1" in capsys.readouterr().out
    for rec, w in zip(P.load(out_w), P.ensemble(runs["dirs"], weights=[2, 1, 1], device=cuda)):
        assert rec["pure"] == w["pure"] and rec["final"] == w["final"]


def test_the_four_cli_refusals(cuda, runs):
    from hybridgl_amd import main as drv
    a, b = str(runs["dirs"][0]), str(runs["dirs"][1])
    out = str(runs["base"] / "never")
    for extra, why in [(["--ensemble_masks", a, "--ensemble_out", out], "two or more directories"),
                       (["--ensemble_masks", a, b, "--ensemble_weights", "1", "2", "3", "--ensemble_out", out], "one weight per directory"),
                       (["--ensemble_masks", a, b, "--score_masks", a, "--ensemble_out", out], "does not combine with --score_masks"),
                       (["--ensemble_masks", a, b, "--proposal_ceiling", "c.json", "--ensemble_out", out], "does not combine"),
                       (["--ensemble_masks", a, b], "needs --ensemble_out")]:
        with pytest.raises(SystemExit) as e:
            drv.main(parse(extra, runs["base"]))
        assert why in str(e.value), (extra, str(e.value))
    assert not os.path.exists(out)
    # sets that are not one run: the branch names the reason and exits
    short = runs["base"] / "short"
    short.mkdir()
    lines = open(runs["dirs"][1] / "masks.rank0.jsonl").read().splitlines()
    (short / "masks.rank0.jsonl").write_text("\n".join(lines[:-1]) + "\n")
    with pytest.raises(SystemExit) as e:
        drv.main(parse(["--ensemble_masks", a, str(short), "--ensemble_out", out], runs["base"]))
    assert "do not hold the same keys" in str(e.value)


def test_module_entry_point_exit_status(runs):
    """python -m hybridgl_amd.main --ensemble_masks ... in a fresh child process: exit 0, OUT written, the line printed"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = runs["base"] / "voted_child"
    cmd = [sys.executable, "-m", "hybridgl_amd.main"] + FLAGS + ["--ensemble_masks"] + [str(d) for d in runs["dirs"]] + \
        ["--ensemble_rule", "union", "--ensemble_out", str(out), "--result_dir", str(runs["base"] / "log_child")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "ensemble of 3 saved runs by union" in r.stdout and "pure hybridgl:" in r.stdout
    lines = [json.loads(s) for s in open(out / "masks.rank0.jsonl")]
    assert len(lines) == 9 and sorted(lines[0]) == sorted(["index", "sentence", "size", "pure", "final", "I", "U", "I_final", "U_final"])
    log = (runs["base"] / "log_child" / "result_log_refcoco_val.txt").read_text()
    assert log.count("Overall IoU / mean IoU") == 1
