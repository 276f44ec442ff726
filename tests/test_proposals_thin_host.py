"""proposals.thin and its command line without a device: the refusals (dst == src, an occupied dst, an unknown score or metric, a
record that does not decode), the meta it writes, the records it keeps -- unchanged and in their stored order -- and what it hands
to ops.rle_nms, which a fake stands in for here (tests/test_gpu_proposals_thin.py runs the real one).  The refusals that
proposals.clean shares with it, and clean's own, run here too: they come before any device call."""
import json
import os

import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import proposals as P
from hybridgl_amd import sam as hsam


def record(H, W, y0, y1, x0, x1, iou, stab):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    seg = hsam.coco_encode_rle(hsam.mask_to_rle(m))
    return {"segmentation": seg, "area": int(m.sum()), "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": iou,
            "point_coords": [[float(x0), float(y0)]], "stability_score": stab, "crop_box": [0, 0, W, H]}


@pytest.fixture()
def src(tmp_path):
    store = P.ProposalStore(tmp_path / "src")
    store.write(3, [record(20, 30, 2, 9, 2, 9, 0.5, 0.9), record(20, 30, 2, 9, 3, 10, 0.9, 0.8), record(20, 30, 12, 18, 20, 28, 0.7, 0.7)])
    store.write(5, [])
    store.write(11, [record(8, 8, 1, 4, 1, 4, 0.1, 0.2), record(8, 8, 1, 4, 1, 4, 0.1, 0.3)])
    store.write_meta({"points_per_side": [5], "sam_model": "tiny"})
    return store


@pytest.fixture()
def fake(monkeypatch):
    """ops.rle_pack and ops.rle_nms on the host: the fake keeps every second entry of an image's walk and records its arguments"""
    calls = []

    def pack(runs, H, W, slot_words=None, device=None):
        n = len(runs)
        sw = max([len(r) for r in runs] + [1])
        slots = torch.zeros((n, sw), dtype=torch.int32)
        table = torch.zeros((n, 4), dtype=torch.int32)
        for i, r in enumerate(runs):
            slots[i, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.int64).astype(np.int32))
            table[i, 0] = len(r)
        return slots, table

    def nms(slots, table, sizes, counts, scores=None, thr=0.7, metric="iou"):
        calls.append({"sizes": [tuple(int(v) for v in s) for s in sizes], "counts": list(counts), "thr": thr, "metric": metric,
                      "scores": None if scores is None else scores.tolist(), "n_counts": table[:, 0].tolist()})
        S = int(slots.shape[0])
        out_idx = torch.full((S,), -9, dtype=torch.int32)
        out_n = torch.zeros(len(counts), dtype=torch.int32)
        result = torch.zeros((S, 4), dtype=torch.int32)
        e = 0
        for g, n in enumerate(counts):
            sc = [0.0] * n if scores is None else scores[e:e + n].tolist()
            order = sorted(range(n), key=lambda i: (-sc[i], i))
            kept = order[::2]
            out_idx[e:e + len(kept)] = torch.tensor(kept, dtype=torch.int32)
            out_n[g] = len(kept)
            e += n
        if getattr(nms, "broken", None) is not None:
            result[nms.broken, 0] = 2
        return out_idx, out_n, result

    monkeypatch.setattr(ops, "rle_pack", pack)
    monkeypatch.setattr(ops, "rle_nms", nms)
    return calls, nms


NAN = float("nan")
THIN_BAD = [((0.5,), {"score": "iou"}, "score"), ((0.5,), {"score": None}, "score"), ((0.5,), {"metric": "dice"}, "metric"),
            ((0.5,), {"metric": 0}, "metric"), ((NAN,), {}, "NaN")]
CLEAN_BAD = [((-1,), {}, "min_area"), ((5, NAN), {}, "NaN"), ((5,), {"nms_thresh": NAN}, "NaN")]


@pytest.mark.parametrize("op,args,bad_args", [(P.thin, (0.5,), THIN_BAD), (P.clean, (5,), CLEAN_BAD)], ids=["thin", "clean"])
def test_refusals(src, tmp_path, fake, op, args, bad_args):
    """what thin and clean refuse alike, and each one's own arguments: all of it before any device call"""
    calls, _ = fake
    with pytest.raises(ValueError, match=f"{op.__name__}: .*same directory"):
        op(src, src.directory, *args)
    with pytest.raises(ValueError, match="same directory"):
        op(src.directory, os.path.join(src.directory, "..", "src"), *args)
    for a, kw, why in bad_args:
        with pytest.raises(ValueError, match=why):
            op(src, tmp_path / "never", *a, **kw)
    with pytest.raises(ValueError, match="no such directory"):
        op(tmp_path / "absent", tmp_path / "never", *args)
    assert not os.path.exists(tmp_path / "never") and calls == []
    # a directory that holds a store -- a record file or only its meta -- is not written into; an empty one is taken
    taken = P.ProposalStore(tmp_path / "taken")
    taken.write_meta({})
    with pytest.raises(ValueError, match="already holds a store"):
        op(src, taken, *args)
    other = P.ProposalStore(tmp_path / "other")
    other.write(1, [])
    with pytest.raises(ValueError, match="already holds a store"):
        op(src, other.directory, *args)
    assert calls == []
    os.makedirs(tmp_path / "empty")
    if op is P.thin:
        assert P.thin(src, tmp_path / "empty", 0.5)["before"] == 5
    else:      # (no fake stands in for clean's device work: a store whose images hold no record never reaches it)
        bare = P.ProposalStore(tmp_path / "bare")
        bare.write(5, [])
        bare.write_meta({"sam_model": "tiny"})
        assert P.clean(bare, tmp_path / "empty", 5) == {"per_image": {5: [0, 0, 0]}, "before": 0, "after": 0, "changed": 0}
        done = P.ProposalStore(tmp_path / "empty")
        assert done.records(5) == [] and done.meta() == {"sam_model": "tiny", "cleaned": {"min_area": 5, "nms_thresh": 0.7, "source": bare.directory}}


def test_what_it_writes_and_what_it_asks(src, tmp_path, fake):
    calls, _ = fake
    rep = P.thin(src, tmp_path / "dst", 0.25, metric="containment", score="predicted_iou", group=2)
    dst = P.ProposalStore(tmp_path / "dst")
    assert rep == {"per_image": {3: [3, 2], 5: [0, 0], 11: [2, 1]}, "before": 5, "after": 3}
    assert dst.image_ids() == [3, 5, 11]
    a = src.records(3)
    # the walk of image 3 by predicted_iou is 1, 2, 0: the fake keeps 1 and 0, and the records come in their stored order, unchanged
    assert dst.records(3) == [a[0], a[1]] and dst.records(5) == [] and dst.records(11) == [src.records(11)[0]]
    assert dst.meta() == {"points_per_side": [5], "sam_model": "tiny",
                          "thinned": {"thr": 0.25, "metric": "containment", "score": "predicted_iou", "source": src.directory}}
    # two calls of two images and one: sizes (an image without a record rides as 1 x 1), counts, the scores of the chosen field
    assert [c["sizes"] for c in calls] == [[(20, 30), (1, 1)], [(8, 8)]] and [c["counts"] for c in calls] == [[3, 0], [2]]
    assert all(c["thr"] == 0.25 and c["metric"] == "containment" for c in calls)
    assert np.allclose(calls[0]["scores"], [0.5, 0.9, 0.7]) and np.allclose(calls[1]["scores"], [0.1, 0.1])
    assert calls[0]["n_counts"] == [len(hsam.rle_counts_from_string(r["segmentation"]["counts"])) for r in a]
    # the other orders
    for score, want in (("stability_score", [0.9, 0.8, 0.7]), ("area", [49.0, 49.0, 48.0]), ("stored", None)):
        del calls[:]
        P.thin(src, tmp_path / ("by_" + score), 1.0, score=score)
        assert len(calls) == 1 and calls[0]["counts"] == [3, 0, 2] and calls[0]["metric"] == "iou"
        assert calls[0]["scores"] is None if want is None else np.allclose(calls[0]["scores"][:3], want)
        assert P.ProposalStore(tmp_path / ("by_" + score)).meta()["thinned"]["score"] == score


def test_a_record_that_does_not_decode_raises(src, tmp_path, fake):
    _, nms = fake
    nms.broken = 4      # the second record of image 11
    with pytest.raises(ValueError, match="image 11 entry 1"):
        P.thin(src, tmp_path / "dst", 0.5)
    nms.broken = None
    bad = src.records(3)
    bad[1]["segmentation"]["counts"] += "o"      # a group cut off by the end of the string
    src.write(3, bad)
    with pytest.raises(ValueError, match="image 3 entry 1: bad counts string"):
        P.thin(src, tmp_path / "dst2", 0.5)


def test_command_line(src, tmp_path, fake, capsys):
    calls, _ = fake
    out = tmp_path / "cli"
    assert P.main(["thin", src.directory, str(out), "--thr", "0.5", "--metric", "containment", "--score", "stored",
                   "--json", str(tmp_path / "rep.json")]) == 0
    assert "proposals: 5 -> 3" in capsys.readouterr().out
    assert calls[0]["metric"] == "containment" and calls[0]["scores"] is None and calls[0]["thr"] == 0.5
    rep = json.load(open(tmp_path / "rep.json"))
    assert rep["before"] == 5 and rep["after"] == 3 and rep["per_image"][0] == {"image_id": 3, "before": 3, "after": 2}
    assert P.ProposalStore(out).meta()["thinned"] == {"thr": 0.5, "metric": "containment", "score": "stored", "source": src.directory}
    with pytest.raises(SystemExit, match="same directory"):
        P.main(["thin", src.directory, src.directory, "--thr", "0.5"])
    with pytest.raises(SystemExit, match="already holds a store"):
        P.main(["thin", src.directory, str(out), "--thr", "0.5"])
    for bad in (["--metric", "dice"], ["--score", "iou"], []):      # argparse refuses an unknown name, and a call without --thr
        with pytest.raises(SystemExit):
            P.main(["thin", src.directory, str(tmp_path / "no")] + bad + ([] if not bad else ["--thr", "0.5"]))
        capsys.readouterr()
    assert not os.path.exists(tmp_path / "no")
    # clean's refusals come through the same writer of the command line, under its own name
    with pytest.raises(SystemExit, match="hybridgl_amd.proposals: clean: .*same directory"):
        P.main(["clean", src.directory, src.directory, "--min_area", "5"])
    with pytest.raises(SystemExit, match="hybridgl_amd.proposals: clean: .*already holds a store"):
        P.main(["clean", src.directory, str(out), "--min_area", "5"])
    with pytest.raises(SystemExit, match="min_area"):
        P.main(["clean", src.directory, str(tmp_path / "no"), "--min_area", "-1"])
    with pytest.raises(SystemExit, match="NaN"):
        P.main(["clean", src.directory, str(tmp_path / "no"), "--min_area", "5", "--nms_thresh", "nan"])
    with pytest.raises(SystemExit):      # argparse refuses a call without --min_area
        P.main(["clean", src.directory, str(tmp_path / "no")])
    capsys.readouterr()
    assert not os.path.exists(tmp_path / "no")
