"""The proposal store with its COCO strings written and read on the device (ProposalRecorder / StoredProposals strings="device",
main --rle_strings device), on the tiny REFER set, the tiny SAM and the recorded run of tests/test_gpu_proposal_store.py: the
files are byte-identical to the host mode's, a stored run reproduces the host mode's rows bit for bit (in groups, through
step(), with and without mask_nms_thresh), a corrupted string raises the store's ValueError with image and entry, a string cap
too small for an image takes the fallback and still writes the same files."""
import filecmp
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_proposal_store import _flags, world      # noqa: F401  (the module fixture: models, data set, runs, the host store)

pytestmark = pytest.mark.gpu


def same_files(a, b, names=None):
    if names is None:
        names = sorted(os.listdir(a))
        assert sorted(os.listdir(b)) == names
    for n in names:
        assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n
    return len(names)


def test_a_store_recorded_on_the_device_is_byte_identical(world, tmp_path):
    from hybridgl_amd import proposals as P
    w = world
    rec = P.ProposalRecorder(w.gen, tmp_path / "dev", P.generator_settings(w.gen, sam_model="tiny", precision="f16x3", proposal_cap=0),
                             strings="device")
    pipe = w.mk(rec)
    assert pipe.run(w.loader(), group=8) == len(w.refs)
    assert rec.flush() == len(w.images) and not rec._pending
    torch.cuda.synchronize()
    assert np.array_equal(pipe.partial_rows(), w.plain.partial_rows()) and pipe.metrics() == w.plain.metrics()
    assert same_files(w.store, str(tmp_path / "dev")) == len(w.images) + 1      # meta.json too
    assert rec.fallbacks == 0      # the tiny masks' strings fit the default room
    with pytest.raises(ValueError, match="strings"):
        P.ProposalRecorder(w.gen, tmp_path / "x", strings="gpu")


def test_a_cap_too_small_and_a_bit_plane_take_the_fallback(world, cuda, tmp_path):
    """the same groups through a host recorder, a device recorder and one whose room is 2 bytes per image (a mask of these
    sizes takes 3 at least); and an image whose
    one survivor is a checkerboard, which the encoder keeps as a bit plane (form 1)"""
    from hybridgl_amd import proposals as P
    w = world
    ids = list(w.images)
    recs = {"host": P.ProposalRecorder(w.gen, tmp_path / "host"), "device": P.ProposalRecorder(w.gen, tmp_path / "device", strings="device"),
            "tight": P.ProposalRecorder(w.gen, tmp_path / "tight", strings="device", string_cap=2)}
    for rec in recs.values():
        for chunk in (ids[:4], ids[4:]):
            rec.group_finish(rec.group_cleanup(rec.group_begin([w.images[i] for i in chunk], None, None, image_ids=chunk)))
        assert rec.flush() == len(ids)
    names = sorted(f"{i}.json" for i in ids)
    assert same_files(str(tmp_path / "host"), str(tmp_path / "device"), names) == len(ids)
    assert same_files(str(tmp_path / "host"), str(tmp_path / "tight"), names) == len(ids)
    busy = sum(1 for i in ids if w.sam_out[i][0].shape[0] > 0)
    assert recs["device"].fallbacks == 0 and recs["tight"].fallbacks == busy > 0
    # a form-1 entry: _record directly, with a mask no generator of this size makes
    yy, xx = np.mgrid[0:64, 0:64]
    board = torch.from_numpy(np.stack([(yy + xx) & 1, (yy < 9) & (xx > 3)]).astype(np.uint8)).to(cuda)
    args = (board, torch.tensor([[0, 0, 64, 64], [4, 0, 60, 9]], device=cuda), torch.tensor([0.5, 0.25], device=cuda),
            torch.tensor([0.75, 1.0], device=cuda), torch.tensor([0, 1], device=cuda))
    for name in ("host", "device"):
        recs[name]._record(4242, *args)
        assert recs[name].flush() == len(ids) + 1
    assert filecmp.cmp(tmp_path / "host" / "4242.json", tmp_path / "device" / "4242.json", shallow=False)
    assert recs["device"].fallbacks == 1 and len(json.load(open(tmp_path / "device" / "4242.json"))[0]["segmentation"]["counts"]) > 4000


@pytest.mark.parametrize("thr", [None, 0.3])
def test_a_stored_run_reads_its_strings_on_the_device(world, cuda, thr):
    from hybridgl_amd import proposals as P
    w = world

    def run(strings, group):
        sp = P.StoredProposals(w.store, cuda, mask_nms_thresh=thr, strings=strings)
        p = w.mk(sp)
        if group is None:
            for i in w.rr.jobs():
                p.step(w.rr.load(i))
        else:
            w.rr.proposals = sp      # files, JSON and packing on the loader threads
            try:
                assert p.run(w.loader(), group=group) == len(w.refs)
            finally:
                w.rr.proposals = None
        torch.cuda.synchronize()
        return p.partial_rows(), p.metrics(), sp.thinned

    want = run("host", 8)
    if thr is None:
        assert np.array_equal(want[0], w.plain.partial_rows())
    else:
        assert want[2][1] < want[2][0], "the threshold should thin something"
    for group in (8, 3, None):
        rows, metrics, thinned = run("device", group)
        assert np.array_equal(rows, want[0]) and metrics == want[1] and thinned == want[2], group


def test_masks_and_columns_equal_the_host_mode(world, cuda):
    from hybridgl_amd import proposals as P
    w = world
    ids = list(w.images)
    images = [w.images[i] for i in ids]
    for kw in ({}, {"mask_nms_thresh": 0.3, "mask_nms_score": "area"}, {"cap": 2}):
        a = P.StoredProposals(w.store, cuda, strings="host", **kw).generate_group(images, ids)
        b = P.StoredProposals(w.store, cuda, strings="device", **kw).generate_group(images, ids)
        for x, y in zip(a, b):
            assert all(torch.equal(torch.nan_to_num(p, nan=-7.0) if p.is_floating_point() else p,
                                   torch.nan_to_num(q, nan=-7.0) if q.is_floating_point() else q) for p, q in zip(x[:4], y[:4]))
    with pytest.raises(ValueError, match="strings"):
        P.StoredProposals(w.store, cuda, strings="gpu")


def test_a_corrupted_string_names_image_and_entry(world, cuda, tmp_path):
    import shutil
    from hybridgl_amd import proposals as P
    w = world
    store = str(tmp_path / "copy")
    shutil.copytree(w.store, store)
    iid = next(i for i in w.images if w.sam_out[i][0].shape[0] >= 2)
    path = os.path.join(store, f"{iid}.json")
    good = json.load(open(path))

    def load_with(recs):
        json.dump(recs, open(path, "w"))
        return P.StoredProposals(store, cuda, strings="device").generate_group([w.images[iid]], [iid])

    assert torch.equal(load_with(good)[0][0], w.sam_out[iid][0])
    bad = json.loads(json.dumps(good))
    bad[1]["segmentation"]["counts"] = good[1]["segmentation"]["counts"] + "o"      # a group cut off by the end of the string
    with pytest.raises(ValueError, match=f"proposal store .*copy: image {iid} entry 1: bad counts string \\(code 2"):
        load_with(bad)
    bad[1]["segmentation"]["counts"] = "o" * 8 + good[1]["segmentation"]["counts"]
    with pytest.raises(ValueError, match=f"image {iid} entry 1: bad counts string \\(code 3"):
        load_with(bad)
    from hybridgl_amd import sam as hsam
    counts = hsam.rle_counts_from_string(good[1]["segmentation"]["counts"]).tolist()
    H, W = good[1]["segmentation"]["size"]      # reads, but stops one pixel short of H*W
    bad[1]["segmentation"]["counts"] = hsam.coco_encode_rle({"size": [H, W], "counts": counts[:-1] + [counts[-1] - 1]})["counts"]
    with pytest.raises(ValueError, match=f"image {iid} entry 1: its counts do not decode"):
        load_with(bad)
    bad[1]["segmentation"]["counts"] = "é"
    with pytest.raises(ValueError, match=f"image {iid}: bad counts string .*entry 1"):
        load_with(bad)


def test_the_driver_flag(world, cuda, golden_dir, tmp_path):
    """--save_proposals with --rle_strings device writes the host run's files; --proposals_dir with it gives the host read's report"""
    from hybridgl_amd import main as drv
    from hybridgl_amd import proposals as P
    w = world
    base = _flags(w.root, golden_dir, "--sam_model", "tiny", "--points_per_side", "5", "--pred_iou_thresh", "-1.0",
                  "--stability_score_thresh", "0", "--min_mask_region_area", "2", "--group", "4", "--workers", "2",
                  "--result_dir", str(tmp_path / "log"), "--max_refs", "9", "--fusion_mode", "G2L")
    parse = drv.default_argument_parser().parse_args
    assert parse(base).rle_strings == "host"
    stores, metrics = {}, {}
    for mode in ("host", "device"):
        stores[mode] = str(tmp_path / f"props_{mode}")
        save = parse(base + ["--save_proposals", stores[mode], "--rle_strings", mode])
        drv.resolve_defaults(save)
        save.precision = "f16x3"
        m, st = drv.evaluate(save, w.model, w.gen, w.gem, cuda)
        assert st["proposals_saved"] == 9
    assert same_files(stores["host"], stores["device"]) == 10
    for mode in ("host", "device"):
        read = parse(base + ["--proposals_dir", stores["host"], "--rle_strings", mode])
        if mode == "host":
            gen = P.StoredProposals(stores["host"], cuda)
        else:      # as the driver builds it
            model, gen, gem = drv.build_models(read, cuda)
        assert isinstance(gen, P.StoredProposals) and gen.strings == mode
        metrics[mode], _ = drv.evaluate(read, w.model, gen, w.gem, cuda)
    assert metrics["host"] == metrics["device"] and metrics["host"]["n_sentences"] >= 9
