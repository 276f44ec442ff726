"""CPU: the entries of the grouped RLE decoder (declared, bound, refusing without a device) and the proposal store on the
host -- records built from the reference's generate() golden written, read back and packed for the device, [] images,
meta.json, files that are missing, truncated or garbled, the atomic write, and the driver's flag rules."""
import json
import os
import re

import numpy as np
import pytest

from hybridgl_amd import _lib
from hybridgl_amd import proposals as P
from hybridgl_amd import sam as hsam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hgl_rle_decode_group_workspace_bytes", "hgl_rle_decode_group_device"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_binding_binds_the_new_entries(lib):
    text = open(os.path.join(ROOT, "include", "hybridgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert re.search(r"#define\s+HGL_ABI_VERSION\s+7\b", text)
    assert lib.hgl_abi_version() == _lib.ABI_VERSION == 7
    # the export cites the reference lines it replaces, as every export does
    doc = text[:text.index("size_t hgl_rle_decode_group_workspace_bytes")].rsplit("/*", 1)[1]
    assert "scripts/amg.py:229-232" in doc and "utils/amg.py:303-346" in doc


def test_group_entry_refuses_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    images = np.array([[4, 4, 0, 0]], np.int64)
    assert lib.hgl_rle_decode_group_device(None, 4, None, 1, images.ctypes.data, 1, None, 16, None, None, None, 0, None) == -2
    assert b"no HIP device" in lib.hgl_last_error()


def test_group_workspace_query_is_host_arithmetic(lib):
    # the run starts: slot_words + 1 words per entry, whatever the images' sizes are
    assert lib.hgl_rle_decode_group_workspace_bytes(2, 10) >= 2 * 11 * 4
    assert lib.hgl_rle_decode_group_workspace_bytes(2, 10) == lib.hgl_rle_decode_workspace_bytes(2, 65, 3, 10)
    assert lib.hgl_rle_decode_group_workspace_bytes(1024, 12800) >= 1024 * 12801 * 4
    assert lib.hgl_rle_decode_group_workspace_bytes(0, 4) == 0 and lib.hgl_rle_decode_group_workspace_bytes(3, -1) == 0


def same(a, b):
    """equal record lists; the stability of an empty mask is 0 / 0 = NaN on both sides, which == does not see as equal"""
    return json.dumps(a) == json.dumps(b)


@pytest.fixture(scope="module")
def golden_records(golden_dir):
    """records in coco_rle mode from the reference's generate() with crop layers (oracle/gen_golden.py, sam_crops.npz 'a_'):
    every third of its 192 survivors, 240 x 320 (the fixture keeps the masks as packed bits)"""
    z = np.load(os.path.join(golden_dir, "sam_crops.npz"))
    sel = range(0, len(z["a_masks"]), 3)
    masks = np.unpackbits(z["a_masks"][list(sel)], axis=-1)[..., :320]
    recs = []
    for i, m in zip(sel, masks):
        assert int(m.sum()) == int(z["a_area"][i])
        ys, xs = np.nonzero(m)      # the reference's bbox is the box of its mask: what StoredProposals holds a store to
        assert z["a_bbox"][i].tolist() == ([0, 0, 0, 0] if not len(ys) else [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()])
        rle = hsam.coco_encode_rle(hsam.mask_to_rle(m))
        recs.append({"segmentation": rle, "area": int(z["a_area"][i]), "bbox": [int(v) for v in z["a_bbox"][i]],
                     "predicted_iou": float(z["a_iou"][i]), "point_coords": [z["a_points"][i].tolist()],
                     "stability_score": float(z["a_stab"][i]), "crop_box": [int(v) for v in z["a_crop_box"][i]]})
    return recs, masks


def test_store_round_trip(tmp_path, golden_records):
    recs, masks = golden_records
    store = P.ProposalStore(tmp_path / "store")
    store.write(581921, recs)
    store.write(7, [])
    meta = {"points_per_side": [8, 4], "pred_iou_thresh": 0.7, "crop_n_layers": 1, "sam_model": "tiny", "precision": "f16x3",
            "proposal_cap": 0, "mask_threshold": 0.0, "min_mask_region_area": 800}
    store.write_meta(meta)
    assert sorted(os.listdir(store.directory)) == ["581921.json", "7.json", "meta.json"]      # no temporary file stays
    again = P.ProposalStore(str(tmp_path / "store"))
    got = again.records(581921)
    assert same(got, recs) and any(r["stability_score"] != r["stability_score"] for r in got) and [type(v) for v in got[0].values()] == [type(v) for v in recs[0].values()]
    assert list(got[0]) == list(P.RECORD_KEYS)
    assert again.records(7) == [] and again.meta() == meta and again.has(7) and not again.has(8)
    assert P.ProposalStore(tmp_path / "nowhere").meta() == {}
    # the file is what anything that reads SAM's output reads: a JSON list whose strings decode to the masks
    raw = json.load(open(store.path(581921)))
    for r, m in zip(raw, masks):
        assert r["segmentation"]["size"] == [240, 320] and np.array_equal(hsam.rle_to_mask(
            {"size": [240, 320], "counts": hsam.rle_counts_from_string(r["segmentation"]["counts"]).tolist()}), m != 0)
        assert r["area"] == int(m.sum())


def test_bad_files_raise_and_name_the_image(tmp_path, golden_records):
    recs, _ = golden_records
    store = P.ProposalStore(tmp_path)
    with pytest.raises(ValueError, match="image 12 has no file"):
        store.records(12)
    store.write(12, recs[:3])
    text = open(store.path(12)).read()
    open(store.path(12), "w").write(text[:len(text) // 2])      # truncated
    with pytest.raises(ValueError, match="image 12"):
        store.records(12)
    open(store.path(12), "wb").write(b"\xff\xfe garbage {")      # garbled
    with pytest.raises(ValueError, match="image 12"):
        store.records(12)
    open(store.path(12), "w").write(json.dumps({"not": "a list"}))
    with pytest.raises(ValueError, match="image 12"):
        store.records(12)
    bad = [dict(recs[0]), {k: v for k, v in recs[1].items() if k != "bbox"}]
    open(store.path(12), "w").write(json.dumps(bad))
    with pytest.raises(ValueError, match="image 12 entry 1"):
        store.records(12)
    bad = [dict(recs[0], segmentation={"size": [240, 320], "counts": [1, 2, 3]})]      # uncompressed counts: another format
    open(store.path(12), "w").write(json.dumps(bad))
    with pytest.raises(ValueError, match="image 12 entry 0"):
        store.records(12)


def test_the_write_is_atomic(tmp_path, golden_records, monkeypatch):
    """a write that fails half way leaves no file under the final name (a first write) or the previous file (a rewrite), and
    no temporary file"""
    recs, _ = golden_records
    store = P.ProposalStore(tmp_path)
    real = json.dump

    def half(obj, f, **kw):
        f.write(json.dumps(obj)[:40])
        f.flush()
        raise OSError("disk full")

    monkeypatch.setattr(P.json, "dump", half)
    with pytest.raises(OSError):
        store.write(5, recs)
    assert os.listdir(tmp_path) == []
    monkeypatch.setattr(P.json, "dump", real)
    store.write(5, recs[:2])
    monkeypatch.setattr(P.json, "dump", half)
    with pytest.raises(OSError):
        store.write(5, recs)
    monkeypatch.setattr(P.json, "dump", real)
    assert os.listdir(tmp_path) == ["5.json"] and same(store.records(5), recs[:2])


def test_prefetch_packs_one_buffer_per_image(tmp_path, golden_records):
    """the host half of StoredProposals: table, counts and the two scores of an image in ONE int32 buffer"""
    from hybridgl_amd import ops
    recs, masks = golden_records
    store = P.ProposalStore(tmp_path)
    store.write(3, recs)
    store.write(4, [])
    sp = P.StoredProposals(store, "cpu")
    rows = sp.prefetch(3, (240, 320))
    counts = [hsam.mask_to_rle(m)["counts"] for m in masks]
    n, sw = len(recs), max(len(c) for c in counts)
    assert (rows.n, rows.H, rows.W, rows.sw) == (n, 240, 320, sw) and rows.buf.numel() == n * (6 + sw)
    slots, table = ops.rle_split(rows.buf.numpy(), n, sw)
    assert table[:, 0].tolist() == [len(c) for c in counts] and not table[:, 1:].any()
    for k, c in enumerate(counts):
        assert slots[k, :len(c)].view(np.uint32).tolist() == c
    tail = rows.buf.numpy()[n * (4 + sw):].view(np.float32)
    assert np.array_equal(tail[:n], np.array([r["predicted_iou"] for r in recs], np.float32))
    assert np.array_equal(tail[n:], np.array([r["stability_score"] for r in recs], np.float32), equal_nan=True)
    assert rows.bbox.tolist() == [r["bbox"] for r in recs]
    assert sp.prefetch(3, (240, 320)) is rows and sp.loaded == 1      # staged once
    empty = sp.prefetch(4, (17, 9))
    assert empty.n == 0 and empty.buf.numel() == 0
    assert same(sp.records(3), recs)
    # errors name the image and the entry; nothing falls back to running SAM (there is no model to run)
    with pytest.raises(ValueError, match="image 9 has no file"):
        sp.prefetch(9, (240, 320))
    with pytest.raises(ValueError, match="image 3 entry 0: size"):
        P.StoredProposals(store, "cpu").prefetch(3, (240, 321))
    with pytest.raises(ValueError, match="image_id"):
        sp.prefetch(None, (240, 320))
    bad = [dict(r) for r in recs[:4]]
    bad[2] = dict(bad[2], segmentation={"size": [240, 320], "counts": bad[2]["segmentation"]["counts"] + "o"})      # cut off in a group
    store.write(6, bad)
    with pytest.raises(ValueError, match="image 6 entry 2"):
        sp.prefetch(6, (240, 320))
    bad[2] = dict(recs[2], segmentation={"size": [320, 240], "counts": recs[2]["segmentation"]["counts"]})
    store.write(6, bad)
    with pytest.raises(ValueError, match="image 6 entry 2: size"):
        sp.prefetch(6, (240, 320))


def test_the_staged_group_holds_the_rows_of_its_images(tmp_path):
    """the host half of a group, P._stage_group: table | slots | iou | stability (| area) of the first counts[g] entries of
    every image, image after image -- a cap that cuts the first image, an image without a record in the middle, the widest slot
    in an image that is not cut -- and the slot width of a group is that of the images that contribute an entry"""
    def rec(m, iou, stab):
        ys, xs = np.nonzero(m)
        return {"segmentation": hsam.coco_encode_rle(hsam.mask_to_rle(m)), "area": int(m.sum()), "predicted_iou": iou, "stability_score": stab,
                "bbox": [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())], "point_coords": [[0.0, 0.0]],
                "crop_box": [0, 0, 8, 8]}

    def bar(y0, y1, x0, x1):
        m = np.zeros((8, 8), np.uint8)
        m[y0:y1, x0:x1] = 1
        return m

    checker = (np.indices((8, 8)).sum(0) % 2).astype(np.uint8)
    store = P.ProposalStore(tmp_path)
    store.write(1, [rec(bar(2, 6, 1, 4), 0.9, 0.5), rec(bar(1, 3, 0, 8), 0.8, 0.25), rec(bar(0, 8, 3, 4), 0.7, 0.125)])
    store.write(2, [])
    store.write(3, [rec(bar(0, 8, 2, 5), 0.6, 0.75)])
    store.write(4, [rec(checker, 0.4, 0.0625), rec(bar(3, 5, 3, 5), 0.3, 1.0)])
    ids = [1, 2, 3, 4]
    for area, kw in ((False, {}), (True, {"mask_nms_thresh": 0.5, "mask_nms_score": "area"})):
        sp = P.StoredProposals(store, "cpu", **kw)
        rows = [sp.prefetch(i, (8, 8)) for i in ids]
        assert [r.n for r in rows] == [3, 0, 1, 2] and rows[3].sw > rows[0].sw > rows[2].sw > 1
        assert all(r.area.size == (r.n if area else 0) for r in rows)
        for counts, sw in (([2, 0, 1, 2], rows[3].sw), ([0, 0, 1, 0], rows[2].sw), ([0, 0, 0, 0], 0)):
            S = sum(counts)
            words = S * (6 + sw + area)
            buf = np.full(words + 5, -7, np.int32)
            got = P._stage_group(rows, counts, area, buf)
            assert got[:2] == (S, sw) and got[2].tolist() == np.cumsum([0] + counts).tolist()
            assert (buf[words:] == -7).all()
            table, slots = buf[:4 * S].reshape(S, 4), buf[4 * S:S * (4 + sw)].reshape(S, sw)
            tail = buf[S * (4 + sw):words].reshape(2 + area, S)
            for r, n, e in zip(rows, counts, got[2]):
                assert np.array_equal(table[e:e + n], r.table[:n])
                for k in range(n):
                    nc = int(r.table[k, 0])
                    assert nc > 0 and np.array_equal(slots[e + k, :nc], r.slots[k, :nc])
                assert (slots[e:e + n, r.sw:] == -7).all()      # beyond an image's own slot width nothing is written
                assert np.array_equal(tail[0, e:e + n], r.iou[:n]) and np.array_equal(tail[1, e:e + n], r.stab[:n])
                if area:
                    assert np.array_equal(tail[2, e:e + n], r.area[:n])
        # the views are the one buffer's, and hold what the records say
        r = rows[0]
        assert r.iou.view(np.float32).tolist() == [np.float32(v) for v in (0.9, 0.8, 0.7)] and r.stab.view(np.float32).tolist() == [0.5, 0.25, 0.125]
        assert np.shares_memory(r.table, r.buf.numpy()) and np.shares_memory(r.stab, r.buf.numpy())
        if area:
            assert r.area.view(np.float32).tolist() == [12.0, 16.0, 8.0]


def test_generator_settings_and_the_flag_rules():
    from hybridgl_amd import main as drv

    class Model:
        mask_threshold = 0.25

    class Gen:
        point_grids = [np.zeros((64, 2)), np.zeros((16, 2))]
        points_per_batch, pred_iou_thresh, stability_score_thresh, stability_score_offset = 64, 0.7, 0.7, 1.0
        box_nms_thresh, crop_nms_thresh, crop_n_layers, crop_overlap_ratio, min_mask_region_area = 0.7, 0.7, 1, 512 / 1500, 800
        model = Model()

    meta = P.generator_settings(Gen(), sam_model="default", precision="f16x3", proposal_cap=64)
    for key in ("points_per_side", "pred_iou_thresh", "stability_score_thresh", "box_nms_thresh", "crop_nms_thresh", "crop_n_layers",
                "min_mask_region_area", "mask_threshold", "sam_model", "precision", "proposal_cap"):
        assert key in meta, key
    assert meta["points_per_side"] == [8, 4] and meta["mask_threshold"] == 0.25 and json.loads(json.dumps(meta)) == meta
    parse = drv.default_argument_parser().parse_args
    for flags in (["--real", "--save_proposals", "a", "--proposals_dir", "b"], ["--save_proposals", "a"], ["--proposals_dir", "b"],
                  ["--real", "--proposals_dir", "b", "--prepare"]):
        with pytest.raises(SystemExit):
            drv.check_proposal_flags(parse(flags))
    for flags in (["--real", "--save_proposals", "a", "--save_masks", "m", "--sweep", "r=0.3,0.5"], ["--real", "--proposals_dir", "b"],
                  ["--real"], []):
        drv.check_proposal_flags(parse(flags))


# (S, G, thin): the words of StoredProposals' read-back without the string codec's status, then the ranges aux, out_src, out_n,
# nms, codes -- 8*S, or 14*S + 2*G with the bounds 8*S, 9*S, 9*S+G, 10*S+G and 14*S+G, worked out by hand
BACK_LAYOUTS = {(1, 1, False): (8, (0, 8), (8, 8), (8, 8), (8, 8), (8, 8)),
                (1, 3, False): (8, (0, 8), (8, 8), (8, 8), (8, 8), (8, 8)),
                (5, 1, False): (40, (0, 40), (40, 40), (40, 40), (40, 40), (40, 40)),
                (5, 3, False): (40, (0, 40), (40, 40), (40, 40), (40, 40), (40, 40)),
                (1, 1, True): (16, (0, 8), (8, 9), (9, 10), (10, 16), (11, 15)),
                (1, 3, True): (20, (0, 8), (8, 9), (9, 12), (12, 20), (13, 17)),
                (5, 1, True): (72, (0, 40), (40, 45), (45, 46), (46, 72), (51, 71)),
                (5, 3, True): (76, (0, 40), (40, 45), (45, 48), (48, 76), (53, 73))}


@pytest.mark.parametrize("strings", [False, True])
@pytest.mark.parametrize("case", sorted(BACK_LAYOUTS))
def test_the_read_back_layout_is_the_one_both_halves_spelled_out(case, strings):
    S, G, thin = case
    words, aux, out_src, out_n, nms, codes = BACK_LAYOUTS[case]
    total, part = P._back_layout(S, G, thin, strings)
    assert total == words + ({1: 4, 5: 20}[S] if strings else 0)
    got = {k: (v.start, v.stop) for k, v in part.items()}
    assert got == {"aux": aux, "out_src": out_src, "out_n": out_n, "nms": nms, "codes": codes, "read": (words, total)}
    chain = [got[k] for k in ("aux", "out_src", "out_n", "nms", "read")]      # disjoint, in order, and they cover [0, total)
    assert chain[0][0] == 0 and chain[-1][1] == total
    assert all(a <= b for a, b in chain) and all(x[1] == y[0] for x, y in zip(chain, chain[1:]))
    assert nms[0] <= codes[0] <= codes[1] <= nms[1] and all(v.step is None for v in part.values())


def test_build_records_is_one_builder_for_counts_strings_and_finished_segmentations(lib):
    """two masks of 5 x 7: the records from their counts, from the strings the device would have written and from ready-made
    segmentations are the JSON the builder gave before generate() shared it"""
    counts = [[11, 3, 2, 3, 2, 3, 11], [0, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 2, 1]]
    rest = ([9, 15], np.array([[2, 1, 3, 3], [0, 0, 7, 5]], np.int64), np.array([0.875, 0.5], np.float32),
            np.array([0.96875, 1.0], np.float32), np.array([[3.5, 2.5], [0.25, 1.0]]), np.array([[0, 0, 7, 5], [1, 0, 7, 4]], np.int64))
    want = ('[{"segmentation": {"size": [5, 7], "counts": ";320009"}, "area": 9, "bbox": [2, 1, 3, 3], "predicted_iou": 0.875, '
            '"point_coords": [[3.5, 2.5]], "stability_score": 0.96875, "crop_box": [0, 0, 7, 5]}, '
            '{"segmentation": {"size": [5, 7], "counts": "02300000000000OO"}, "area": 15, "bbox": [0, 0, 7, 5], "predicted_iou": 0.5, '
            '"point_coords": [[0.25, 1.0]], "stability_score": 1.0, "crop_box": [1, 0, 6, 4]}]')
    assert P.build_records is hsam.build_records
    assert json.dumps(P.build_records(5, 7, counts, *rest)) == want
    assert json.dumps(P.build_records(5, 7, [np.asarray(c, np.uint32) for c in counts], *rest)) == want
    assert json.dumps(P.build_records(5, 7, None, *rest, [b";320009", b"02300000000000OO"])) == want
    segs = [{"size": [5, 7], "counts": ";320009"}, {"size": [5, 7], "counts": "02300000000000OO"}]
    assert json.dumps(P.build_records(5, 7, None, *rest, segmentations=segs)) == want
    raw = P.build_records(5, 7, None, *rest, segmentations=[{"size": [5, 7], "counts": c} for c in counts])      # uncompressed_rle
    assert [r["segmentation"]["counts"] for r in raw] == counts and [type(r["area"]) for r in raw] == [int, int]
    assert all(type(r["predicted_iou"]) is float and type(r["bbox"][0]) is int and type(r["crop_box"][3]) is int for r in raw)
