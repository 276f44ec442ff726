"""hgl_rle_encode_device (csrc/rle.hip) through ops.rle_encode / sam.masks_to_rle: bit-exact against the reference's
maskApi.c vectors and digests (tests/golden/gtmask*.npz) and against the host codec sam.mask_to_rle, plus the contract of the
slot forms (containment, selection by a device index tensor, out-of-range indices) and the mask generator's RLE modes."""
import os

import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import sam as hsam
from oracle import gen_gtmask_golden as GG

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A      # as int32: positive, never a table value of the shapes below


def bit_plane(mask):
    """bit p % 32 of word p / 32 over the column-major order p = x*H + y, packed by numpy"""
    flat = (np.asarray(mask) != 0).T.reshape(-1).astype(np.uint8)
    flat = np.concatenate([flat, np.zeros((-len(flat)) % 32, np.uint8)])
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)


def encode(masks, cuda, sel=None, slot_words=None, as_bool=False):
    """ops.rle_encode into a sentinel-filled buffer -> (slots uint32 [S, slot_words], table int32 [S, 4]) on the host"""
    masks = np.ascontiguousarray(masks)
    N, H, W = masks.shape
    t = torch.from_numpy(masks.astype(np.uint8)).to(cuda)
    if as_bool:
        t = t.bool()
    S = N if sel is None else int(sel.numel())
    sw = ops.rle_slot_words(H, W) if slot_words is None else slot_words
    flat = torch.full((S * (4 + sw),), SENTINEL, dtype=torch.int32, device=cuda)
    slots, table = ops.rle_encode(t, sel, slot_words, out=flat)
    assert tuple(slots.shape) == (S, sw) and tuple(table.shape) == (S, 4)
    return slots.cpu().numpy().view(np.uint32), table.cpu().numpy()


def check_entry(slot, row, mask, what=""):
    """one entry against the host codec: the table row, what the slot holds in its form, and nothing beyond it"""
    H, W = mask.shape
    want = hsam.mask_to_rle(mask)["counts"]
    n, words, sw = len(want), (H * W + 31) // 32, len(slot)
    form = 0 if n <= sw else (1 if words <= sw else 2)
    assert row.tolist() == [n, form, int((mask != 0).sum()), 0], (what, row.tolist(), n, form)
    if form == 0:
        assert slot[:n].tolist() == want, what
        assert (slot[n:] == SENTINEL).all(), what
    elif form == 1:
        assert np.array_equal(slot[:words], bit_plane(mask)), what
        assert (slot[words:] == SENTINEL).all(), what
        assert hsam.rle_from_slot(slot, n, 1, H, W) == want, what
    else:
        assert (slot == SENTINEL).all(), what
    return form


def blobs(n, H, W, seed):
    """seeded unions of ellipses: long runs, some touching the border"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, ry, rx = rng.random() * H, rng.random() * W, (0.05 + 0.3 * rng.random()) * H, (0.05 + 0.3 * rng.random()) * W
            out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
    return out


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "gtmask.npz"))


@pytest.fixture(scope="module")
def fuzz_gold(golden_dir):
    return np.load(os.path.join(golden_dir, "gtmask_fuzz.npz"))


def test_reference_vectors(cuda, gold):
    """every r{j}_mask of the reference's maskApi.c vectors -> exactly r{j}_counts and, through coco_encode_rle, r_strings"""
    strs = [str(s) for s in gold["r_strings"]]
    for j in range(int(gold["n_rle"][0])):
        H, W = (int(v) for v in gold[f"r{j}_size"])
        mask = gold[f"r{j}_mask"]
        rle, = hsam.masks_to_rle(torch.from_numpy(np.ascontiguousarray(mask[None])).to(cuda))
        assert rle == {"size": [H, W], "counts": gold[f"r{j}_counts"].tolist()}, j
        assert hsam.coco_encode_rle(rle) == {"size": [H, W], "counts": strs[j]}, j
        slots, table = encode(mask[None], cuda)
        assert int(table[0, 2]) == int(mask.sum())


def test_fuzz_against_the_reference_digests(cuda, fuzz_gold):
    """The 120 masks of the host codec's fuzz (sizes 1 .. 299, blobs and noise), each encoded twice: with a slot of H*W + 1
    words (the run form, even for noise) and with the default slot (noise then takes the bit-plane form).  Counts and
    strings against the digests of the reference's own outputs: bit-exact."""
    forms = set()
    for t, m in enumerate(GG.fuzz_rle_masks()):
        H, W = m.shape
        for sw in (H * W + 1, None):
            slots, table = encode(m[None], cuda, slot_words=sw)
            form = check_entry(slots[0], table[0], m, (t, sw))
            assert form == 0 or sw is None
            forms.add((sw is None, form))
            counts = hsam.rle_from_slot(slots[0], int(table[0, 0]), form, H, W)
            s = hsam.coco_encode_rle({"size": [H, W], "counts": counts})["counts"]
            assert GG.digest(counts) == str(fuzz_gold["rle_counts_digest"][t]), (t, sw)
            assert GG.digest(s) == str(fuzz_gold["rle_string_digest"][t]), (t, sw)
    assert forms == {(False, 0), (True, 0), (True, 1)}      # both forms occurred with the default slot


SIZES = [(1, 1), (1, 70), (70, 1), (33, 5), (63, 64), (64, 63), (65, 129), (100, 37)]


def edge_masks(H, W):
    out = {k: np.zeros((H, W), np.uint8) for k in ("zeros", "ones", "first", "last", "spans a column boundary",
                                                   "ends at a column boundary")}
    out["ones"][:] = 1
    out["first"][0, 0] = 1
    out["last"][H - 1, W - 1] = 1
    x = max(W // 2 - 1, 0)
    out["spans a column boundary"][H - 1, x] = 1      # the last pixel of column x and the first of column x + 1: one run
    out["spans a column boundary"][0, min(x + 1, W - 1)] = 1
    out["ends at a column boundary"][H // 2:, x] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = ((yy + xx) & 1).astype(np.uint8)
    out["checkerboard from (0,0)"] = ((yy + xx + 1) & 1).astype(np.uint8)
    return out


@pytest.mark.parametrize("H,W", SIZES)
def test_edge_masks_against_the_host_codec(cuda, H, W):
    cases = edge_masks(H, W)
    assert hsam.mask_to_rle(cases["zeros"])["counts"] == [H * W] and hsam.mask_to_rle(cases["ones"])["counts"] == [0, H * W]
    batch = np.stack(list(cases.values()))
    for sw in (H * W + 1, None):      # the run form for all of them; the default slot (the checkerboards take the bit plane)
        slots, table = encode(batch, cuda, slot_words=sw, as_bool=sw is None)
        for i, name in enumerate(cases):
            check_entry(slots[i], table[i], batch[i], (name, H, W, sw))
        if sw is not None:
            i = list(cases).index("zeros")
            assert slots[i, 0] == H * W and table[i, 0] == 1
            i = list(cases).index("ones")
            assert slots[i, :2].tolist() == [0, H * W] and table[i, 0] == 2


@pytest.mark.parametrize("H,W", [(480, 640), (640, 480)])
def test_blob_batches_at_image_size(cuda, H, W):
    """non-square: a transposition anywhere gives other runs"""
    batch = blobs(8, H, W, seed=H)
    rles = hsam.masks_to_rle(torch.from_numpy(batch).to(cuda))
    slots, table = encode(batch, cuda)
    for i in range(8):
        assert rles[i] == hsam.mask_to_rle(batch[i]), i
        assert check_entry(slots[i], table[i], batch[i], i) == 0


def test_one_megapixel_mask_takes_many_chunks(cuda):
    """1024 x 1024: 16384 column words, 64 chunks of the scan with a carried rank and position; blobs plus a noisy band"""
    m = blobs(1, 1024, 1024, seed=3)[0]
    m[300:340] ^= (np.random.default_rng(4).random((40, 1024)) < 0.3).astype(np.uint8)
    slots, table = encode(m[None], cuda)
    assert check_entry(slots[0], table[0], m) == 0
    assert int(table[0, 0]) > 10000


def test_selection_by_a_device_index_tensor(cuda):
    H, W = 37, 50
    batch = blobs(5, H, W, seed=11)
    batch[3] ^= (np.random.default_rng(12).random((H, W)) < 0.5).astype(np.uint8)      # one entry in the bit-plane form
    order = [4, 0, 0, 3, 3, 3, 1]      # S > N, repeats
    sel = torch.tensor(order, dtype=torch.int64, device=cuda)
    slots, table = encode(batch, cuda, sel=sel)
    forms = [check_entry(slots[s], table[s], batch[n], (s, n)) for s, n in enumerate(order)]
    assert set(forms) == {0, 1}
    rles = hsam.masks_to_rle(torch.from_numpy(batch).to(cuda), sel.to(torch.int32))      # any integer dtype
    assert rles == [hsam.mask_to_rle(batch[n]) for n in order]
    # sel=None, S = 3 through the C entry: masks 0 .. 2
    from hybridgl_amd import _lib
    lib = _lib.load()
    t = torch.from_numpy(batch).to(cuda)
    sw = ops.rle_slot_words(H, W)
    flat = torch.full((3 * (4 + sw),), SENTINEL, dtype=torch.int32, device=cuda)
    ws = ops.workspace(lib.hgl_rle_encode_workspace_bytes(3, H, W), cuda, "rle")
    _lib.check(lib.hgl_rle_encode_device(t.data_ptr(), 5, H, W, None, 3, flat.data_ptr() + 48, sw, flat.data_ptr(), ws.data_ptr(),
                                         ws.numel(), torch.cuda.current_stream().cuda_stream), "hgl_rle_encode_device")
    s3, t3 = ops.rle_split(flat.cpu().numpy(), 3, sw)
    for i in range(3):
        check_entry(s3[i].view(np.uint32), t3[i], batch[i], i)
    # ... and S > N without an index tensor is refused, as is a workspace that is too small
    assert lib.hgl_rle_encode_device(t.data_ptr(), 5, H, W, None, 6, flat.data_ptr() + 48, sw, flat.data_ptr(), ws.data_ptr(),
                                     ws.numel(), None) == -1
    assert lib.hgl_rle_encode_device(t.data_ptr(), 5, H, W, None, 3, flat.data_ptr() + 48, sw, flat.data_ptr(), ws.data_ptr(),
                                     8, None) == -3


def test_indices_out_of_range_are_form_3(cuda):
    """the kernel guards the indices itself (the host never sees them): nothing read, nothing written but the table row"""
    H, W = 20, 24
    batch = blobs(3, H, W, seed=21)
    order = [2, -1, 3, 1, 1 << 40]
    slots, table = encode(batch, cuda, sel=torch.tensor(order, dtype=torch.int64, device=cuda))
    for s, n in enumerate(order):
        if 0 <= n < 3:
            check_entry(slots[s], table[s], batch[n], s)
        else:
            assert table[s].tolist() == [0, 3, 0, 0] and (slots[s] == SENTINEL).all(), s


def test_a_slot_too_small_for_either_form_stays_untouched(cuda):
    H, W = 33, 40
    yy, xx = np.mgrid[0:H, 0:W]
    # a checkerboard that starts with foreground: H*W runs of one pixel after the leading 0 count
    batch = np.stack([((yy + xx + 1) & 1).astype(np.uint8), np.zeros((H, W), np.uint8), blobs(1, H, W, seed=5)[0]])
    slots, table = encode(batch, cuda, slot_words=4)
    assert [check_entry(slots[i], table[i], batch[i], i) for i in range(3)][:2] == [2, 0]
    assert table[0].tolist() == [H * W + 1, 2, int(batch[0].sum()), 0] and (slots[0] == SENTINEL).all()
    # exactly the bit plane's size: the checkerboard (H*W + 1 runs) is kept as bits
    slots, table = encode(batch, cuda)
    assert [check_entry(slots[i], table[i], batch[i], i) for i in range(3)][:2] == [1, 0]


def test_two_calls_give_identical_bytes(cuda):
    batch = blobs(4, 130, 70, seed=31)
    batch[1] ^= (np.random.default_rng(32).random((130, 70)) < 0.4).astype(np.uint8)
    a = encode(batch, cuda)
    b = encode(batch, cuda)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_generator_rle_modes_equal_the_host_codec(cuda):
    """SamAutomaticMaskGenerator.generate() in the RLE modes (runs from the device, area from the table) gives the records
    the host codec gives on the binary_mask records' masks"""
    from hybridgl_amd import weights
    from oracle.cases import sam_tiny_case
    sd = weights.sam_state_dict("tiny", 0)
    model = hsam.Sam(sd, weights.SAM_CONFIGS["tiny"], cuda)
    c = sam_tiny_case()
    kw = dict(points_per_side=4, pred_iou_thresh=-1e9, stability_score_thresh=0.0, crop_n_layers=0, min_mask_region_area=20,
              box_nms_thresh=1.5)
    plain = hsam.SamAutomaticMaskGenerator(model, **kw).generate(c["image"])
    assert len(plain) > 0 and plain[0]["segmentation"].shape == (160, 200)
    for mode in ("uncompressed_rle", "coco_rle"):
        gen = hsam.SamAutomaticMaskGenerator(model, output_mode=mode, **kw)
        anns = gen.generate(c["image"])
        assert len(anns) == len(plain)
        for a, b in zip(anns, plain):
            assert a["segmentation"] == gen._segmentation(b["segmentation"])
            assert a["area"] == int(b["segmentation"].sum()) and type(a["area"]) is int
            assert a["bbox"] == b["bbox"] and a["crop_box"] == b["crop_box"] and a["point_coords"] == b["point_coords"]
