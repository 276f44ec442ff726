"""hgl_rle_decode_device / hgl_rle_iou_device (csrc/rle.hip) through ops.rle_pack / ops.rle_decode / ops.rle_iou and
sam.rles_to_masks: bit-exact against the oracle's counts_to_mask and the host codec sam.rle_to_mask (pinned to the reference's
maskApi.c by the CPU tests) on the reference's vectors, the codec's fuzz, the edge shapes of the column-word and tile
boundaries, both slot forms straight from the device encoder, malformed counts, and the contract of the entry (containment,
unaligned outputs, determinism)."""
import os

import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import sam as hsam
from oracle import gen_gtmask_golden as GG
from oracle import gtmask_oracle as G

pytestmark = pytest.mark.gpu

SENT = 0x5A


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


def decode(slots, table, H, W, spare=4096, offset=0):
    """ops.rle_decode into a sentinel-filled buffer with `spare` bytes behind S*H*W (and `offset` in front): the spare bytes
    stay, every byte inside is 0 or 1 -> (masks [S,H,W] uint8, status [S,4]) on the host"""
    S = int(slots.shape[0])
    n = S * H * W
    buf = torch.full((offset + n + spare,), SENT, dtype=torch.uint8, device=slots.device)
    masks, status = ops.rle_decode(slots, table, H, W, out=buf[offset:offset + n])
    assert tuple(masks.shape) == (S, H, W) and tuple(status.shape) == (S, 4) and masks.data_ptr() == buf.data_ptr() + offset
    host = buf.cpu().numpy()
    assert (host[:offset] == SENT).all() and (host[offset + n:] == SENT).all(), "wrote outside the output"
    inside = host[offset:offset + n]
    assert inside.max(initial=0) <= 1, "a byte inside is neither 0 nor 1"
    return inside.reshape(S, H, W), status.cpu().numpy()


def decode_counts(counts_list, H, W, cuda, slot_words=None, **kw):
    slots, table = ops.rle_pack(counts_list, H, W, slot_words=slot_words, device=cuda)
    return decode(slots, table, H, W, **kw)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "gtmask.npz"))


def test_oracle_and_host_codec_agree():
    """the two references of this file say the same on the malformed inputs used below"""
    for H, W in ((4, 4), (33, 5)):
        for c in ([], [H * W], [0, H * W], [3, 0, 0, 2, 0, 4, H * W - 9], [5, H * W - 6], [5, 2, H * W], [0xFFFFFFFF, 5]):
            assert np.array_equal(G.counts_to_mask(c, H, W) != 0, hsam.rle_to_mask({"size": [H, W], "counts": c})), c


def test_reference_vectors(cuda, gold):
    """every r{j}_counts of the reference's maskApi.c vectors -> r{j}_mask with status (0, area); the same from r_strings"""
    strs = [str(s) for s in gold["r_strings"]]
    for j in range(int(gold["n_rle"][0])):
        H, W = (int(v) for v in gold[f"r{j}_size"])
        want = gold[f"r{j}_mask"] != 0
        masks, status = decode_counts([gold[f"r{j}_counts"]], H, W, cuda)
        assert np.array_equal(masks[0] != 0, want), j
        assert status[0].tolist() == [0, int(want.sum()), 0, 0], j
        for counts in (strs[j], strs[j].encode("ascii"), gold[f"r{j}_counts"].tolist()):
            got = hsam.rles_to_masks([{"size": [H, W], "counts": counts}], device=cuda)
            assert got.dtype == torch.bool and tuple(got.shape) == (1, H, W) and got.is_cuda
            assert np.array_equal(got[0].cpu().numpy(), want), j


def test_rles_to_masks_batch_and_errors(cuda, gold):
    H, W = 33, 5
    batch = blobs(5, H, W, seed=2)
    rles = [hsam.mask_to_rle(m) for m in batch]
    rles[1] = hsam.coco_encode_rle(rles[1])
    got = hsam.rles_to_masks(rles, device=cuda)
    assert np.array_equal(got.cpu().numpy(), batch != 0)
    bad = list(rles)
    bad[3] = {"size": [H, W], "counts": [5, 2]}
    with pytest.raises(ValueError, match="entry 3"):
        hsam.rles_to_masks(bad, device=cuda)
    bad[3] = {"size": [H, W + 1], "counts": [H * (W + 1)]}
    with pytest.raises(ValueError, match="entry 3"):
        hsam.rles_to_masks(bad, device=cuda)


def test_fuzz(cuda):
    """the 120 masks of the host codec's fuzz (sizes 1 .. 299, blobs and noise) from their packed counts"""
    for t, m in enumerate(GG.fuzz_rle_masks()):
        H, W = m.shape
        counts = hsam.mask_to_rle(m)["counts"]
        masks, status = decode_counts([counts], H, W, cuda, spare=64)
        assert np.array_equal(masks[0], m), (t, H, W)
        assert status[0].tolist() == [0, int(m.sum()), 0, 0], t


SIZES = [(1, 1), (1, 70), (70, 1), (33, 5), (63, 64), (64, 63), (65, 129), (100, 37), (129, 260)]


@pytest.mark.parametrize("H,W", SIZES)
def test_edge_masks(cuda, H, W):
    """H = 63 / 64 / 65 sit on the column-word edge, 70 and 260 exceed one column tile on the narrow and the wide store path;
    the checkerboards have H*W (+ 1) counts: many 256-count chunks, in a slot of H*W + 1 words"""
    cases = edge_masks(H, W)
    batch = np.stack(list(cases.values()))
    counts = [hsam.mask_to_rle(m)["counts"] for m in batch]
    assert max(len(c) for c in counts) == (H * W + 1 if H & 1 else H * W + 2 - W)      # even H: equal pixels meet at the column boundaries
    for c, m in zip(counts, batch):
        assert np.array_equal(G.counts_to_mask(c, H, W), m)
    masks, status = decode_counts(counts, H, W, cuda, slot_words=H * W + 1)
    for i, name in enumerate(cases):
        assert np.array_equal(masks[i], batch[i]), (name, H, W)
        assert status[i].tolist() == [0, int(batch[i].sum()), 0, 0], (name, H, W)
    # the same masks through the device encoder's default slot: the checkerboards arrive as bit planes
    slots, table = ops.rle_encode(torch.from_numpy(batch).to(cuda))
    masks, status = decode(slots, table, H, W)
    assert np.array_equal(masks, batch)
    assert status[:, 0].tolist() == [0] * len(batch) and status[:, 1].tolist() == batch.reshape(len(batch), -1).sum(1).tolist()


@pytest.mark.parametrize("H,W", [(130, 70), (65, 129), (96, 128)])
def test_encode_then_decode_on_the_device(cuda, H, W):
    """ops.rle_encode -> ops.rle_decode with the default slot and no host in between: noise arrives as form 1, blobs as form 0
    (a blob of few columns certainly: two runs per column)"""
    batch = blobs(6, H, W, seed=H)
    batch[0] = 0
    batch[0, H // 4:H // 2, 2:5] = 1
    rng = np.random.default_rng(W)
    batch[1] = (rng.random((H, W)) < 0.5).astype(np.uint8)
    batch[4] ^= (rng.random((H, W)) < 0.4).astype(np.uint8)
    batch[2] *= 255      # any non-zero byte is foreground
    t = torch.from_numpy(batch).to(cuda)
    slots, table = ops.rle_encode(t)
    masks, status = decode(slots, table, H, W)
    tab = table.cpu().numpy()
    assert set(tab[:, 1].tolist()) == {0, 1}      # both forms occurred
    assert np.array_equal(masks, (batch != 0).astype(np.uint8))
    assert status[:, 0].tolist() == [0] * 6 and np.array_equal(status[:, 1], tab[:, 2])
    assert (status[:, 2:] == 0).all()


def test_selection_with_an_index_out_of_range(cuda):
    H, W = 20, 24
    batch = blobs(3, H, W, seed=21)
    order = [2, -1, 3, 1, 0]
    slots, table = ops.rle_encode(torch.from_numpy(batch).to(cuda), torch.tensor(order, dtype=torch.int64, device=cuda))
    masks, status = decode(slots, table, H, W)
    for s, n in enumerate(order):
        if 0 <= n < 3:
            assert np.array_equal(masks[s], batch[n]) and status[s].tolist() == [0, int(batch[n].sum()), 0, 0], s
        else:
            assert not masks[s].any() and status[s].tolist() == [2, 0, 0, 0], s


@pytest.mark.parametrize("H,W", [(4, 4), (33, 5)])
def test_malformed_and_unusual_counts(cuda, H, W):
    HW = H * W
    cases = [([], 1), ([HW], 0), ([0, HW], 0), ([3, 0, 0, 2, 0, 4, HW - 9], 0), ([0, 0, 0, 3, 0, 0, 2, HW - 5, 0], 0),
             ([5, HW - 6], 1), ([5, 2, HW], 1), ([0xFFFFFFFF, 5], 1), ([2, 0xFFFFFFFF, 0xFFFFFFFF, 7], 1)]
    assert sum(cases[5][0]) == HW - 1 and sum(cases[6][0]) == HW + 7
    masks, status = decode_counts([c for c, _ in cases], H, W, cuda)
    for i, (c, code) in enumerate(cases):
        want = G.counts_to_mask(c, H, W)
        assert np.array_equal(masks[i], want), c
        assert status[i].tolist() == [code, int(want.sum()), 0, 0], c
    assert not masks[0].any() and not masks[1].any() and masks[2].all() and not masks[7].any()
    # table rows that name no mask: zeros, code 2 -- and the neighbours stay exact
    good = hsam.mask_to_rle(blobs(1, H, W, seed=3)[0])["counts"]
    slots, table = ops.rle_pack([good] * 7, H, W, device=cuda)
    sw = int(slots.shape[1])
    table[1, 0] = sw + 1
    table[2, 0] = -1
    for row, form in ((3, 2), (4, 3), (5, 7)):
        table[row, 1] = form
    masks, status = decode(slots, table, H, W)
    want = G.counts_to_mask(good, H, W)
    for i in range(7):
        if i in (0, 6):
            assert np.array_equal(masks[i], want) and status[i].tolist() == [0, int(want.sum()), 0, 0]
        else:
            assert not masks[i].any() and status[i].tolist() == [2, 0, 0, 0], i
    # form 1 in a slot that cannot hold the plane is no mask either (nothing is read beyond the slot)
    slots, table = ops.rle_pack([[HW]], H, W, slot_words=(HW + 31) // 32 - 1 or 1, device=cuda)
    if int(slots.shape[1]) < (HW + 31) // 32:
        table[0, 1] = 1
        masks, status = decode(slots, table, H, W)
        assert not masks.any() and status[0].tolist() == [2, 0, 0, 0]


def test_form_1_ignores_bits_beyond_the_image(cuda):
    H, W = 33, 5      # 165 pixels: 6 words, 27 spare bits in the last
    m = blobs(1, H, W, seed=9)[0]
    flat = np.concatenate([m.T.reshape(-1), np.ones(27, np.uint8)])
    words = np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)
    slots = torch.from_numpy(words.view(np.int32).reshape(1, 6).copy()).to(cuda)
    table = torch.tensor([[99, 1, 0, 0]], dtype=torch.int32, device=cuda)
    masks, status = decode(slots, table, H, W)
    assert np.array_equal(masks[0], m) and status[0].tolist() == [0, int(m.sum()), 0, 0]


def test_unaligned_output_takes_the_narrow_path(cuda):
    """W % 4 == 0 with the output at an odd byte offset: byte stores, same masks, nothing outside"""
    H, W = 65, 260
    batch = blobs(3, H, W, seed=41)
    counts = [hsam.mask_to_rle(m)["counts"] for m in batch]
    for offset in (0, 1, 3):
        masks, status = decode_counts(counts, H, W, cuda, offset=offset)
        assert np.array_equal(masks, batch), offset
        assert status[:, 1].tolist() == batch.reshape(3, -1).sum(1).tolist()


def test_launch_counts(cuda):
    """a single-size decode is the group decode of one image: the same two kernel functions and the same instantiation of the
    rows kernel (the starts kernels differ by design: only the group entry's keeps the box); the IoU launches five"""
    import abi_ref
    H, W = 65, 63
    batch = blobs(10, H, W, seed=51)
    slots, table = ops.rle_pack([hsam.mask_to_rle(m)["counts"] for m in batch], H, W, device=cuda)
    single = abi_ref.rle_kernels(lambda: ops.rle_decode(slots, table, H, W))
    group = abi_ref.rle_kernels(lambda: ops.rle_decode_group(slots, table, [(H, W)], [10]))
    assert [k for k, _ in single] == ["rle_starts_kernel", "rle_rows_kernel"], single
    assert [k for k, _ in group] == [k for k, _ in single] and group[1] == single[1] == ("rle_rows_kernel", "1"), (single, group)
    iou = abi_ref.rle_kernels(lambda: ops.rle_iou(slots, table, slots, table, H, W))
    assert [k for k, _ in iou] == ["rle_starts_kernel", "rle_plane_kernel"] * 2 + ["rle_iou_kernel"], iou


def test_two_calls_give_identical_bytes(cuda):
    H, W = 130, 70
    batch = blobs(4, H, W, seed=31)
    batch[1] ^= (np.random.default_rng(32).random((H, W)) < 0.4).astype(np.uint8)
    slots, table = ops.rle_encode(torch.from_numpy(batch).to(cuda))
    a = decode(slots, table, H, W)
    b = decode(slots, table, H, W)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    x = ops.rle_iou(slots, table, slots.flip(0).contiguous(), table.flip(0).contiguous(), H, W).cpu().numpy()
    y = ops.rle_iou(slots, table, slots.flip(0).contiguous(), table.flip(0).contiguous(), H, W).cpu().numpy()
    assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("H,W", [(100, 37), (65, 129)])
def test_rle_iou(cuda, H, W):
    a, b = blobs(8, H, W, seed=H), blobs(8, H, W, seed=W)
    b[5] = 0
    a[6] = (np.random.default_rng(7).random((H, W)) < 0.5).astype(np.uint8)      # form 1 from the encoder's default slot
    # 4 x the plane's words: every blob fits as runs (at most 6 per column), the noise (about H*W/2 runs) only as a bit plane
    sa, ta = ops.rle_encode(torch.from_numpy(a).to(cuda), slot_words=4 * ops.rle_slot_words(H, W))
    sb, tb = ops.rle_pack([hsam.mask_to_rle(m)["counts"] for m in b], H, W, device=cuda)      # form 0, another slot size
    assert ta.cpu().numpy()[:, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and sa.shape[1] != sb.shape[1]
    iu = ops.rle_iou(sa, ta, sb, tb, H, W)
    assert iu.dtype == torch.int64 and tuple(iu.shape) == (8, 2) and iu.is_cuda
    want = [[int((x & y).sum()), int((x | y).sum())] for x, y in zip(a, b)]
    assert iu.cpu().numpy().tolist() == want
    assert want[5] == [0, int(a[5].sum())]      # A against zeros
    assert ops.rle_iou(sb, tb, sa, ta, H, W).cpu().numpy().tolist() == want
    areas = a.reshape(8, -1).sum(1)
    assert ops.rle_iou(sa, ta, sa, ta, H, W).cpu().numpy().tolist() == [[int(v), int(v)] for v in areas]
    # an entry that holds no mask, on either side
    t2 = tb.clone()
    t2[2, 1] = 3
    t2[4, 0] = -1
    for got in (ops.rle_iou(sa, ta, sb, t2, H, W), ops.rle_iou(sb, t2, sa, ta, H, W)):
        got = got.cpu().numpy().tolist()
        assert got[2] == [-1, -1] and got[4] == [-1, -1]
        assert [g for i, g in enumerate(got) if i not in (2, 4)] == [w for i, w in enumerate(want) if i not in (2, 4)]
    # counts that stop short of H*W count as decoded (clipped, the rest background)
    short = [c[:-1] if len(c) > 1 else c for c in (hsam.mask_to_rle(m)["counts"] for m in b)]
    ss, ts = ops.rle_pack(short, H, W, device=cuda)
    clipped = np.stack([G.counts_to_mask(c, H, W) for c in short])
    assert ops.rle_iou(sa, ta, ss, ts, H, W).cpu().numpy().tolist() == [[int((x & y).sum()), int((x | y).sum())]
                                                                         for x, y in zip(a, clipped)]


def test_rle_pack(cuda):
    lists = [[12], np.array([0, 12], np.uint32), [1, 2, 3, 6], [], [0xFFFFFFFF, 5]]
    slots, table = ops.rle_pack(lists, 3, 4, device=cuda)
    assert slots.dtype == torch.int32 and table.dtype == torch.int32 and slots.is_cuda and table.is_cuda
    assert tuple(slots.shape) == (5, 4) and tuple(table.shape) == (5, 4)      # the longest list
    t, s = table.cpu().numpy(), slots.cpu().numpy().view(np.uint32)
    assert t[:, 0].tolist() == [1, 2, 4, 0, 2] and (t[:, 1] == 0).all()
    for i, c in enumerate(lists):
        assert s[i, :len(c)].tolist() == [int(v) for v in c]
    slots, table = ops.rle_pack(lists, 3, 4, slot_words=9, device=cuda)
    assert tuple(slots.shape) == (5, 9)
    with pytest.raises(ValueError, match="entry 2"):
        ops.rle_pack(lists, 3, 4, slot_words=3, device=cuda)
    masks, status = ops.rle_decode(slots, table, 3, 4)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (5, 3, 4) and status.cpu().numpy()[:, 0].tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(ValueError):
        ops.rle_decode(slots, table, 3, 4, out=torch.empty(5 * 3 * 4 + 1, dtype=torch.uint8, device=cuda))


def test_entry_refuses_what_it_cannot_hold(cuda):
    from hybridgl_amd import _lib
    lib = _lib.load()
    slots, table = ops.rle_pack([[16]], 4, 4, device=cuda)
    out = torch.empty(16, dtype=torch.uint8, device=cuda)
    status = torch.empty((1, 4), dtype=torch.int32, device=cuda)
    ws = ops.workspace(lib.hgl_rle_decode_workspace_bytes(1, 4, 4, 1), cuda, "rle")
    args = (slots.data_ptr(), 1, table.data_ptr(), 1)
    assert lib.hgl_rle_decode_device(*args, 4, 4, out.data_ptr(), status.data_ptr(), ws.data_ptr(), 8, None) == -3
    assert lib.hgl_rle_decode_device(*args, 1 << 16, 1 << 15, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert b"2^31" in lib.hgl_last_error()
    iu = torch.empty((1, 2), dtype=torch.int64, device=cuda)
    assert lib.hgl_rle_iou_device(*args[:3], *args[:3], 1, 4, 4, iu.data_ptr(), ws.data_ptr(), 8, None) == -3
    assert lib.hgl_rle_iou_device(*args[:3], *args[:3], 1, 1 << 16, 1 << 15, iu.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
