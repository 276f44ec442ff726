"""hgl_rle_select_device (csrc/rle.hip) on the GPU: the stable per-image compaction of an encoded set.  The entry moves bits, so
every comparison is equality: the C entry on fenced, pre-filled buffers against the numpy statement of the contract
(tests/rle_select_cases.py) applied to buffers filled the same way -- so a word the call must not write is a word that kept its
fill -- over entry counts that cross every boundary of the rank kernel's scan, every keep pattern, max_keep around the number
kept, both slot forms, both move paths (16-byte and dword, a slot longer than one chunk, a base 4 bytes off), 0 .. 8 side
columns and an entry that holds no mask; and ops.rle_select driven by ops.rle_nms on the lists of the golden file
(tests/golden/rle_nms_fuzz.npz): the survivors are the stored keep flags', and the decode of the compacted set is the decode of
the source, gathered."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops

import rle_nms_cases as NC
import rle_select_cases as SC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 64
SIZES8 = [(4, 4), (5, 3), (4, 4), (9, 2), (3, 7), (6, 6), (4, 4), (2, 2)]
COUNTS8 = [1, 63, 64, 0, 65, 130, 4096, 2]      # every boundary of the scan: a wave, a chunk of 256, the per-image limit; none mid-group
PATTERNS = ["none", "all", "first", "last", "alternating", "random"]


def make_set(sizes, counts, sw, seed, dead=True):
    """(slots [S,sw] uint32 of random words, table [S,4] int32) with rows of form 0 (any count the slot holds, 0 included), of
    form 1 where the plane fits, and -- `dead` -- an entry of form 2 in the middle of every list of three or more"""
    rng = np.random.default_rng(seed)
    S = sum(counts)
    slots = rng.integers(0, 1 << 32, (S, sw), dtype=np.uint64).astype(np.uint32)
    table = np.zeros((S, 4), np.int32)
    table[:, 0] = rng.integers(0, sw + 1, S)
    table[:, 2:] = rng.integers(0, 1 << 20, (S, 2))
    e = 0
    for (H, W), n in zip(sizes, counts):
        if (H * W + 31) // 32 <= sw:
            table[e:e + n, 1] = rng.integers(0, 2, n)
        if dead and n >= 3:
            table[e + n // 2, :2] = (int(rng.integers(0, sw + 1)), 2)
        e += n
    return slots, table


def pattern(name, counts, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        k = np.zeros(n, np.uint8)
        if name == "all":
            k[:] = 1
        elif name == "first":
            k[:1] = 1
        elif name == "last":
            k[n - 1:] = 7      # any nonzero byte keeps
        elif name == "alternating":
            k[::2] = 1
        elif name == "random":
            k[:] = rng.integers(0, 2, n)
        out.append(k)
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def raw(slots, table, images, keep, nms, cols, fill, device, offset=0):
    """the C entry on destination buffers pre-filled with `fill` and fenced by guard words; offset: 4-byte words by which both
    slot buffers' bases are moved off their allocation.  -> (rc, (out_slots, out_table, out_cols, out_src, out_n), fences intact)"""
    lib = _lib.load()
    S, sw = slots.shape
    C, G = (0 if cols is None else cols.shape[0]), len(images)
    images = np.ascontiguousarray(images, dtype=np.int64)
    # (an empty tensor has no address: a set without an entry still names its selector, by a byte nobody reads)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))).to(device)
    d_slots = torch.zeros(S * sw + offset + 4, dtype=torch.int32, device=device)
    if S:
        d_slots[offset:offset + S * sw] = up(slots.view(np.int32).reshape(-1))
    d_table, d_keep, d_nms, d_cols = up(table), up(keep), up(nms), up(None if C == 0 else cols.view(np.int32))
    sizes = [S * sw, 4 * S, C * S, S, G]
    bufs = [torch.full((n + 2 * GUARD + offset,), fill, dtype=torch.int32, device=device) for n in sizes]
    ptr = lambda t: None if t is None else t.data_ptr()
    outs = [b.data_ptr() + 4 * GUARD + (4 * offset if k == 0 else 0) for k, b in enumerate(bufs)]
    if C == 0:
        outs[2] = None
    rc = lib.hgl_rle_select_device(d_slots.data_ptr() + 4 * offset, sw, ptr(d_table), S, images.ctypes.data, G, ptr(d_keep), ptr(d_nms),
                                   ptr(d_cols), C, *outs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    fences = all((h[:GUARD + (offset if k == 0 else 0)] == fill).all() and (h[len(h) - GUARD:] == fill).all() for k, h in enumerate(host))
    o = [h[GUARD + (offset if k == 0 else 0):][:n] for k, (h, n) in enumerate(zip(host, sizes))]
    return rc, (o[0].view(np.uint32).reshape(S, sw), o[1].reshape(S, 4), o[2].view(np.uint32).reshape(C, S), o[3], o[4]), fences


def statement(slots, table, images, keep, cols, fill):
    S, sw = slots.shape
    C = 0 if cols is None else cols.shape[0]
    cols = np.zeros((0, S), np.uint32) if cols is None else cols
    init = [np.full((S, sw), fill, np.uint32), np.full((S, 4), fill, np.int32), np.full((C, S), fill, np.uint32),
            np.full(S, fill, np.int32), np.full(len(images), fill, np.int32)]
    return SC.select(slots, table, images, keep, cols, *init)


def agree(got, want, where):
    for a, b, what in zip(got, want, ("out_slots", "out_table", "out_cols", "out_src", "out_n")):
        assert np.array_equal(a, b), (where, what)


def columns(C, S, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (C, S), dtype=np.uint64).astype(np.uint32) if C else None


@pytest.mark.parametrize("sw,C,offset", [(8, 0, 0), (7, 1, 0), (8, 3, 0), (7, 8, 0), (8, 8, 1), (1, 2, 0)],
                         ids=["wide-c0", "odd-c1", "wide-c3", "odd-c8", "wide-stride-base-off-c8", "one-word-c2"])
def test_eight_images_every_pattern(sw, C, offset, cuda):
    """G = 8 with an image that owns none in mid-group; slot_words a multiple of 4 with aligned bases (the 16-byte path), odd (the
    dword path), and a multiple of 4 behind a base 4 bytes off (the dword path with an aligned stride)"""
    slots, table = make_set(SIZES8, COUNTS8, sw, 5)
    S = len(table)
    images = ops.rle_select_layout(SIZES8, COUNTS8).tolist()
    cols = columns(C, S, 6)
    assert SC.plan(images, S, sw, C, 1, 0, 4 * offset, (1 << 40) + 4 * offset)[0][2] == int(sw % 4 == 0 and offset == 0)
    moved = 0
    for name in PATTERNS:
        keep = pattern(name, COUNTS8)
        rc, got, fences = raw(slots, table, images, keep, None, cols, 0x11111111, cuda, offset)
        assert rc == 0 and fences, name
        want = statement(slots, table, images, keep, cols, 0x11111111)
        agree(got, want, name)
        e = 0
        for n, k in zip(COUNTS8, got[4]):
            assert k == {"none": 0, "all": n, "first": min(n, 1), "last": min(n, 1), "alternating": (n + 1) // 2}.get(name, k)
            e += n
        moved += int(got[4].sum())
    assert moved > S


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 255, 256, 257, 4096])
def test_one_image_alone(n, cuda):
    """G = 1 at every count where the scan takes another step"""
    slots, table = make_set([(4, 4)], [n], 4, n)
    images = [[4, 4, 0, -1]]
    cols = columns(2, n, n + 1)
    for name in ("random", "all", "last"):
        keep = pattern(name, [n], seed=n)
        rc, got, fences = raw(slots, table, images, keep, None, cols, 0x22222222, cuda)
        assert rc == 0 and fences
        agree(got, statement(slots, table, images, keep, cols, 0x22222222), (n, name))
        if n == 0:      # nothing is launched: out_n is the caller's
            assert got[4].tolist() == [0x22222222]


def test_max_keep_around_the_number_kept(cuda):
    slots, table = make_set(SIZES8, COUNTS8, 8, 9)
    S = len(table)
    keep = pattern("random", COUNTS8, seed=4)
    cols = columns(2, S, 10)
    kept, e = [], 0
    for n in COUNTS8:
        kept.append(int(keep[e:e + n].sum()))
        e += n
    assert kept[6] > 1000 and kept[3] == 0
    for what, limits in {"0": [0] * 8, "1": [1] * 8, "k-1": [max(k - 1, 0) for k in kept], "k": kept, "k+1": [k + 1 for k in kept],
                         "-1": [-1] * 8, "mixed": [-1, 5, 64, 3, 0, 65, 1025, 1]}.items():
        images = ops.rle_select_layout(SIZES8, COUNTS8, limits).tolist()
        rc, got, fences = raw(slots, table, images, keep, None, cols, 0x33333333, cuda)
        assert rc == 0 and fences, what
        agree(got, statement(slots, table, images, keep, cols, 0x33333333), what)
        assert got[4].tolist() == [min(k, m) if m >= 0 else k for k, m in zip(kept, limits)], what
        # the first max_keep of the kept list, in stored order
        e = 0
        for n, k in zip(COUNTS8, got[4]):
            assert got[3][e:e + k].tolist() == np.flatnonzero(keep[e:e + n])[:k].tolist()
            e += n


@pytest.mark.parametrize("sw,offset", [(2060, 0), (2061, 0), (2060, 3)], ids=["wide", "odd", "wide-stride-base-off"])
def test_slots_longer_than_one_chunk(sw, offset, cuda):
    """256 x 257 entries: a plane of 2056 words and run lists of any length up to the slot -- past the 2048 words of a move
    chunk, with the counts that end just before, at and just behind the boundary"""
    sizes, counts = [(256, 257), (4, 4), (256, 257)], [9, 3, 5]
    slots, table = make_set(sizes, counts, sw, 21, dead=False)
    table[:6, 0] = (2047, 2048, 2049, 2050, 2051, sw)
    table[:6, 1] = 0
    table[6:9, 1] = 1
    table[13, :2] = (sw + 1, 0)      # more counts than the slot holds: no mask, the row moves alone
    images = ops.rle_select_layout(sizes, counts).tolist()
    cols = columns(1, len(table), 22)
    for name in ("all", "alternating"):
        keep = pattern(name, counts)
        a = raw(slots, table, images, keep, None, cols, 0x11111111, cuda, offset)
        b = raw(slots, table, images, keep, None, cols, 0x77777777, cuda, offset)
        assert a[0] == b[0] == 0 and a[2] and b[2]
        wa, wb = statement(slots, table, images, keep, cols, 0x11111111), statement(slots, table, images, keep, cols, 0x77777777)
        agree(a[1], wa, name)
        agree(b[1], wb, name)
        # two calls into differently filled buffers: the same defined bytes (where the statements agree), the fill elsewhere
        for x, y, p, q in zip(a[1], b[1], wa, wb):
            same = p == q
            assert np.array_equal(x[same], y[same]) and (x[~same] == 0x11111111).all() and (y[~same] == 0x77777777).all()
        assert (~(wa[0] == wb[0])).sum() > 0 and (wa[0] == wb[0]).sum() > 4 * 2048


def test_an_entry_that_holds_no_mask_and_the_refusals(cuda):
    sizes, counts, sw = [(4, 4), (6, 5)], [5, 4], 4
    slots, table = make_set(sizes, counts, sw, 30, dead=False)
    table[2] = (3, 2, 77, 78)      # code 2 in mid-list ...
    slots[2] = POISON              # ... with a poisoned slot
    images = ops.rle_select_layout(sizes, counts).tolist()
    cols = columns(3, 9, 31)
    keep = np.ones(9, np.uint8)
    rc, got, fences = raw(slots, table, images, keep, None, cols, 0x44444444, cuda)
    assert rc == 0 and fences
    agree(got, statement(slots, table, images, keep, cols, 0x44444444), "keep")
    assert got[1][2].tolist() == [3, 2, 77, 78] and (got[0][2] == 0x44444444).all() and not (got[0] == POISON).any()
    # through an NMS result the entry is not kept: code 2; neither is a suppressed one
    nms = np.zeros((9, 4), np.int32)
    nms[:, 3] = -1
    nms[2] = (2, 0, -1, -1)
    nms[1, 0] = 1      # code 1 counts as decoded
    nms[4, 3] = 0
    nms[7] = (3, 0, -1, -1)
    rc, got, fences = raw(slots, table, images, None, nms, cols, 0x44444444, cuda)
    assert rc == 0 and fences
    agree(got, statement(slots, table, images, SC.kept_from_nms(nms), cols, 0x44444444), "nms_result")
    assert got[3].tolist() == [0, 1, 3, -1, -1, 0, 1, 3, -1] and got[4].tolist() == [3, 3]
    assert got[1][3].tolist() == [1, 0, 0, 0] and got[0][3, 0] == 16 and got[0][8, 0] == 30 and (got[0][3, 1:] == 0x44444444).all()
    assert (got[2][:, [3, 4, 8]] == 0).all()
    # refused: nothing is enqueued, so nothing is written
    lib = _lib.load()
    for what, kw in {"both": dict(keep=keep, nms=nms), "neither": dict(keep=None, nms=None),
                     "entries step back": dict(keep=keep, nms=None, images=[images[1], images[0]]),
                     "4097 entries": dict(keep=np.ones(4097, np.uint8), nms=None, images=[[4, 4, 0, -1]],
                                          slots=np.zeros((4097, 1), np.uint32), table=np.zeros((4097, 4), np.int32), cols=None)}.items():
        rc, got, fences = raw(kw.get("slots", slots), kw.get("table", table), kw.get("images", images), kw["keep"], kw["nms"],
                              kw.get("cols", cols), 0x55555555, cuda)
        assert rc == -1 and fences, what
        assert all((g.view(np.uint32) == 0x55555555).all() for g in got), what
    d = torch.zeros(9 * sw + 9 * 4 + 16, dtype=torch.int32, device=cuda)
    flags = torch.ones(9, dtype=torch.uint8, device=cuda)
    im = np.asarray(images, dtype=np.int64)
    st = torch.cuda.current_stream().cuda_stream
    s0, t0 = d.data_ptr(), d.data_ptr() + 4 * 9 * sw
    side = torch.zeros(64, dtype=torch.int32, device=cuda)
    for what, (os_, ot_) in {"out_slots overlaps slots": (s0 + 4 * (9 * sw - 1), side.data_ptr()),
                             "out_table overlaps table": (side.data_ptr(), t0 + 16)}.items():
        rc = lib.hgl_rle_select_device(s0, sw, t0, 9, im.ctypes.data, 2, flags.data_ptr(), None, None, 0, os_, ot_, None,
                                       side.data_ptr(), side.data_ptr(), st)
        assert rc == -1 and what.encode() in lib.hgl_last_error(), what
    torch.cuda.synchronize()
    assert not d.any() and not side.any()
    # ops: one selector, 4-byte columns; no entry -> no launch, zero counts
    ds, dt = torch.from_numpy(slots.view(np.int32)).to(cuda), torch.from_numpy(table).to(cuda)
    with pytest.raises(ValueError):
        ops.rle_select(ds, dt, sizes, counts)
    with pytest.raises(ValueError):
        ops.rle_select(ds, dt, sizes, counts, keep=flags, nms_result=torch.from_numpy(nms).to(cuda))
    with pytest.raises(ValueError):
        ops.rle_select(ds, dt, sizes, counts, keep=flags, cols=torch.zeros((1, 9), dtype=torch.float64, device=cuda))
    o = ops.rle_select(ds[:0], dt[:0], [(4, 4), (5, 5)], [0, 0], keep=flags[:0])
    assert o[0].numel() == 0 and o[3].numel() == 0 and o[4].cpu().tolist() == [0, 0]
    # ops against the statement, bool flags and float columns
    fcols = torch.from_numpy(cols[:2].view(np.float32).copy()).to(cuda)
    o = ops.rle_select(ds, dt, sizes, counts, keep=torch.from_numpy(SC.kept_from_nms(nms)).to(cuda), cols=fcols, max_keep=[2, None])
    want = statement(slots, table, ops.rle_select_layout(sizes, counts, [2, None]).tolist(), SC.kept_from_nms(nms), cols[:2], 0)
    assert o[2].dtype == torch.float32 and np.array_equal(o[2].cpu().numpy().view(np.uint32), want[2])
    assert np.array_equal(o[1].cpu().numpy(), want[1]) and o[3].cpu().tolist() == want[3].tolist() == [0, 1, -1, -1, -1, 0, 1, 3, -1]
    assert o[4].cpu().tolist() == [2, 3]


# ---- driven by the mask NMS, on the lists of the golden file
_src = {}


def source(name, masks, form, device):
    """(slots, table, the decode of the set [n,H,W] on the host, its status), once per list and form"""
    key = (name, form)
    if key not in _src:
        n, H, W = masks.shape
        s, t = ops.rle_encode(torch.from_numpy(masks).to(device), slot_words=H * W + 1 if form == 0 else ops.rle_slot_words(H, W))
        s, t = s.contiguous(), t.contiguous()
        dec, _, status = ops.rle_decode_group(s, t, [(H, W)], [n])
        dec = dec[0].cpu().numpy()
        assert np.array_equal(dec, masks)
        _src[key] = (s, t, dec)
    return _src[key]


@pytest.mark.parametrize("form", [0, 1])
def test_driven_by_the_mask_nms_on_the_golden_lists(form, cuda):
    z = NC.golden()
    checked = placeholders = 0
    for name, H, W, masks, scores in NC.sets():
        n = len(masks)
        s, t, dec = source(name, masks, form, cuda)
        dscores = torch.from_numpy(scores).to(cuda)
        iou = torch.arange(n, dtype=torch.float32, device=cuda) / 7
        cols = torch.stack([iou, -iou]).contiguous()
        for thr in (0.0, 0.5, 1.0):
            for scored in (False, True):
                out_idx, out_n, result = ops.rle_nms(s, t, [(H, W)], [n], dscores if scored else None, thr)
                cs, ct, cc, src, k = ops.rle_select(s, t, [(H, W)], [n], nms_result=result, cols=cols)
                pix, boxes, status = ops.rle_decode_group(cs, ct, [(H, W)], [n])
                k = int(k.cpu()[0])
                src, status, pix = src.cpu().numpy(), status.cpu().numpy(), pix[0].cpu().numpy()
                where = (name, thr, scored)
                assert k == int(out_n.cpu()[0]) and src[:k].tolist() == sorted(out_idx.cpu().numpy()[:k].tolist()), where
                if name + "_keep" in z:      # the sorted kept set of the stored flags
                    flags = z[name + "_keep"][np.flatnonzero(z[name + "_thr"] == thr)[0], int(scored)]
                    assert src[:k].tolist() == np.flatnonzero(flags).tolist(), where
                    checked += 1
                assert (src[k:] == -1).all()
                # the decode of the output is the decode of the source, gathered; placeholders are empty code-0 masks
                assert np.array_equal(pix[:k], dec[src[:k]]), where
                assert not pix[k:].any() and (status[:, 0] == 0).all() and (status[k:, 1] == 0).all(), where
                assert np.array_equal(status[:k, 1], dec[src[:k]].reshape(k, -1).sum(1)), where
                assert np.array_equal(cc.cpu().numpy()[:, :k], cols.cpu().numpy()[:, src[:k]]) and not cc[:, k:].any()
                assert np.array_equal(ct.cpu().numpy()[:k], t.cpu().numpy()[src[:k]])
                placeholders += n - k
    assert checked == 8 * 3 * 2 and placeholders > 200
    if form == 1:
        assert any((source(name, masks, 1, cuda)[1][:, 1] == 1).any() for name, _, _, masks, _ in NC.sets("se"))
