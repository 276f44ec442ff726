"""hgl_rle_match_device (csrc/rle.hip) through ops.rle_match: every mask of one encoded set against every mask of another, image
by image.  Integer equality, no tolerance: the intersections, the areas, the best partners and their counts equal a dense
int64 count (A.reshape(na,-1) @ B.reshape(nb,-1).T) with the tie rule applied in Python integers -- on the shapes at which the
word layout, the tiles and the chunks change, on both slot forms, on every kind of entry the decoder knows; the crowd flags
and the ratios against the reference's rleIou (tests/golden/rle_match_fuzz.npz); groups against per-image calls byte for byte;
the contract of the entry (workspace, refused geometry, containment with guard words, determinism)."""
import os

import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops
from hybridgl_amd import sam as hsam

pytestmark = pytest.mark.gpu

SHAPES = [(70, 37, 19, 23), (64, 64, 17, 33), (3, 50, 3, 5), (129, 5, 40, 9)]
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rle_match_fuzz.npz"))


# ---- entries: ("mask", m, form) a mask in slot form 0 / 1; ("counts", list) raw counts (code 1 when they miss H*W); ("dead",)
def decode_counts(counts, H, W):
    """the decoder's rule: positions summed without wrap, runs clipped at H*W, pixels past the last run 0"""
    HW = H * W
    flat = np.zeros(HW, np.uint8)
    p = 0
    for j, c in enumerate(counts):
        e = min(p + int(c), HW)
        if j & 1:
            flat[p:e] = 1
        p = e
    return flat.reshape(W, H).T.copy(), (0 if sum(int(c) for c in counts) == HW else 1)


def build_set(entries, H, W, device):
    """(slots, table) on the device and the host's view of them: masks [n,H,W], codes [n]"""
    HW = H * W
    pw = (HW + 31) // 32
    rows, masks, codes = [], [], []
    for e in entries:
        if e[0] == "dead":
            rows.append((np.zeros(0, np.uint32), 5, 2))
            masks.append(np.zeros((H, W), np.uint8))
            codes.append(2)
        elif e[0] == "counts":
            m, code = decode_counts(e[1], H, W)
            rows.append((np.asarray(e[1], dtype=np.uint32), len(e[1]), 0))
            masks.append(m)
            codes.append(code)
        elif e[2] == 0:
            c = np.asarray(hsam.mask_to_rle(e[1])["counts"], dtype=np.uint32)
            rows.append((c, len(c), 0))
            masks.append(e[1])
            codes.append(0)
        else:
            bits = np.zeros(pw * 32, np.uint8)
            bits[:HW] = e[1].T.reshape(-1)
            bits[HW:] = 1      # bits beyond H*W are ignored
            rows.append((np.packbits(bits, bitorder="little").view(np.uint32), 0, 1))
            masks.append(e[1])
            codes.append(0)
    n = len(rows)
    if n == 0:
        return (torch.zeros((0, 1), dtype=torch.int32, device=device), torch.zeros((0, 4), dtype=torch.int32, device=device),
                np.zeros((0, H, W), np.uint8), np.zeros(0, np.int64))
    sw = max([len(r[0]) for r in rows] + [1])
    slots = np.full((n, sw), 0xFFFFFFFF, np.uint32)      # words beyond what the form defines are never read
    table = np.zeros((n, 4), np.int32)
    for i, (w, cnt, form) in enumerate(rows):
        slots[i, :len(w)] = w
        table[i] = (cnt, form, -7, -7)      # columns 2 and 3 are not read
    return (torch.from_numpy(slots.view(np.int32)).to(device), torch.from_numpy(table).to(device),
            np.stack(masks).astype(np.uint8).reshape(n, H, W), np.asarray(codes, np.int64))


def join(sets, device):
    """per-image (slots, table) sets of their own slot sizes -> one set of the widest slot"""
    sw = max([int(s.shape[1]) for s, _ in sets] + [1])
    slots = [torch.cat([s, torch.zeros((s.shape[0], sw - s.shape[1]), dtype=torch.int32, device=device)], 1) for s, _ in sets]
    return torch.cat(slots).contiguous(), torch.cat([t for _, t in sets]).contiguous()


def expect(ma, ca, mb, cb, crowd=None):
    """(inter [na,nb], match_a [na,4], match_b [nb,4]) of one image from the dense count, in Python integers"""
    na, nb, HW = len(ma), len(mb), ma.shape[1] * ma.shape[2]
    A, B = ma.reshape(na, HW).astype(np.int64), mb.reshape(nb, HW).astype(np.int64)      # (reshape(0, -1) is refused)
    I = A @ B.T
    area_a, area_b = A.sum(1), B.sum(1)
    I[ca == 2, :] = -1
    I[:, cb == 2] = -1
    crowd = np.zeros(nb, bool) if crowd is None else np.asarray(crowd, bool)

    def D(i, j):
        return int(area_a[i]) if crowd[j] else int(area_a[i] + area_b[j] - I[i, j])

    def best(pairs):
        bi, bI, bD = -1, 0, 1
        for idx, (i, j) in enumerate(pairs):
            v = int(I[i, j])
            if v > 0 and (bi < 0 or v * bD > bI * D(i, j)):      # strictly better only: the lowest index keeps a tie
                bi, bI, bD = idx, v, D(i, j)
        return bi, bI

    match_a = np.zeros((na, 4), np.int64)
    match_b = np.zeros((nb, 4), np.int64)
    for i in range(na):
        match_a[i] = (2, 0, -1, 0) if ca[i] == 2 else (ca[i], area_a[i]) + best([(i, j) for j in range(nb)])
    for j in range(nb):
        match_b[j] = (2, 0, -1, 0) if cb[j] == 2 else (cb[j], area_b[j]) + best([(i, j) for i in range(na)])
    return I, match_a, match_b


def run_one(ea, eb, H, W, device, crowd=None, matrix=True):
    sa, ta, ma, ca = build_set(ea, H, W, device)
    sb, tb, mb, cb = build_set(eb, H, W, device)
    cr = None if crowd is None else torch.from_numpy(np.asarray(crowd, np.uint8)).to(device)
    inter, a, b = ops.rle_match(sa, ta, sb, tb, [(H, W)], [len(ea)], [len(eb)], crowd_b=cr, matrix=matrix)
    return inter, a, b, expect(ma, ca, mb, cb, crowd)


def check_one(ea, eb, H, W, device, crowd=None):
    inter, a, b, (I, wa, wb) = run_one(ea, eb, H, W, device, crowd)
    assert inter[0].dtype == torch.int32 and tuple(inter[0].shape) == I.shape
    assert np.array_equal(inter[0].cpu().numpy(), I)
    assert np.array_equal(a.cpu().numpy(), wa), (a.cpu().numpy(), wa)
    assert np.array_equal(b.cpu().numpy(), wb), (b.cpu().numpy(), wb)
    return I, wa, wb


def as_entries(masks, forms):
    return [("mask", m, f) for m, f in zip(masks, forms)]


@pytest.mark.parametrize("forms", ["00", "11", "01", "mixed"])
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_fixture_shapes_in_both_forms(cuda, gold, k, forms):
    H, W, na, nb = SHAPES[k]
    for tag in "se":
        a, b = gold[f"{tag}{k}_a"], gold[f"{tag}{k}_b"]
        fa = [i & 1 for i in range(na)] if forms == "mixed" else [int(forms[0])] * na
        fb = [(i // 2) & 1 for i in range(nb)] if forms == "mixed" else [int(forms[1])] * nb
        I, _, _ = check_one(as_entries(a, fa), as_entries(b, fb), H, W, cuda)
        assert np.array_equal(I, gold[f"{tag}{k}_inter"])      # the reference's rleArea(rleMerge(.., intersect))


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_crowd_flags_and_ratios_against_the_reference(cuda, gold, k):
    """I / D in float64 from the call's exact integers is rleIou's double, bit for bit; the best partner is its arg-max"""
    H, W, na, nb = SHAPES[k]
    a, b = gold[f"s{k}_a"], gold[f"s{k}_b"]
    for crowd, name in ((None, "iou"), (gold[f"s{k}_crowd"], "iou_crowd")):
        I, wa, wb = check_one(as_entries(a, [0] * na), as_entries(b, [1] * nb), H, W, cuda, crowd)
        ref = gold[f"s{k}_{name}"]
        flags = np.zeros(nb, bool) if crowd is None else crowd.astype(bool)
        D = np.where(flags[None, :], wa[:, 1:2] + 0 * wb[None, :, 1], wa[:, 1:2] + wb[None, :, 1] - I)
        assert np.array_equal(np.where(D > 0, I / np.maximum(D, 1), 0.0), ref)
        for i in range(na):
            assert wa[i, 2] == (int(np.argmax(ref[i])) if ref[i].max() > 0 else -1), i
        for j in range(nb):
            assert wb[j, 2] == (int(np.argmax(ref[:, j])) if ref[:, j].max() > 0 else -1), j


def blobs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, ry, rx = rng.random() * H, rng.random() * W, (0.05 + 0.3 * rng.random()) * H + 0.5, (0.05 + 0.3 * rng.random()) * W + 0.5
            out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
    return out


def every_kind(n, H, W, seed):
    """n entries: blobs in both forms and, at fixed places, an empty and a full mask, counts that miss H*W (code 1: too short,
    too long, a count that would wrap 32 bits), zero-length runs, entries that hold no mask (code 2)"""
    HW = H * W
    out = as_entries(blobs(n, H, W, seed), [(i // 3) & 1 for i in range(n)])
    special = [("mask", np.zeros((H, W), np.uint8), 0), ("mask", np.ones((H, W), np.uint8), 1), ("counts", [1, HW + 7]),
               ("dead",), ("counts", [0, 1]), ("counts", [0xFFFFFFFF, 5]), ("counts", [0, 0, 0, 1, 0, 0, 0, HW - 1, 0]), ("dead",),
               ("counts", [2, 0xFFFFFFFF, 0xFFFFFFFF, 7] if HW > 9 else [0, HW]), ("mask", np.ones((H, W), np.uint8), 0)]
    for i, e in enumerate(special):
        if 2 + 3 * i < n:
            out[2 + 3 * i] = e
    return out


# counts on either side of the 32 x 64 tile in both directions; 70 x 37 has 74 plane words, no multiple of the chunk of 32;
# 200 x 9 has 36 (one chunk and a rest of 4); the one-pixel, one-row and one-column images
@pytest.mark.parametrize("H,W,na,nb", [(70, 37, 33, 65), (70, 37, 65, 129), (64, 64, 32, 64), (200, 9, 31, 63), (1, 1, 3, 2),
                                       (1, 40, 5, 7), (40, 1, 7, 5), (3, 50, 1, 1)])
def test_every_kind_of_entry_and_tile_edges(cuda, H, W, na, nb):
    ea, eb = every_kind(na, H, W, 10 * H + W), every_kind(nb, H, W, 20 * H + W)
    crowd = (np.arange(nb) % 3 == 1).astype(np.uint8)
    I, wa, wb = check_one(ea, eb, H, W, cuda, crowd)
    check_one(ea, eb, H, W, cuda, None)
    if na > 11 and nb > 11:
        assert (wa[:, 0] == 1).any() and (wa[:, 0] == 2).any() and (I == -1).any() and (wb[:, 0] == 1).any()
        assert (wa[wa[:, 0] == 2][:, 1:] == (0, -1, 0)).all()
        dead_b = np.flatnonzero(wb[:, 0] == 2)
        assert not np.isin(wa[:, 2], dead_b).any()      # an entry that holds no mask is nobody's best


def test_ties_go_to_the_lowest_index(cuda):
    H, W = 6, 7
    a = np.zeros((2, H, W), np.uint8)
    a[0, 1:3, 1] = 1                                  # 2 pixels
    a[1, 0:4, 4] = 1                                  # 4 pixels
    b = np.zeros((5, H, W), np.uint8)
    b[0, 5, 6] = 1                                    # meets nobody
    b[1, 0:2, 4] = 1                                  # half of a[1]: I = 2, U = 4
    b[2, 1, 1] = 1                                    # half of a[0]: I = 1, U = 2
    b[3] = b[2]                                       # a duplicate of b[2]
    b[4] = b[1]                                       # a duplicate of b[1]
    for fa, fb in ((0, 0), (1, 1), (0, 1)):
        I, wa, wb = check_one(as_entries(a, [fa] * 2), as_entries(b, [fb] * 5), H, W, cuda)
        assert wa[:, 2].tolist() == [2, 1] and wa[:, 3].tolist() == [1, 2]      # 2 before 3, 1 before 4
        assert wb[:, 2].tolist() == [-1, 1, 0, 0, 1] and wb[0, 3] == 0
    # 1/2 against 2/4 in one row: equal ratios, different counts; the lower index wins whichever comes first
    row = np.zeros((1, H, W), np.uint8)
    row[0, 1:3, 1] = 1
    row[0, 0:4, 4] = 1                                # 6 pixels; a crowd partner divides by that area whatever it covers
    for order in ((b[2], b[1]), (b[1], b[2])):
        c = np.stack(order)
        I, wa, wb = check_one(as_entries(row, [0]), as_entries(c, [0, 0]), H, W, cuda, crowd=[1, 1])
        assert sorted(I[0].tolist()) == [1, 2] and wa[0, 2] == int(np.argmax(I[0]))      # 2/6 beats 1/6
    a2 = np.zeros((1, H, W), np.uint8)
    a2[0, 0:2, 0] = 1                                 # area 2
    b2 = np.zeros((2, H, W), np.uint8)
    b2[0, 0, 0] = 1                                   # I = 1, U = 2
    b2[1, 0:2, 0] = 1
    b2[1, 0:2, 1] = 1                                 # I = 2, U = 4
    for order in ((0, 1), (1, 0)):
        I, wa, wb = check_one(as_entries(a2, [0]), as_entries(b2[list(order)], [0, 0]), H, W, cuda)
        assert sorted(I[0].tolist()) == [1, 2] and wa[0, 2] == 0 and wa[0, 3] == I[0, 0]


def group_case(device, sizes, counts_a, counts_b, seed):
    per = []
    for g, ((H, W), na, nb) in enumerate(zip(sizes, counts_a, counts_b)):
        sa, ta, ma, ca = build_set(every_kind(na, H, W, seed + g), H, W, device)
        sb, tb, mb, cb = build_set(every_kind(nb, H, W, seed + 100 + g), H, W, device)
        per.append(((sa, ta), (sb, tb), (ma, ca, mb, cb)))
    A = join([p[0] for p in per], device)
    B = join([p[1] for p in per], device)
    return per, A, B


@pytest.mark.parametrize("name", ["four", "sixty-four"])
def test_groups_equal_per_image_calls(cuda, name):
    if name == "four":
        sizes, counts_a, counts_b = [(70, 37), (64, 64), (3, 50), (129, 5)], [19, 0, 3, 40], [23, 33, 0, 70]
    else:
        sizes, counts_a, counts_b = [(8, 8)] * 64, [(g * 5) % 4 for g in range(64)], [(g * 3) % 5 for g in range(64)]
    per, (sa, ta), (sb, tb) = group_case(cuda, sizes, counts_a, counts_b, 7)
    crowd = torch.from_numpy((np.arange(sum(counts_b)) % 4 == 2).astype(np.uint8)).to(cuda)
    inter, a, b = ops.rle_match(sa, ta, sb, tb, sizes, counts_a, counts_b, crowd_b=crowd)
    inter2, a2, b2 = ops.rle_match(sa, ta, sb, tb, sizes, counts_a, counts_b, crowd_b=crowd)
    none, a3, b3 = ops.rle_match(sa, ta, sb, tb, sizes, counts_a, counts_b, crowd_b=crowd, matrix=False)
    assert none is None and len(inter) == len(sizes)
    for x, y in ((a, a2), (b, b2), (a, a3), (b, b3)):      # two calls give the same bytes; no matrix, the same matches
        assert torch.equal(x, y)
    ea = eb = 0
    for g, (((psa, pta), (psb, ptb), (ma, ca, mb, cb)), na, nb) in enumerate(zip(per, counts_a, counts_b)):
        assert tuple(inter[g].shape) == (na, nb) and torch.equal(inter[g], inter2[g])
        cg = crowd[eb:eb + nb]
        I, wa, wb = expect(ma, ca, mb, cb, cg.cpu().numpy())
        assert np.array_equal(inter[g].cpu().numpy(), I), g
        assert np.array_equal(a[ea:ea + na].cpu().numpy(), wa) and np.array_equal(b[eb:eb + nb].cpu().numpy(), wb), g
        H, W = sizes[g]
        one, oa, ob = ops.rle_match(psa, pta, psb, ptb, [(H, W)], [na], [nb], crowd_b=cg.contiguous())
        assert torch.equal(one[0], inter[g]) and torch.equal(oa, a[ea:ea + na]) and torch.equal(ob, b[eb:eb + nb]), g
        ea += na
        eb += nb
    assert any(n == 0 for n in counts_a) and any(n == 0 for n in counts_b)


def raw_call(lib, sa, ta, sb, tb, images, inter, elems, ma, mb, ws_bytes=None, want=True):
    images = np.ascontiguousarray(images, dtype=np.int64)
    Sa, Sb = int(sa.shape[0]), int(sb.shape[0])
    need = lib.hgl_rle_match_workspace_bytes(images.ctypes.data, len(images), Sa, int(sa.shape[1]), Sb, int(sb.shape[1]), int(want))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=sa.device)
    rc = lib.hgl_rle_match_device(sa.data_ptr(), int(sa.shape[1]), ta.data_ptr(), Sa, sb.data_ptr(), int(sb.shape[1]), tb.data_ptr(), Sb,
                                  images.ctypes.data, len(images), None, inter.data_ptr() if want else None, elems, ma.data_ptr(),
                                  mb.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    return rc, need


def test_contract_workspace_refusals_and_containment(cuda):
    lib = _lib.load()
    sizes, counts_a, counts_b = [(70, 37), (3, 50), (64, 64)], [33, 3, 5], [65, 0, 9]
    per, (sa, ta), (sb, tb) = group_case(cuda, sizes, counts_a, counts_b, 31)
    Sa, Sb = sum(counts_a), sum(counts_b)
    # the matrices out of order, with gaps between them and guard words at both ends
    offs = [9 + 5 * 9 + 4, 9 + 5 * 9 + 2, 9]
    elems = offs[0] + 33 * 65 + 11
    images = [[H, W, e_a, e_b, o] for (H, W), e_a, e_b, o in zip(sizes, [0, 33, 36], [0, 65, 65], offs)]
    inter = torch.full((elems,), POISON, dtype=torch.int32, device=cuda)
    ma = torch.full((Sa + 2, 4), POISON, dtype=torch.int32, device=cuda)
    mb = torch.full((Sb + 2, 4), POISON, dtype=torch.int32, device=cuda)
    rc, need = raw_call(lib, sa, ta, sb, tb, images, inter, elems, ma[1:], mb[1:])
    assert rc == 0, lib.hgl_last_error()
    torch.cuda.synchronize()
    got = inter.cpu().numpy()
    written = np.zeros(elems, bool)
    for g, o in enumerate(offs):
        n = counts_a[g] * counts_b[g]
        written[o:o + n] = True
        ma_g, ca, mb_g, cb = per[g][2]
        assert np.array_equal(got[o:o + n].reshape(counts_a[g], counts_b[g]), expect(ma_g, ca, mb_g, cb)[0]), g
    assert (got[~written] == POISON).all() and (~written).sum() == elems - 33 * 65 - 5 * 9
    assert (ma[0] == POISON).all() and (ma[-1] == POISON).all() and (mb[0] == POISON).all() and (mb[-1] == POISON).all()
    assert (ma[1:-1, 0] != POISON).all() and (mb[1:-1, 0] != POISON).all()
    # a short workspace; refused geometries: nothing is enqueued, the buffers keep their bytes
    inter.fill_(POISON)
    ma.fill_(POISON)
    assert raw_call(lib, sa, ta, sb, tb, images, inter, elems, ma[1:], mb[1:], ws_bytes=need - 1)[0] == -3
    assert b"workspace" in lib.hgl_last_error()
    bad = [list(r) for r in images]
    bad[2][4] = offs[0] - 5 * 9 + 1      # image 2's last element is image 0's first (image 1's matrix is empty: it overlaps nothing)
    for rows, n_elems, msg in ((bad, elems, b"overlap"), (images, offs[0] + 33 * 65 - 1, b"outside"),
                               ([[70, 37, 0, 0, 0], [3, 50, 34, 65, 0], [64, 64, 33, 65, 0]], elems, b"A entries"),
                               ([[0, 37, 0, 0, 0]] + images[1:], elems, b"bad size")):
        assert raw_call(lib, sa, ta, sb, tb, rows, inter, n_elems, ma[1:], mb[1:])[0] == -1
        assert msg in lib.hgl_last_error(), lib.hgl_last_error()
    assert raw_call(lib, sa, ta, sb, tb, [[8, 8, 0, 0, 0]] * 65, inter, elems, ma[1:], mb[1:])[0] == -1
    torch.cuda.synchronize()
    assert (inter == POISON).all() and (ma == POISON).all()
    # ops.rle_match validates in the style of rle_decode_group
    with pytest.raises(ValueError, match="counts sum"):
        ops.rle_match(sa, ta, sb, tb, sizes, [33, 3, 4], counts_b)
    with pytest.raises(ValueError, match="crowd_b"):
        ops.rle_match(sa, ta, sb, tb, sizes, counts_a, counts_b, crowd_b=torch.zeros(3, dtype=torch.uint8, device=cuda))
    with pytest.raises(_lib.HybridGLError):
        ops.rle_match(sa.cpu(), ta, sb, tb, sizes, counts_a, counts_b)
