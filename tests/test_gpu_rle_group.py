"""hgl_rle_decode_group_device (csrc/rle.hip) through ops.rle_decode_group: one call for a group of images of several sizes
against a host oracle built from the slots and the table (masks, status, boxes: exact) and against ops.rle_decode +
sam.mask_boxes per image (a group of one equals a group of many; mask_boxes is a kernel of its own) -- on the sizes at which
the row tiling, the store paths and the image lookup change, on every kind of entry the decoder knows, and the contract of
the entry (containment with guard bytes, determinism, refused geometry, a launch count that does not depend on the group)."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops
from hybridgl_amd import sam as hsam
from oracle import gen_gtmask_golden as GG
from oracle import gtmask_oracle as G

import abi_ref

pytestmark = pytest.mark.gpu

SENT = 0x5A


def special_masks(H, W):
    """empty, full, one pixel in each corner, a run that crosses a column boundary (box: the full height)"""
    out = np.zeros((7, H, W), np.uint8)
    out[1] = 1
    out[2, 0, 0] = out[3, 0, W - 1] = out[4, H - 1, 0] = out[5, H - 1, W - 1] = 1
    x = max(W // 2 - 1, 0)
    out[6, H - 1, x] = 1
    out[6, 0, min(x + 1, W - 1)] = 1
    return out


def blobs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, ry, rx = rng.random() * H, rng.random() * W, (0.05 + 0.3 * rng.random()) * H, (0.05 + 0.3 * rng.random()) * W
            out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
    return out


def counts_of(masks):
    return [hsam.mask_to_rle(m)["counts"] for m in masks]


def image_counts(H, W):
    """the run lists of one image: the special masks, blobs, zero-length runs, and counts that miss H*W (code 1)"""
    HW = H * W
    lists = counts_of(special_masks(H, W)) + counts_of(blobs(3, H, W, seed=H * 1000 + W))
    lists += [[0, 0, 0, 1, 0, 0, 0, HW - 1, 0], [HW, 0, 0], [], [0xFFFFFFFF, 5], [1, HW + 7], [0, 1]]
    if HW > 9:
        lists += [[3, 0, 0, 2, 0, 4, HW - 9], [5, HW - 6], [2, 0xFFFFFFFF, 0xFFFFFFFF, 7]]
    return lists


def join(sets):
    """per-image (slots, table) device sets of their own slot sizes -> one set of the widest slot (words beyond n are zeros)"""
    sw = max(int(s.shape[1]) for s, _ in sets)
    slots = torch.zeros((sum(int(s.shape[0]) for s, _ in sets), sw), dtype=torch.int32, device=sets[0][0].device)
    e = 0
    for s, _ in sets:
        slots[e:e + int(s.shape[0]), :int(s.shape[1])] = s
        e += int(s.shape[0])
    return slots, torch.cat([t for _, t in sets]).contiguous()


def reference(slots, table, sizes, counts):
    """the per-image path: ops.rle_decode + sam.mask_boxes for every image that owns entries"""
    masks, boxes, status, e = [], [], [], 0
    for (H, W), n in zip(sizes, counts):
        if n == 0:
            masks.append(torch.empty((0, H, W), dtype=torch.uint8, device=slots.device))
            continue
        m, st = ops.rle_decode(slots[e:e + n].contiguous(), table[e:e + n].contiguous(), H, W)
        masks.append(m)
        boxes.append(hsam.mask_boxes(m))
        status.append(st)
        e += n
    return masks, torch.cat(boxes), torch.cat(status)


def host_oracle(slots, table, sizes, counts):
    """the decoder's contract on the host, from the slots and the table as the device holds them -> per image masks [n,H,W]
    uint8, and for all entries status rows (code, area, 0, 0) and inclusive XYXY boxes (zeros for an empty mask)"""
    words = slots.cpu().numpy().view(np.uint32)
    tab = table.cpu().numpy()
    sw = words.shape[1]
    masks, status, boxes, e = [], [], [], 0
    for (H, W), n in zip(sizes, counts):
        out = np.zeros((n, H, W), np.uint8)
        for i in range(n):
            cnt, form = int(tab[e + i, 0]), int(tab[e + i, 1])
            plane_words = (H * W + 31) // 32
            code = 2
            if form == 0 and 0 <= cnt <= sw:
                c = [int(v) for v in words[e + i, :cnt]]
                out[i] = G.counts_to_mask(c, H, W)
                code = 0 if sum(c) == H * W else 1
            elif form == 1 and cnt >= 0 and plane_words <= sw:      # n_counts < 0 is no mask in either form (include/hybridgl.h)
                bits = np.unpackbits(words[e + i, :plane_words].astype("<u4").view(np.uint8), bitorder="little")
                out[i] = bits[:H * W].reshape(W, H).T
                code = 0
            ys, xs = np.nonzero(out[i])
            boxes.append([xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0, 0, 0, 0])
            status.append([code, int(out[i].sum()), 0, 0])
        masks.append(out)
        e += n
    return masks, np.array(status, np.int32).reshape(-1, 4), np.array(boxes, np.int32).reshape(-1, 4)


def check_group(slots, table, sizes, counts):
    got_m, got_b, got_s = ops.rle_decode_group(slots, table, sizes, counts)
    want_m, want_s, want_b = host_oracle(slots, table, sizes, counts)
    assert len(got_m) == len(sizes)
    for g, (a, b) in enumerate(zip(got_m, want_m)):
        assert np.array_equal(a.cpu().numpy(), b), (g, sizes[g])
    assert np.array_equal(got_s.cpu().numpy(), want_s), (got_s.cpu().numpy() != want_s).any(1).nonzero()[0].tolist()
    assert np.array_equal(got_b.cpu().numpy(), want_b), (got_b.cpu().numpy() != want_b).any(1).nonzero()[0].tolist()
    ref_m, ref_b, ref_s = reference(slots, table, sizes, counts)
    for g, (a, b) in enumerate(zip(got_m, ref_m)):
        assert tuple(a.shape) == (counts[g],) + tuple(sizes[g]) and a.dtype == torch.uint8
        assert torch.equal(a, b), (g, sizes[g])
    assert got_b.dtype == torch.int32 and torch.equal(got_b, ref_b.to(torch.int32)), \
        (got_b - ref_b.to(torch.int32)).abs().amax(1).nonzero().reshape(-1).tolist()
    assert torch.equal(got_s, ref_s)
    return got_m, got_b, got_s


# 1x1; 64x64; 65x63: W % 4 != 0 and a second word of rows; 63x260: the second column tile of the wide path; 130x4; 3x5 in front
# of 64x64 makes the latter's base odd (byte path at W % 4 == 0); 260x70: a second block of row tiles on the byte path
SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (64, 64), (260, 70)]


def test_group_of_many_sizes_from_packed_counts(cuda):
    """every size at once, an image without entries in the middle and one at the end"""
    sizes, counts, sets = [], [], []
    for i, (H, W) in enumerate(SIZES):
        lists = image_counts(H, W)
        if (H, W) == (3, 5):      # as many entries (9, 8 or 7 of 15 bytes) as leave the next image's first byte off a 4-byte boundary
            before = sum(n * h * w for (h, w), n in zip(sizes, counts))
            lists = lists[:next(k for k in (9, 8, 7) if (before + 15 * k) % 4)]
        sets.append(ops.rle_pack(lists, H, W, device=cuda))
        sizes.append((H, W))
        counts.append(len(lists))
        if i == 2:
            sizes.append((17, 12))
            counts.append(0)
    sizes.append((40, 40))
    counts.append(0)
    slots, table = join(sets)
    images, _ = ops.rle_group_layout(sizes, counts)
    assert images[sizes.index((3, 5)) + 1, 3] % 4 != 0
    masks, boxes, status = check_group(slots, table, sizes, counts)
    st = status.cpu().numpy()
    assert set(st[:, 0].tolist()) == {0, 1} and (st[:, 2:] == 0).all()
    # the run that crosses a column boundary spans the full height; an empty mask has the zero box
    b = boxes.cpu().numpy()
    e = int(images[1, 2])
    assert b[e + 6].tolist() == [31, 0, 32, 63] and b[e].tolist() == [0, 0, 0, 0] and b[e + 1].tolist() == [0, 0, 63, 63]


def test_both_forms_straight_from_the_encoder_and_entries_without_a_mask(cuda):
    """checkerboards and noise arrive from ops.rle_encode as bit planes (form 1), blobs as counts; forms 2 and 3 and
    n_counts > slot_words are code 2: zeros, the zero box"""
    sizes, counts, sets, want = [], [], [], []
    for H, W in ((65, 63), (64, 64), (3, 5), (63, 260), (20, 33)):
        yy, xx = np.mgrid[0:H, 0:W]
        batch = np.concatenate([special_masks(H, W), blobs(2, H, W, seed=W), ((yy + xx) & 1).astype(np.uint8)[None],
                                ((yy + xx + 1) & 1).astype(np.uint8)[None],
                                (np.random.default_rng(H).random((1, H, W)) < 0.5).astype(np.uint8)])
        sets.append(ops.rle_encode(torch.from_numpy(batch).to(cuda)))
        sizes.append((H, W))
        counts.append(len(batch))
        want.append(batch)
    slots, table = join(sets)
    forms = table.cpu().numpy()[:, 1]
    assert set(forms.tolist()) == {0, 1}
    masks, boxes, status = check_group(slots, table, sizes, counts)
    for g, batch in enumerate(want):
        assert np.array_equal(masks[g].cpu().numpy(), batch), sizes[g]
    assert np.array_equal(status.cpu().numpy()[:, 1], np.concatenate([b.reshape(len(b), -1).sum(1) for b in want]))
    table = table.clone()
    sw = int(slots.shape[1])
    bad = [1, 8, counts[0] + 2, counts[0] + 9, sum(counts) - 1]
    table[bad[0], 1] = 2
    table[bad[1], 1] = 3
    table[bad[2], 0] = sw + 1
    table[bad[2], 1] = 0
    table[bad[3], 0] = -1
    table[bad[4], 1] = 7
    masks, boxes, status = check_group(slots, table, sizes, counts)
    st, b = status.cpu().numpy(), boxes.cpu().numpy()
    for s in bad:
        assert st[s].tolist() == [2, 0, 0, 0] and b[s].tolist() == [0, 0, 0, 0], s
    flat = torch.cat([m.reshape(m.shape[0], -1).any(1) for m in masks]).cpu().numpy()
    assert not flat[bad].any() and flat.sum() > len(flat) // 2


def test_fuzz(cuda):
    """the 120 masks of the host codec's fuzz (sizes 1 .. 299), each an image of its own, 60 images to a call"""
    fuzz = list(GG.fuzz_rle_masks())
    for lo in range(0, len(fuzz), 60):
        part = fuzz[lo:lo + 60]
        sizes = [m.shape for m in part]
        sets = [ops.rle_pack(counts_of([m]), m.shape[0], m.shape[1], device=cuda) for m in part]
        slots, table = join(sets)
        masks, boxes, status = check_group(slots, table, sizes, [1] * len(part))
        for g, m in enumerate(part):
            assert np.array_equal(masks[g][0].cpu().numpy(), m), (lo + g, m.shape)
        assert status.cpu().numpy()[:, :2].tolist() == [[0, int(m.sum())] for m in part]


def _raw(lib, slots, table, images, G, out, boxes, status, ws, S=None, ws_bytes=None, masks_bytes=None):
    images = np.ascontiguousarray(images, dtype=np.int64)
    return lib.hgl_rle_decode_group_device(slots.data_ptr(), int(slots.shape[1]), table.data_ptr(),
                                           int(slots.shape[0]) if S is None else S, images.ctypes.data, G, out.data_ptr(),
                                           out.numel() if masks_bytes is None else masks_bytes, boxes.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                           torch.cuda.current_stream().cuda_stream)


def _small_group(cuda):
    sizes = [(65, 63), (3, 5), (64, 64), (130, 4)]
    lists = [image_counts(H, W)[:8] for H, W in sizes]
    slots, table = join([ops.rle_pack(c, H, W, device=cuda) for c, (H, W) in zip(lists, sizes)])
    return sizes, [8] * 4, slots, table


def test_guard_bytes_and_two_calls(cuda):
    """extents laid out with gaps of 1, 2 and 7 bytes between them and spare bytes behind: every extent byte is 0 / 1, every
    other byte keeps the sentinel; the bytes equal the packed call's; a second call writes the same"""
    lib = _lib.load()
    sizes, counts, slots, table = _small_group(cuda)
    images, _ = ops.rle_group_layout(sizes, counts)
    gaps = [5, 1, 2, 7]
    o, ext = 0, []
    for g, ((H, W), n) in enumerate(zip(sizes, counts)):
        o += gaps[g]
        images[g, 3] = o
        ext.append((o, o + n * H * W))
        o += n * H * W
    total = o + 4096
    S = int(slots.shape[0])
    ws = ops.workspace(lib.hgl_rle_decode_group_workspace_bytes(S, int(slots.shape[1])), cuda, "rle")
    ref_m, ref_b, ref_s = ops.rle_decode_group(slots, table, sizes, counts)
    runs = []
    for _ in range(2):
        buf = torch.full((total,), SENT, dtype=torch.uint8, device=cuda)
        boxes = torch.full((S, 4), -9, dtype=torch.int32, device=cuda)
        status = torch.full((S, 4), -9, dtype=torch.int32, device=cuda)
        assert _raw(lib, slots, table, images, len(sizes), buf, boxes, status, ws) == 0, lib.hgl_last_error()
        host = buf.cpu().numpy()
        inside = np.zeros(total, bool)
        for g, (a, b) in enumerate(ext):
            inside[a:b] = True
            assert torch.equal(buf[a:b].view(ref_m[g].shape), ref_m[g]), g
        assert host[inside].max() <= 1, "a byte inside is neither 0 nor 1"
        assert (host[~inside] == SENT).all(), "wrote outside the extents"
        assert torch.equal(boxes, ref_b) and torch.equal(status, ref_s)
        runs.append((host.tobytes(), boxes.cpu().numpy().tobytes(), status.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_bad_geometry_is_refused_and_nothing_is_enqueued(cuda):
    lib = _lib.load()
    sizes, counts, slots, table = _small_group(cuda)
    good, total = ops.rle_group_layout(sizes, counts)
    S, G = int(slots.shape[0]), len(sizes)
    ws = ops.workspace(lib.hgl_rle_decode_group_workspace_bytes(S, int(slots.shape[1])), cuda, "rle")
    buf = torch.full((total + 64,), SENT, dtype=torch.uint8, device=cuda)
    boxes = torch.full((S, 4), -9, dtype=torch.int32, device=cuda)
    status = torch.full((S, 4), -9, dtype=torch.int32, device=cuda)

    def bad(images, G=G, code=-1, **kw):
        assert _raw(lib, slots, table, images, G, buf, boxes, status, ws, **kw) == code, lib.hgl_last_error()

    overlap = good.copy()
    overlap[2, 3] -= 1
    bad(overlap)
    assert b"overlap" in lib.hgl_last_error()
    swapped = good.copy()      # overlap-free, inside, but image 1 lies in front of image 0
    swapped[1, 3], swapped[0, 3] = 0, counts[1] * 15
    beyond = good.copy()
    beyond[3, 3] += 65
    bad(beyond)
    bad(good, masks_bytes=total - 1)
    decreasing = good.copy()
    decreasing[2, 2] = decreasing[1, 2] - 1
    bad(decreasing)
    late = good.copy()
    late[0, 2] = 1
    bad(late)
    past = good.copy()
    past[3, 2] = S + 1
    bad(past)
    negative = good.copy()
    negative[1, 3] = -4
    bad(negative)
    zero = good.copy()
    zero[1, 0] = 0
    bad(zero)
    huge = good.copy()
    huge[3, 0], huge[3, 1] = 1 << 16, 1 << 15
    bad(huge)
    many = np.zeros((65, 4), np.int64)
    many[:, :2] = 4
    many[1:, 2] = S
    bad(many, G=65)
    assert b"65 images" in lib.hgl_last_error()
    bad(good, G=0)
    bad(good, code=-3, ws_bytes=8)
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (boxes == -9).all() and (status == -9).all(), "a refused call wrote"
    # the geometry that was only rearranged is accepted
    assert _raw(lib, slots, table, swapped, G, buf, boxes, status, ws) == 0, lib.hgl_last_error()
    ref_m, ref_b, ref_s = ops.rle_decode_group(slots, table, sizes, counts)
    assert torch.equal(buf[:counts[1] * 15].view(ref_m[1].shape), ref_m[1]) and torch.equal(boxes, ref_b)


def test_the_launches_do_not_depend_on_the_group(cuda):
    """six images of six sizes, and a group whose images take different store paths, launch the two kernels of a group of one
    (which instantiation of the rows kernel: test_every_rows_kernel_writes_the_same_bytes)"""
    sizes = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5)]
    sets = [ops.rle_pack(image_counts(H, W)[:10], H, W, device=cuda) for H, W in sizes]
    slots, table = join(sets)
    one = abi_ref.rle_kernels(lambda: ops.rle_decode_group(*sets[1], sizes[1:2], [10]))
    six = abi_ref.rle_kernels(lambda: ops.rle_decode_group(slots, table, sizes, [10] * 6))
    # 3 x 5 with 8 entries is narrow, 64 x 64 behind it at byte 120 is wide
    m_slots, m_table = join([ops.rle_pack(image_counts(3, 5)[:8], 3, 5, device=cuda), sets[1]])
    mixed = abi_ref.rle_kernels(lambda: ops.rle_decode_group(m_slots, m_table, [(3, 5), (64, 64)], [8, 10]))
    assert len(one) == 2 and len(six) == 2 and len(mixed) == 2, (one, six, mixed)
    for got in (one, six, mixed):
        assert [k for k, _ in got] == ["rle_starts_kernel", "rle_rows_kernel"], got
    assert mixed[1][1] == "0", mixed


def test_every_rows_kernel_writes_the_same_bytes(cuda):
    """65 x 260 entries of every kind through rle_rows_kernel<4>, <1> and <0>: ops.rle_decode into an aligned and into an odd
    address, and as the second image of a group behind a 3 x 5 image whose 8 (7) entries leave it at byte 120 (105) -- the
    bytes, the status rows and (group calls) the boxes equal the host oracle"""
    H, W = 65, 260
    yy, xx = np.mgrid[0:H, 0:W]
    dense = np.stack([(yy + xx) & 1, np.random.default_rng(5).random((H, W)) < 0.5]).astype(np.uint8)
    planes = ops.rle_encode(torch.from_numpy(dense).to(cuda))
    assert planes[1].cpu().numpy()[:, 1].tolist() == [1, 1]
    slots, table = join([ops.rle_pack(image_counts(H, W), H, W, device=cuda), planes])
    S = int(slots.shape[0])
    n = S * H * W
    (want_m,), want_s, want_b = host_oracle(slots, table, [(H, W)], [S])
    assert np.array_equal(want_m[-2:], dense) and set(want_s[:, 0].tolist()) == {0, 1}

    def single(offset, V):
        buf = torch.full((offset + n + 64,), SENT, dtype=torch.uint8, device=cuda)
        assert buf.data_ptr() % 4 == 0
        res = []
        names = abi_ref.rle_kernels(lambda: res.append(ops.rle_decode(slots, table, H, W, out=buf[offset:offset + n])))
        assert names == [("rle_starts_kernel", names[0][1]), ("rle_rows_kernel", V)], names
        host = buf.cpu().numpy()
        assert (host[:offset] == SENT).all() and (host[offset + n:] == SENT).all(), "wrote outside the output"
        return host[offset:offset + n].reshape(S, H, W), res[0][1].cpu().numpy(), None

    def behind(k, V):
        first = ops.rle_pack(image_counts(3, 5)[:k], 3, 5, device=cuda)
        g_slots, g_table = join([first, (slots, table)])
        images, _ = ops.rle_group_layout([(3, 5), (H, W)], [k, S])
        assert images[1, 3] == 15 * k
        res = []
        names = abi_ref.rle_kernels(lambda: res.append(ops.rle_decode_group(g_slots, g_table, [(3, 5), (H, W)], [k, S])))
        assert names == [("rle_starts_kernel", names[0][1]), ("rle_rows_kernel", V)], names
        masks, boxes, status = res[0]
        assert masks[0].data_ptr() % 4 == 0
        return masks[1].cpu().numpy(), status[k:].cpu().numpy(), boxes[k:].cpu().numpy()

    for name, (m, st, b) in (("aligned: <4>", single(0, "4")), ("odd address: <1>", single(1, "1")),
                             ("behind 120 bytes: <0>, wide branch", behind(8, "0")), ("behind 105 bytes: <1>", behind(7, "1"))):
        assert m.max() <= 1 and np.array_equal(m, want_m), name
        assert np.array_equal(st, want_s), name
        assert b is None or np.array_equal(b, want_b), name


def test_front_end_checks(cuda):
    slots, table = ops.rle_pack([[16], [0, 16]], 4, 4, device=cuda)
    with pytest.raises(ValueError, match="counts sum"):
        ops.rle_decode_group(slots, table, [(4, 4)], [3])
    with pytest.raises(ValueError, match="uint8 elements"):
        ops.rle_decode_group(slots, table, [(4, 4)], [2], out=torch.empty(33, dtype=torch.uint8, device=cuda))
    with pytest.raises(_lib.HybridGLError):
        ops.rle_decode_group(slots, table, [(4, 4)] * 65, [2] + [0] * 64)
    masks, boxes, status = ops.rle_decode_group(slots[:0], table[:0], [(4, 4), (2, 3)], [0, 0])
    assert [tuple(m.shape) for m in masks] == [(0, 4, 4), (0, 2, 3)] and tuple(boxes.shape) == (0, 4)
    out = torch.empty(32, dtype=torch.uint8, device=cuda)
    masks, boxes, status = ops.rle_decode_group(slots, table, [(4, 4)], [2], out=out)
    assert masks[0].data_ptr() == out.data_ptr() and boxes.cpu().tolist() == [[0, 0, 0, 0], [0, 0, 3, 3]]
    assert status.cpu().tolist() == [[0, 0, 0, 0], [0, 16, 0, 0]]
