"""hgl_rle_paint_device (csrc/rle_paint.hip) on the GPU.  Everything is integers and bytes, so every comparison is equality:
`out`, `labels` and `status` of the call, into sentinel-filled buffers, against the numpy statement of the contract
(tests/paint_cases.py) applied to buffers filled the same way.  Sizes: 1 x 1, one row, one column, either side of the 64-row
word and of the 64-column tile, 31 x 33, groups that cross both at once, one group of 64 mixed images (some without entries,
some without list positions, odd pixel offsets), 480 x 640 once.  Also: forms 0 and 1 of the same masks; slot_words either
side of the form-0 / form-1 boundary; base=None; labels on and off; K = 0; S = 0; a paint list that is a device tensor straight
from ops.rle_nms; rle_encode -> rle_paint against rle_decode's pixels; refused geometries through the raw ABI leave the
sentinels intact.  Every call is made twice and compared bit for bit."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops

import paint_cases as PC

pytestmark = pytest.mark.gpu

FENCE = 0xA5
CASES = PC.cases()


def dev_set(case, cuda):
    slots = torch.from_numpy(case["slots"].view(np.int32).copy()).to(cuda)
    table = torch.from_numpy(case["table"].copy()).to(cuda)
    return slots, table


def run(case, cuda, with_base=True, with_labels=True, device_list=False):
    """ops.rle_paint twice into fenced `out` buffers -> (out [P,3], labels [P] or None, status [K,4]) as numpy"""
    images, total, base, *_ = PC.expect(case, with_base, with_labels)
    slots, table = dev_set(case, cuda)
    order, style = case["order"], case["style"]
    if device_list:
        order = torch.from_numpy(order.copy()).to(cuda)
        style = torch.from_numpy(style.view(np.int32).copy()).to(cuda)
    b = torch.from_numpy(base.reshape(-1).copy()).to(cuda) if with_base else None
    got = []
    for _ in range(2):
        out = torch.full((3 * total,), FENCE, dtype=torch.uint8, device=cuda)
        pics, labs, status = ops.rle_paint(slots, table, case["sizes"], case["counts"], order, case["order_counts"], style, base=b,
                                           out=out, labels=with_labels)
        assert pics[0].data_ptr() == out.data_ptr() and [tuple(p.shape) for p in pics] == [(h, w, 3) for h, w in case["sizes"]]
        lab = torch.cat([l.reshape(-1) for l in labs]).cpu().numpy() if with_labels else None
        got.append((out.cpu().numpy().reshape(-1, 3), lab, status.cpu().numpy()))
    assert all(a is None or np.array_equal(a, b) for a, b in zip(got[0], got[1])), "two calls differ"
    return got[0]


def check(case, cuda, **kw):
    with_base, with_labels = kw.get("with_base", True), kw.get("with_labels", True)
    _, _, _, out, labels, status, _ = PC.expect(case, with_base, with_labels)
    g_out, g_lab, g_status = run(case, cuda, **kw)
    assert np.array_equal(g_status, status), (case["seed"], g_status.tolist(), status.tolist())
    assert np.array_equal(g_out, out), (case["seed"], np.argwhere(g_out != out)[:5].tolist())
    if with_labels:
        assert np.array_equal(g_lab, labels), case["seed"]
    return g_out


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: "x".join(f"{h}x{w}" for h, w in CASES[k]["sizes"]) + f"-{CASES[k]['seed']}")
def test_the_cases_bit_equal(cuda, k):
    check(CASES[k], cuda, with_base=True, with_labels=True, device_list=bool(k % 2))


def test_black_canvases_and_labels_off(cuda):
    for c in (CASES[0], CASES[7], CASES[19], CASES[-1], CASES[-2]):
        check(c, cuda, with_base=False, with_labels=False)
        check(c, cuda, with_base=False, with_labels=True)
        check(c, cuda, with_base=True, with_labels=False)


def test_forms_0_and_1_of_the_same_masks_give_the_same_bytes(cuda):
    for seed, sizes in ((6, [(65, 3)]), (8, [(3, 65)]), (10, [(70, 67), (31, 33)])):
        a, b = PC.make_case(seed, sizes, form=0), PC.make_case(seed, sizes, form=1)
        assert all(np.array_equal(x, y) for x, y in zip(a["masks"], b["masks"])) and not np.array_equal(a["table"], b["table"])
        assert np.array_equal(check(a, cuda), check(b, cuda))


def test_slot_words_either_side_of_the_form_boundary(cuda):
    """an entry whose plane is exactly slot_words long is read, one word more than the slot holds is code 2; likewise the counts"""
    H, W = 9, 15                                     # 135 pixels: 5 plane words
    rng = np.random.default_rng(11)
    M = rng.random((H, W)) < 0.5
    n = len(PC.counts_of(M))
    for sw, forms in ((5, [1]), (4, [1]), (n, [0]), (n - 1, [0])):
        slots = np.zeros((1, max(n, 5)), np.uint32)
        table = np.zeros((1, 4), np.int32)
        if forms[0] == 1:
            slots[0, :5] = PC.plane_of(M)
            table[0] = (n, 1, int(M.sum()), 0)
        else:
            slots[0, :n] = PC.counts_of(M)
            table[0] = (n, 0, int(M.sum()), 0)
        case = dict(seed=sw, sizes=[(H, W)], counts=[1], order=np.zeros(1, np.int32), order_counts=[1],
                    style=PC.style_row((9, 8, 7), 0.25, 0.75, (1, 2, 3))[None], slots=np.ascontiguousarray(slots[:, :sw]), table=table, sw=sw,
                    base_seed=3)
        want_code = 0 if sw in (5, n) else 2
        assert PC.expect(case)[5][0, 0] == want_code
        check(case, cuda)


def test_k_0_and_s_0(cuda):
    c = CASES[-1]
    G = len(c["sizes"])
    none = dict(c, order=np.zeros(0, np.int32), order_counts=[0] * G, style=np.zeros((0, 4), np.uint32))
    out = check(none, cuda)                                              # K = 0 with G > 0 still copies the bases
    assert np.array_equal(out, PC.base_of(c, len(out)))
    check(none, cuda, with_base=False)
    empty = dict(c, counts=[0] * G, slots=c["slots"][:0], table=c["table"][:0])      # S = 0: every position is code 3
    _, _, _, _, _, status, _ = PC.expect(empty)
    assert (status[:, 0] == 3).all()
    check(empty, cuda)


def test_a_group_of_64_mixed_images(cuda):
    sizes = [EDGE for EDGE in PC.EDGE_SIZES] * 6 + [(66, 70), (13, 7), (1, 1), (5, 63)]
    assert len(sizes) == 64
    case = PC.make_case(77, sizes, form=2)
    images, total = PC.layout(case["sizes"], case["counts"], case["order_counts"])
    assert 0 in case["counts"] and 0 in case["order_counts"] and any(r[4] % 2 for r in images) and any(r[4] % 4 == 1 for r in images)
    check(case, cuda)
    check(case, cuda, with_base=False, with_labels=False, device_list=True)


def test_480x640_once(cuda):
    check(PC.make_case(5, [(480, 640)], form=2), cuda)


def test_a_paint_list_straight_from_rle_nms(cuda):
    """the kept indices of the mask NMS are the list: a device tensor, never read back; the tail beyond out_n is -1 = code 3"""
    rng = np.random.default_rng(4)
    sizes, counts = [(40, 70), (65, 20)], [6, 5]
    masks = []
    for (H, W), n in zip(sizes, counts):
        base = [PC.blob(rng, H, W, "box") for _ in range(n // 2)]
        masks += (base * 3)[:n]      # duplicates: the NMS drops them
    need = max(len(PC.counts_of(M)) for M in masks)
    slots, table = PC.encode_set(masks, need, [0] * len(masks))
    d_slots, d_table = torch.from_numpy(slots.view(np.int32).copy()).to(cuda), torch.from_numpy(table.copy()).to(cuda)
    out_idx, out_n, result = ops.rle_nms(d_slots, d_table, sizes, counts, thr=0.5)
    style = np.stack([PC.style_row(PC.PALETTE[i % 8], 0.5, 0.5, PC.PALETTE[(i + 1) % 8]) for i in range(sum(counts))])
    # on the device, with no count read back: what lies behind an image's out_n kept indices names no entry
    image_of = torch.from_numpy(np.repeat(np.arange(len(counts)), counts)).to(cuda)
    local = torch.arange(sum(counts), device=cuda) - torch.from_numpy(np.repeat(np.cumsum([0] + counts[:-1]), counts)).to(cuda)
    out_idx = torch.where(local < out_n.long()[image_of], out_idx, torch.full_like(out_idx, -1))
    pics, labs, status = ops.rle_paint(d_slots, d_table, sizes, counts, out_idx, counts, style, labels=True)
    order = out_idx.cpu().numpy()
    n = out_n.cpu().numpy()
    assert (n < np.array(counts)).all() and (n > 0).all()
    case = dict(seed=0, sizes=sizes, counts=counts, order=order, order_counts=counts, style=style, slots=slots, table=table, sw=need,
                base_seed=0)
    _, _, _, out, labels, want, _ = PC.expect(case, with_base=False)
    assert np.array_equal(status.cpu().numpy(), want) and (want[:, 0] == 3).sum() == sum(counts) - n.sum()
    assert np.array_equal(torch.cat([p.reshape(-1, 3) for p in pics]).cpu().numpy(), out)
    assert np.array_equal(torch.cat([l.reshape(-1) for l in labs]).cpu().numpy(), labels)


def test_encode_then_paint_equals_painting_the_decoded_pixels(cuda):
    rng = np.random.default_rng(9)
    H, W, N = 67, 130, 5
    masks = np.stack([PC.blob(rng, H, W, k) for k in ("disc", "noise", "box", "cross", "disc")])
    d_masks = torch.from_numpy(masks).to(cuda)
    for sw in (None, 200):      # the default slot: the noise entry is a bit plane (form 1); 200 words: it fits neither way (code 2)
        slots, table = ops.rle_encode(d_masks, slot_words=sw)
        decoded, dstatus = ops.rle_decode(slots, table, H, W)
        style = np.stack([PC.style_row(PC.PALETTE[i], 0.5, 0.5, PC.PALETTE[i + 1]) for i in range(N)])
        base = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
        pics, labs, status = ops.rle_paint(slots, table, [(H, W)], [N], list(range(N)), [N], style, base=[base], labels=True)
        # the numpy contract on rle_decode's pixels, entry by entry
        canvas = base.cpu().numpy().copy()
        lab = np.full((H, W), -1, np.int32)
        dec, codes = decoded.cpu().numpy().astype(bool), dstatus.cpu().numpy()[:, 0]
        for i in range(N):
            if codes[i] == 2:
                continue
            M, E = dec[i], PC.edge_of(dec[i])
            canvas[M] = PC.blend(canvas[M], PC.PALETTE[i], 0.5, 0.5)[0]
            canvas[E] = PC.PALETTE[i + 1]
            lab[M] = i
        assert np.array_equal(pics[0].cpu().numpy(), canvas) and np.array_equal(labs[0].cpu().numpy(), lab)
        assert np.array_equal(status.cpu().numpy()[:, :2], dstatus.cpu().numpy()[:, :2])
        assert (2 in codes) == (sw == 200)


def test_refused_geometries_through_the_raw_abi_enqueue_nothing(cuda):
    lib = _lib.load()
    c = CASES[-1]
    slots, table = dev_set(c, cuda)
    S, sw, K = len(c["table"]), c["sw"], len(c["order"])
    gaps = [5] * len(c["sizes"])
    images, total, base, out, labels, status, _ = PC.expect(c, gaps=gaps)
    total += 7      # room behind the last canvas
    order = torch.from_numpy(c["order"].copy()).to(cuda)
    style = torch.from_numpy(c["style"].view(np.int32).copy()).to(cuda)
    d_base = torch.from_numpy(np.concatenate([base, np.zeros((7, 3), np.uint8)]).reshape(-1)).to(cuda)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rows, S_=S, K_=K, sw_=sw, total_=total, base_=d_base, out_=None):
        d_out = torch.full((3 * total,), FENCE, dtype=torch.uint8, device=cuda)
        d_lab = torch.full((total,), -7, dtype=torch.int32, device=cuda)
        d_st = torch.full((K, 4), -7, dtype=torch.int32, device=cuda)
        arr = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
        rc = lib.hgl_rle_paint_device(slots.data_ptr(), sw_, table.data_ptr(), S_, order.data_ptr(), style.data_ptr(), K_,
                                      arr.ctypes.data, len(arr), None if base_ is None else base_.data_ptr(),
                                      d_out.data_ptr() if out_ is None else out_, total_, d_lab.data_ptr(), d_st.data_ptr(),
                                      ws.data_ptr(), ws.numel(), stream)
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy().reshape(-1, 3), d_lab.cpu().numpy(), d_st.cpu().numpy()

    # the accepted call with gaps: what lies between the canvases and behind the last keeps its sentinel
    rc, g_out, g_lab, g_st = call(images)
    assert rc == 0
    want_out = np.full((total, 3), FENCE, np.uint8)
    want_out[:len(out)] = out
    want_lab = np.full(total, -7, np.int32)
    inside = np.zeros(total, bool)
    for H, W, _, _, p in images:
        inside[p:p + H * W] = True
    want_lab[inside] = labels[inside[:len(labels)]]
    assert np.array_equal(g_out, want_out) and np.array_equal(g_lab, want_lab) and np.array_equal(g_st, status)
    assert need_ok(lib, images, S, sw, K, total)
    # refusals: nothing is enqueued, every sentinel is intact, the reason is named
    edit = lambda g, col, v: [[v if (i == g and j == col) else x for j, x in enumerate(r)] for i, r in enumerate(images)]
    bad = [("images", dict(rows=[])), ("bad size", dict(rows=edit(0, 0, 0))), ("entries", dict(rows=edit(0, 2, 1))),
           ("list entries", dict(rows=edit(0, 3, 1))), ("lie outside", dict(rows=images, total_=total - 8)),
           ("lie outside", dict(rows=edit(0, 4, -1))), ("slot_words", dict(rows=images, sw_=-1)), ("bad sizes", dict(rows=images, K_=-1)),
           ("out overlaps base", dict(rows=images, out_=d_base.data_ptr() + 3))]
    if len(images) > 1:
        bad.append(("overlap", dict(rows=edit(1, 4, images[0][4] + 1))))
    for why, kw in bad:
        rc, g_out, g_lab, g_st = call(**kw)
        assert rc == -1 and why in lib.hgl_last_error().decode(), (why, lib.hgl_last_error())
        assert (g_out == FENCE).all() and (g_lab == -7).all() and (g_st == -7).all(), why
    assert np.array_equal(d_base.cpu().numpy().reshape(-1, 3)[:len(base)], base)      # the overlapping call wrote nothing
    # a workspace one byte short is refused too, with its own code
    need = lib.hgl_rle_paint_workspace_bytes(np.asarray(images, dtype=np.int64).ctypes.data, len(images), S, sw, K, total)
    arr = np.asarray(images, dtype=np.int64)
    d_out = torch.full((3 * total,), FENCE, dtype=torch.uint8, device=cuda)
    d_st = torch.full((K, 4), -7, dtype=torch.int32, device=cuda)
    assert lib.hgl_rle_paint_device(slots.data_ptr(), sw, table.data_ptr(), S, order.data_ptr(), style.data_ptr(), K, arr.ctypes.data,
                                    len(arr), None, d_out.data_ptr(), total, None, d_st.data_ptr(), ws.data_ptr(), need - 1, stream) == -3
    torch.cuda.synchronize()
    assert (d_out == FENCE).all() and (d_st == -7).all()


def need_ok(lib, images, S, sw, K, total):
    need = lib.hgl_rle_paint_workspace_bytes(np.asarray(images, dtype=np.int64).ctypes.data, len(images), S, sw, K, total)
    return 0 < need <= 1 << 24


def test_ops_refuses_before_any_upload(cuda):
    c = CASES[0]
    slots, table = dev_set(c, cuda)
    args = (c["sizes"], c["counts"], c["order"], c["order_counts"], c["style"])
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, c["sizes"], [c["counts"][0] + 1], *args[2:])               # counts that do not sum to S
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, c["sizes"], c["counts"], c["order"], [len(c["order"]) + 1], c["style"])
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, [(0, 5)], *args[1:])
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, *args, out=torch.empty(5, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, *args[:4], c["style"][:1].repeat(3, 0))
    H, W = c["sizes"][0]
    buf = torch.zeros(3 * H * W + 3, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, *args, base=buf[:3 * H * W], out=buf[1:1 + 3 * H * W])      # two bytes shared
    with pytest.raises(ValueError):
        ops.rle_paint(slots, table, *args, base=[torch.zeros(H + 1, W, 3, dtype=torch.uint8, device=cuda)])
    one = ops.rle_paint(slots, table, *args[:4], c["style"][0])      # one row serves every position
    assert one[2].shape == (len(c["order"]), 4)
