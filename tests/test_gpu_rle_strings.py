"""COCO's compressed RLE strings written and read on the device (csrc/rle_string.hip: hgl_rle_to_strings_device,
hgl_rle_from_strings_device) through ops and through the raw ABI into sentinel-filled buffers, against the numpy statement of
the contract (tests/rle_string_cases.py, itself held against the host codec in tests/test_rle_string_cases_host.py) and against
the host codec.  Every comparison is exact; every call runs twice and is compared bit for bit."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops, sam

import abi_ref
import rle_string_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def write_sets():
    return RC.write_sets()


@pytest.fixture(scope="module")
def read_sets():
    return RC.read_sets()


def raw_to_strings(cuda, slots, table, cap, pad=16):
    """the raw entry into fenced buffers: (bytes [cap], offsets, status) plus the fences' state"""
    lib = _lib.load()
    S, sw = slots.shape
    d_slots = torch.from_numpy(slots.view(np.int32).copy()).to(cuda)
    d_table = torch.from_numpy(table.copy()).to(cuda)
    d_bytes = torch.full((pad + cap + pad,), RC.FENCE8, dtype=torch.uint8, device=cuda)
    d_off = torch.full((S + 3,), -77, dtype=torch.int64, device=cuda)
    d_status = torch.full((S + 2,), RC.FENCE32, dtype=torch.int32, device=cuda)
    first = None
    for rep in range(2):
        _lib.check(lib.hgl_rle_to_strings_device(d_slots.data_ptr(), sw, d_table.data_ptr(), S, d_bytes.data_ptr() + pad, cap,
                                                 d_off.data_ptr() + 8, d_status.data_ptr() + 4, torch.cuda.current_stream().cuda_stream),
                   "hgl_rle_to_strings_device")
        b, o, st = d_bytes.cpu().numpy(), d_off.cpu().numpy(), d_status.cpu().numpy()
        assert (b[:pad] == RC.FENCE8).all() and (b[pad + cap:] == RC.FENCE8).all(), "wrote outside the bytes"
        assert o[0] == -77 and o[-1] == -77 and st[0] == RC.FENCE32 and st[-1] == RC.FENCE32, "wrote outside offsets / status"
        got = (b[pad:pad + cap].copy(), o[1:-1].copy(), st[1:-1].copy())
        if rep == 0:
            first = got
    for a, b in zip(first, got):
        assert np.array_equal(a, b), "two calls differ"
    return got


@pytest.mark.parametrize("name", ["empty", "one", "deltas", "chunks", "mixed", "align", "many"])
def test_the_writer_equals_the_contract_under_every_cap(cuda, write_sets, name):
    slots, table = write_sets[name]
    S = len(table)
    total = int(RC.to_strings(slots, table, 0)[1][S])
    for cap in sorted({total, max(total - 1, 0), 0, total + 9}):
        want = RC.to_strings(slots, table, cap)
        got = raw_to_strings(cuda, slots, table, cap)
        for g, w, what in zip(got, want, ("bytes", "offsets", "status")):
            assert np.array_equal(g, w), (name, cap, what, np.flatnonzero(g != w)[:8])
    # through ops: the three views of one flat buffer, and the default cap
    d_slots = torch.from_numpy(slots.view(np.int32).copy()).to(cuda)
    d_table = torch.from_numpy(table.copy()).to(cuda)
    flat = torch.full((ops.rle_strings_bytes(S, total + 3),), RC.FENCE8, dtype=torch.uint8, device=cuda)
    data, offsets, status = ops.rle_to_strings(d_slots, d_table, total + 3, out=flat)
    want = RC.to_strings(slots, table, total + 3)
    assert np.array_equal(data.cpu().numpy(), want[0]) and np.array_equal(offsets.cpu().numpy(), want[1])
    assert np.array_equal(status.cpu().numpy(), want[2])
    host = ops.rle_strings_split(flat.cpu().numpy(), S, total + 3)
    assert all(np.array_equal(h, w) for h, w in zip(host, want))
    data, offsets, status = ops.rle_to_strings(d_slots, d_table)
    assert data.numel() == ops.RLE_STRING_CAP_PER_ENTRY * S and int(offsets[S]) == total


def raw_from_strings(cuda, data, offsets, S, sw):
    lib = _lib.load()
    d_data = torch.from_numpy(data.copy()).to(cuda)
    d_off = torch.from_numpy(np.asarray(offsets, np.int64).copy()).to(cuda)
    d_slots = torch.full((S * sw + 2,), RC.FENCE32, dtype=torch.int32, device=cuda)
    d_table = torch.full((S * 4 + 2,), RC.FENCE32, dtype=torch.int32, device=cuda)
    d_status = torch.full((S * 4 + 2,), RC.FENCE32, dtype=torch.int32, device=cuda)
    first = None
    for rep in range(2):
        _lib.check(lib.hgl_rle_from_strings_device(d_data.data_ptr() if len(data) else None, len(data), d_off.data_ptr(), S,
                                                   d_slots.data_ptr() + 4, sw, d_table.data_ptr() + 4, d_status.data_ptr() + 4,
                                                   torch.cuda.current_stream().cuda_stream), "hgl_rle_from_strings_device")
        sl, tb, st = d_slots.cpu().numpy(), d_table.cpu().numpy(), d_status.cpu().numpy()
        for a in (sl, tb, st):
            assert a[0] == RC.FENCE32 and a[-1] == RC.FENCE32, "wrote outside an output"
        got = (sl[1:-1].view(np.uint32).reshape(S, sw).copy(), tb[1:-1].reshape(S, 4).copy(), st[1:-1].reshape(S, 4).copy())
        if rep == 0:
            first = got
    for a, b in zip(first, got):
        assert np.array_equal(a, b), "two calls differ"
    return got


@pytest.mark.parametrize("name", ["empty", "one", "good", "mixed", "random", "tight", "broken", "negative"])
def test_the_reader_equals_the_contract(cuda, read_sets, name):
    data, offsets, S, sw = read_sets[name]
    want = RC.from_strings(data, offsets, S, sw)
    got = raw_from_strings(cuda, data, offsets, S, sw)
    if S == 0:      # nothing launched: table and status keep the fence
        return
    for g, w, what in zip(got, want, ("slots", "table", "status")):
        assert np.array_equal(g, w), (name, what, np.argwhere(g != w)[:8])


def test_the_reader_through_ops_equals_rle_pack_of_the_host_parser(cuda, read_sets):
    """every accepted string: slot and row bit-equal to ops.rle_pack([rle_counts_from_string(s)]) in the words the contract defines"""
    data, offsets, S, sw = read_sets["good"]
    strings = [bytes(data[offsets[s]:offsets[s + 1]]) for s in range(S)]
    buf, off, n_counts = ops.rle_strings_pack(strings)
    assert np.array_equal(off, offsets) and int(n_counts.max()) == sw
    dev = buf.to(cuda, non_blocking=True)
    out = torch.zeros(S * (4 + sw), dtype=torch.int32, device=cuda)      # rle_pack's staging is zeroed: so is this
    slots, table, status = ops.rle_from_strings(dev[8 * (S + 1):], dev[:8 * (S + 1)].view(torch.int64), S, sw, out=out)
    p_slots, p_table = ops.rle_pack([sam.rle_counts_from_string(s) for s in strings], 1, 1, slot_words=sw, device=cuda)
    assert torch.equal(slots, p_slots) and torch.equal(table, p_table)
    assert status.cpu().numpy().tolist() == [[0, int(n), 0, 0] for n in n_counts]


def test_the_round_trip_is_the_identity(cuda, write_sets):
    for name, (slots, table) in write_sets.items():
        S, sw = slots.shape
        if S == 0:
            continue
        d_slots = torch.from_numpy(slots.view(np.int32).copy()).to(cuda)
        d_table = torch.from_numpy(table.copy()).to(cuda)
        total = int(RC.to_strings(slots, table, 0)[1][S])
        data, offsets, status = ops.rle_to_strings(d_slots, d_table, total)
        back, row, st = ops.rle_from_strings(data, offsets, S, sw)
        back, row, st, status = back.cpu().numpy().view(np.uint32), row.cpu().numpy(), st.cpu().numpy(), status.cpu().numpy()
        for s in range(S):
            if status[s] == 0:
                n = int(table[s, 0])
                assert st[s].tolist() == [0, n, 0, 0] and row[s].tolist() == [n, 0, 0, 0] and np.array_equal(back[s, :n], slots[s, :n]), (name, s)
            else:      # an entry without a string reads back as the empty string
                assert st[s].tolist() == [0, 0, 0, 0], (name, s)


@pytest.fixture(scope="module")
def ellipses():
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:64, 0:64]
    m = np.zeros((17, 64, 64), np.uint8)
    for i in range(16):
        cy, cx, a, b = rng.uniform(8, 56), rng.uniform(8, 56), rng.uniform(2, 30), rng.uniform(2, 30)
        m[i] = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1.0
    m[16] = (yy + xx) & 1      # 4096 runs: more than the 128 words of its slot, so the encoder keeps the bit plane (form 1)
    return m


def test_masks_through_the_whole_chain(cuda, ellipses):
    masks = torch.from_numpy(ellipses).to(cuda)
    want = [sam.coco_encode_rle(sam.mask_to_rle(m)) for m in ellipses]
    slots, table = ops.rle_encode(masks)
    assert table.cpu().numpy()[:, 1].tolist() == [0] * 16 + [1]
    data, offsets, status = ops.rle_to_strings(slots, table)
    o, raw = offsets.cpu().numpy(), data.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0] * 16 + [1] and o[17] == o[16]
    for s in range(16):
        assert bytes(raw[o[s]:o[s + 1]]).decode("ascii") == want[s]["counts"], s
    back, row, st = ops.rle_from_strings(data, offsets, 17, int(slots.shape[1]))
    assert st.cpu().numpy()[:, 0].tolist() == [0] * 17
    decoded, code = ops.rle_decode(back, row, 64, 64)
    assert code.cpu().numpy()[:16, 0].tolist() == [0] * 16
    assert np.array_equal(decoded.cpu().numpy()[:16], ellipses[:16])
    # the public pair: the checkerboard is finished on the host, and everything comes back
    got = sam.masks_to_coco_rle(masks)
    assert got == want and got == [sam.coco_encode_rle(r) for r in sam.masks_to_rle(masks)]
    sel = torch.tensor([16, 3, 3, 0], device=cuda)
    assert sam.masks_to_coco_rle(masks, sel) == [want[16], want[3], want[3], want[0]]
    assert sam.masks_to_coco_rle(masks[:0]) == []
    again = sam.coco_rles_to_masks(got, device=cuda)
    assert again.dtype == torch.bool and np.array_equal(again.cpu().numpy(), ellipses.astype(bool))
    assert torch.equal(again, sam.rles_to_masks(got, device=cuda))


def test_strings_that_do_not_read_raise(cuda, ellipses):
    good = [sam.coco_encode_rle(sam.mask_to_rle(m)) for m in ellipses[:3]]
    for bad, code in (("o", 2), ("1" + "o" * 8 + "1", 3)):
        with pytest.raises(ValueError, match=f"entry 1 .*code {code}"):
            sam.coco_rles_to_masks([good[0], {"size": [64, 64], "counts": bad}, good[2]], device=cuda)
    with pytest.raises(ValueError, match="entry 2 does not decode"):
        sam.coco_rles_to_masks([good[0], good[1], {"size": [64, 64], "counts": "5"}], device=cuda)
    with pytest.raises(ValueError, match="entry 0 holds a NUL"):
        sam.coco_rles_to_masks([{"size": [64, 64], "counts": b"1\x00"}], device=cuda)
    with pytest.raises(ValueError, match="entry 1 carries its counts as list"):
        sam.coco_rles_to_masks([good[0], {"size": [64, 64], "counts": [4096]}], device=cuda)


def test_a_cap_too_small_takes_the_second_call(cuda, ellipses):
    masks = torch.from_numpy(ellipses[:16]).to(cuda)
    slots, table = ops.rle_encode(masks)
    want = [sam.coco_encode_rle(sam.mask_to_rle(m))["counts"].encode("ascii") for m in ellipses[:16]]
    assert sam.strings_from_device(slots, table, 64, 64, cap=10) == want == sam.strings_from_device(slots, table, 64, 64)


def test_the_launches_do_not_depend_on_the_set(cuda, write_sets, read_sets):
    def writer(name):
        slots, table = write_sets[name]
        d = torch.from_numpy(slots.view(np.int32).copy()).to(cuda), torch.from_numpy(table.copy()).to(cuda)
        return [k for k, _ in abi_ref.rle_kernels(lambda: ops.rle_to_strings(*d))]

    def reader(name):
        data, offsets, S, sw = read_sets[name]
        d = torch.from_numpy(data.copy()).to(cuda), torch.from_numpy(offsets.copy()).to(cuda)
        return [k for k, _ in abi_ref.rle_kernels(lambda: ops.rle_from_strings(*d, S, sw))]

    three = ["rle_strlengths_kernel", "rle_stroffsets_kernel", "rle_strwrite_kernel"]
    assert writer("one") == three and writer("many") == three and writer("chunks") == three
    assert writer("empty") == three[1:2]
    assert reader("one") == ["rle_strread_kernel"] and reader("random") == ["rle_strread_kernel"] and reader("empty") == []
