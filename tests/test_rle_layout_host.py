"""The flat-buffer layouts of the RLE entries (ops.RLE_BLOCKS / rle_block / rle_block_words), the one check of a lent buffer
(ops._out) and the one check of a group call (ops._rle_group), on the host.  Every layout is restated here by hand, in the
form the wrappers spelled it before they shared the table: slices of the flat buffer and byte offsets from its base."""
import itertools

import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import proposals as P


def _by_hand(name, f, S, sw, G, C, Sb):
    """[(part, its first int32 element)] of block `name` in the flat buffer f (exactly the block's size), written out"""
    if name == "set":
        return [(f[:4 * S].reshape(S, 4), 0), (f[4 * S:4 * S + S * sw].reshape(S, sw), 4 * S)]
    if name == "status":
        return _by_hand("set", f, S, sw, G, C, Sb) + [(f[S * (4 + sw):].reshape(S, 4), S * (4 + sw))]
    if name == "clean":
        return _by_hand("set", f, S, sw, G, C, Sb) + [(f[S * (4 + sw):S * (8 + sw)].reshape(S, 4), S * (4 + sw)),
                                                      (f[S * (8 + sw):].reshape(S, 4), S * (8 + sw))]
    if name == "select":
        return _by_hand("set", f, S, sw, G, C, Sb) + [(f[S * (4 + sw):].reshape(C, S), S * (4 + sw))]
    if name == "group":      # C: 1 with the area bits, else 0
        return _by_hand("set", f, S, sw, G, C, Sb) + [(f[S * (4 + sw):S * (6 + sw)].reshape(2, S), S * (4 + sw)),
                                                      (f[S * (6 + sw):S * (7 + sw)], S * (6 + sw))]
    if name == "back":
        return [(f[:S], 0), (f[S:], S)]
    if name == "nms":
        return [(f[:S], 0), (f[S:5 * S].reshape(S, 4), S), (f[5 * S:], 5 * S)]
    if name == "aux":
        return [(f.reshape(2, S, 4)[0], 0), (f.reshape(2, S, 4)[1], 4 * S)]
    if name == "match":
        return [(f.reshape(S + Sb, 4)[:S], 0), (f.reshape(S + Sb, 4)[S:], 4 * S)]
    raise KeyError(name)


WORDS = {"set": lambda S, sw, G, C, Sb: S * (4 + sw), "status": lambda S, sw, G, C, Sb: S * (8 + sw),
         "clean": lambda S, sw, G, C, Sb: S * (12 + sw), "select": lambda S, sw, G, C, Sb: S * (4 + sw + C),
         "group": lambda S, sw, G, C, Sb: S * (6 + sw + C), "back": lambda S, sw, G, C, Sb: S + G,
         "nms": lambda S, sw, G, C, Sb: S * 5 + G, "aux": lambda S, sw, G, C, Sb: 8 * S, "match": lambda S, sw, G, C, Sb: 4 * (S + Sb)}


def test_every_block_of_the_table_is_restated_here():
    assert sorted(ops.RLE_BLOCKS) == sorted(WORDS)


@pytest.mark.parametrize("name", sorted(WORDS))
def test_a_block_is_the_slices_the_wrappers_wrote_by_hand(name):
    for S, sw, G, C in itertools.product((0, 1, 5), (1, 9, 80), (1, 3), (0, 2)):
        if name == "group":
            C = C // 2      # the area bits: there or not
        Sb = C + 1          # the second set of "match": 1 or 3 entries
        words = ops.rle_block_words(name, S, sw, G=G, C=C, Sb=Sb)
        assert words == WORDS[name](S, sw, G, C, Sb) == ops.rle_block_ends(name, S, sw, G=G, C=C, Sb=Sb)[-1]
        host = np.arange(words, dtype=np.int32)
        tensor = torch.arange(words, dtype=torch.int32)
        base = tensor.data_ptr()
        for flat in (host, tensor):
            parts = ops.rle_block(name, flat, S, sw, G=G, C=C, Sb=Sb)
            want = _by_hand(name, flat, S, sw, G, C, Sb)
            assert len(parts) == len(want)
            at = 0
            for p, (w, first) in zip(parts, want):
                assert tuple(p.shape) == tuple(w.shape), (name, S, sw, G, C)
                a = p if flat is host else p.numpy()
                assert np.array_equal(a, w if flat is host else w.numpy())
                # consecutive, without a gap or an overlap: a part begins where the one before it ended
                assert first == at and (a.size == 0 or (int(a.reshape(-1)[0]) == at and int(a.reshape(-1)[-1]) == at + a.size - 1))
                at += a.size
                if a.size:
                    assert np.shares_memory(a, host if flat is host else tensor.numpy())
                if flat is tensor:      # the pointer a kernel gets: the base plus the bytes the wrappers added by hand
                    assert p.data_ptr() == (base + 4 * first if p.numel() else 0)      # (torch gives no pointer into a part of no element,
                    assert ops._ptr(p) == (base + 4 * first if words else 0)           # and the slots are named also where slot_words is 0)
            assert at == words
    if name == "set":
        flat = torch.arange(5 * (4 + 9), dtype=torch.int32)
        slots, table = ops.rle_split(flat, 5, 9)
        assert table.data_ptr() == flat.data_ptr() and slots.data_ptr() == flat.data_ptr() + 16 * 5
        assert torch.equal(table, flat[:20].reshape(5, 4)) and torch.equal(slots, flat[20:].reshape(5, 9))


def test_the_pointers_of_the_entries_are_the_ones_added_by_hand():
    """base + 16 * S, base + 4 * S * (4 + sw), base + 4 * S * (8 + sw): what the wrappers passed before the views' own pointers"""
    S, sw = 5, 9
    flat = torch.zeros(S * (12 + sw), dtype=torch.int32)
    base = flat.data_ptr()
    table, slots, boxes, result = ops.rle_block("clean", flat, S, sw)
    assert [t.data_ptr() for t in (table, slots, boxes, result)] == [base, base + 16 * S, base + 4 * S * (4 + sw), base + 4 * S * (8 + sw)]
    table, slots, status = ops.rle_block("status", flat[:S * (8 + sw)], S, sw)
    assert [t.data_ptr() for t in (table, slots, status)] == [base, base + 16 * S, base + 4 * S * (4 + sw)]
    table, slots, cols = ops.rle_block("select", flat[:S * (4 + sw + 2)], S, sw, C=2)
    assert [t.data_ptr() for t in (table, slots, cols)] == [base, base + 16 * S, base + 4 * S * (4 + sw)]
    table, slots, boxes, result = ops.rle_block("clean", flat[:S * 12], S, 0)      # slots of no word: torch has no pointer, _ptr names them
    assert slots.shape == (S, 0) and slots.data_ptr() == 0
    assert [ops._ptr(t) for t in (table, slots, boxes, result)] == [base, base + 16 * S, base + 4 * S * (4 + 0), base + 4 * S * (8 + 0)]


@pytest.mark.parametrize("area", [False, True])
def test_the_staged_group_of_the_proposal_store_is_one_more_block(area):
    for S, sw in itertools.product((0, 1, 5), (1, 9, 80)):
        words = P._group_words(S, sw, area)
        assert words == S * (6 + sw + bool(area))
        for flat in (np.arange(words, dtype=np.int32), torch.arange(words, dtype=torch.int32)):
            slots, table, cols, extra = P._split_group(flat, S, sw, area)
            want = (flat[4 * S:4 * S + S * sw].reshape(S, sw), flat[:4 * S].reshape(S, 4), flat[S * (4 + sw):S * (6 + sw)].reshape(2, S),
                    flat[S * (6 + sw):S * (7 + sw)])
            for p, w in zip((slots, table, cols, extra), want):
                assert tuple(p.shape) == tuple(w.shape) and np.array_equal(np.asarray(p), np.asarray(w))
            assert len(extra) == (S if area else 0)
            assert sum(int(np.asarray(p).size) for p in (slots, table, cols, extra)) == words


@pytest.mark.parametrize("thin, device_strings", list(itertools.product([False, True], repeat=2)))
def test_the_read_back_takes_its_sizes_from_the_blocks(thin, device_strings):
    for S, G in itertools.product((0, 1, 5), (1, 3)):
        t = int(thin)
        e = np.cumsum([0, 8 * S, t * S, t * G, t * S, 4 * t * S, t * G, 4 * S * device_strings]).tolist()
        words, part = P._back_layout(S, G, thin, device_strings)
        assert words == e[7] == 8 * S + t * (6 * S + 2 * G) + 4 * S * device_strings
        assert part == {"aux": slice(e[0], e[1]), "out_src": slice(e[1], e[2]), "out_n": slice(e[2], e[3]), "nms": slice(e[3], e[6]),
                        "codes": slice(e[4], e[5]), "read": slice(e[6], e[7])}
        if thin:      # the stretches group_begin lends are the blocks' sizes
            assert part["nms"].stop - part["nms"].start == ops.rle_block_words("nms", S, G=G)
            assert part["out_n"].stop - part["out_src"].start == ops.rle_block_words("back", S, G=G)
        assert part["aux"].stop == ops.rle_block_words("aux", S)


CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype, word", [(torch.int32, "int32"), (torch.uint8, "uint8")])
def test_the_out_check_refuses_what_a_kernel_must_not_get(dtype, word):
    n = 24
    fresh = ops._out(None, n, dtype, CPU, "out")
    assert fresh.shape == (n,) and fresh.dtype == dtype and fresh.device == CPU and fresh.is_contiguous()
    own = torch.zeros((2, n // 2), dtype=dtype)      # any contiguous shape of the right element count: handed back flat
    got = ops._out(own, n, dtype, CPU, "out")
    assert got.shape == (n,) and got.data_ptr() == own.data_ptr()
    got[5] = 7
    assert int(own[0, 5]) == 7
    other = torch.float32 if dtype == torch.int32 else torch.int8
    for bad in (torch.zeros(n - 1, dtype=dtype), torch.zeros(n + 1, dtype=dtype), torch.zeros(n, dtype=other),
                torch.zeros(2 * n, dtype=dtype)[::2], torch.zeros((n // 2, 4), dtype=dtype)[:, :2],
                torch.empty(n, dtype=dtype, device="meta")):
        with pytest.raises(ValueError, match=f"out: expected {n} {word} elements"):
            ops._out(bad, n, dtype, CPU, "out")
    with pytest.raises(ValueError, match="aux: expected 0 int32 elements"):
        ops._out(torch.zeros(1, dtype=torch.int32), 0, torch.int32, CPU, "aux")
    assert ops._out(torch.zeros((0, 4), dtype=torch.int32), 0, torch.int32, CPU, "status").shape == (0,)


def test_the_group_check_refuses_counts_that_do_not_describe_the_set(monkeypatch):
    monkeypatch.setattr(ops, "_dev", lambda t, dtype, name: t.data_ptr())      # host tensors stand in: nothing is launched here
    sizes = [(4, 4), (5, 3), (2, 2)]
    slots, table = torch.zeros((5, 9), dtype=torch.int32), torch.zeros((5, 4), dtype=torch.int32)
    sets, images, total, G = ops._rle_group("op", [(slots, table)], ops.rle_nms_layout, sizes, [2, 3, 0])
    assert sets == [(slots.data_ptr(), 9, table.data_ptr(), 5)] and (total, G) == (0, 3)
    assert images.dtype == np.int64 and images.tolist() == [[4, 4, 0], [5, 3, 2], [2, 2, 5]]
    _, images, total, _ = ops._rle_group("op", [(slots, table)], ops.rle_group_layout, sizes, [2, 3, 0])
    assert images.tolist() == [[4, 4, 0, 0], [5, 3, 2, 32], [2, 2, 5, 77]] and total == 77
    _, images, _, _ = ops._rle_group("op", [(slots, table)], ops.rle_select_layout, sizes, [2, 3, 0], max_keep=[1, None, -4])
    assert images.tolist() == [[4, 4, 0, 1], [5, 3, 2, -1], [2, 2, 5, -1]]
    # an entry count stands for a set that does not exist yet (rle_from_polygons, the output of rle_merge)
    sets, images, _, G = ops._rle_group("op", [(slots, table), 4], ops.rle_merge_layout, sizes, [2, 3, 0], [1, 1, 2])
    assert sets[1] == (None, 0, None, 4) and images.tolist() == [[4, 4, 0, 0], [5, 3, 2, 1], [2, 2, 5, 2]]
    for counts in ([2, 2, 0], [2, 3, 1]):      # short, long
        with pytest.raises(ValueError, match="op: counts sum"):
            ops._rle_group("op", [(slots, table)], ops.rle_nms_layout, sizes, counts)
        with pytest.raises(ValueError, match="op: counts sum"):
            ops._rle_group("op", [5], ops.rle_nms_layout, sizes, counts)
    with pytest.raises(ValueError, match="image 1 has -1"):      # the sum alone would pass
        ops._rle_group("op", [(slots, table)], ops.rle_nms_layout, sizes, [6, -1, 0])
    with pytest.raises(ValueError, match="3 sizes and 2 counts"):
        ops._rle_group("op", [(slots, table)], ops.rle_nms_layout, sizes, [2, 3])
    with pytest.raises(ValueError, match="3 sizes, 3 and 2 counts"):
        ops._rle_group("op", [(slots, table), (slots, table)], ops.rle_match_layout, sizes, [2, 3, 0], [2, 3])
    with pytest.raises(ValueError, match="counts sum to 4, the set has 5"):      # the second of two sets
        ops._rle_group("op", [(slots, table), (slots, table)], ops.rle_match_layout, sizes, [2, 3, 0], [2, 2, 0])
    with pytest.raises(ValueError, match=r"expected slots \[S, slot_words\] and table \[S, 4\]"):      # a set of two lengths
        ops._rle_group("op", [(slots, table[:4])], ops.rle_nms_layout, sizes, [2, 3, 0])
    assert ops.rle_clean_layout is ops.rle_nms_layout
