"""The buffers a caller lends to the RLE wrappers (`out`, `aux`, `back`, `status`), on the GPU: every wrapper that takes one, and
every such buffer.  A sentinel-filled buffer of the size the layout helper states (ops.rle_block_words, ops.rle_strings_bytes)
comes back as the wrapper's views and holds the bytes the call with out=None returns; a buffer one element short, of another
dtype or strided is refused before any launch and keeps its sentinel.

The world: two images of 4 x 4 and 5 x 3 with 2 and 3 entries and a third image of 2 x 2 that owns none, S = 5.  Every call
runs at two slot widths, "default" and "explicit".  For the wrappers that take their width from the set they are given, default
is the set ops.rle_pack makes (its widest run list) and explicit the one-word set of ops.rle_encode's default; for
rle_remove_small_regions and rle_from_strings the explicit width is one word and two words, smaller than the default.  The
default of rle_encode, rle_from_polygons and rle_merge is one word already at these sizes and the library takes no set of
zero-word slots, so their explicit width is a larger one (6 words: the runs where the default holds planes)."""
import numpy as np
import pytest
import torch

from hybridgl_amd import ops
from hybridgl_amd import sam as hsam

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
SIZES, COUNTS, S, G = [(4, 4), (5, 3), (2, 2)], [2, 3, 0], 5, 3
HW = [16, 16, 15, 15, 15]      # the pixels of every entry's image
RECT = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
POLYGONS = [[RECT(1, 1, 3, 3)], [RECT(0, 0, 1, 4), RECT(2, 3, 4, 4)], [RECT(0, 0, 3, 5)], [RECT(0, 0, 3, 2)], []]


def _masks():
    a, b = np.zeros((2, 4, 4), np.uint8), np.zeros((3, 5, 3), np.uint8)
    a[0, 1:3, 1:3] = 1
    a[1, :, 0] = 1
    a[1, 3, 2:] = 1
    b[0] = 1
    b[1, :2] = 1
    b[2, 0, 0] = 1
    b[2, 2:, 1:] = 1
    return a, b


@pytest.fixture(scope="module")
def world(cuda):
    """the masks on the device, the two encoded sets ("default": rle_pack's, "explicit": one word per entry) and the strings"""
    host = _masks()
    dev = [torch.from_numpy(m).to(cuda) for m in host]
    rles = [hsam.mask_to_rle(m) for ms in host for m in ms]
    runs = [r["counts"] for r in rles]
    planes = [ops.rle_encode(m) for m in dev]
    sets = {"default": ops.rle_pack(runs, 1, 1, device=cuda),
            "explicit": (torch.cat([p[0] for p in planes]).contiguous(), torch.cat([p[1] for p in planes]).contiguous()),
            "image1": {"default": ops.rle_pack(runs[2:], 5, 3, device=cuda), "explicit": planes[1]}}
    assert sets["default"][0].shape[1] > 1 and sets["explicit"][0].shape == (S, 1)
    packed, _, n_counts = ops.rle_strings_pack([hsam.coco_encode_rle(r)["counts"] for r in rles])
    strings = packed.to(cuda)
    torch.cuda.synchronize()
    return {"masks": dev, "sets": sets, "offsets": strings[:8 * (S + 1)].view(torch.int64), "data": strings[8 * (S + 1):],
            "n_counts": int(n_counts.max())}


def _same_set(got, want, hw, lent):
    """two (slots, table): the rows, and of every slot the words its row defines; in a lent buffer the other words kept the fill
    where `lent` says the wrapper leaves them alone"""
    (gs, gt), (ws, wt) = got, want
    assert torch.equal(gt, wt)
    for s, (nc, form) in enumerate(wt[:, :2].tolist()):
        n = nc if form == 0 else (hw[s] + 31) // 32 if form == 1 else 0
        assert n <= gs.shape[1] and torch.equal(gs[s, :n], ws[s, :n]), s
        if lent:
            assert bool((gs[s, n:] == SENT).all()), s


def _cases(world, width, cuda):
    """name -> (call(buffer or None) -> outputs, the buffer's elements, its dtype, which outputs are its views,
    same(got, want, lent): the comparison of a call's outputs with the default call's)"""
    slots, table = world["sets"][width]
    s1, t1 = world["sets"]["image1"][width]
    sw = int(slots.shape[1])
    wider = None if width == "default" else 6
    W, i32, u8 = ops.rle_block_words, torch.int32, torch.uint8
    equal = lambda got, want, lent: all(torch.equal(g, w) for g, w in zip(got, want)) or pytest.fail("outputs differ")
    cases = {}

    cases["rle_encode"] = (lambda b: ops.rle_encode(world["masks"][1], None, wider, out=b), W("set", 3, wider or 1), i32, (0, 1),
                           lambda g, w, lent: _same_set(g, w, HW[2:], False))

    cap = ops.RLE_STRING_CAP_PER_ENTRY * S

    def same_strings(g, w, lent):
        total = int(w[1][S])
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]) and torch.equal(g[0][:total], w[0][:total])
        assert not lent or bool((g[0][total:] == (SENT & 0xFF)).all())      # behind the last string nothing is written
    cases["rle_to_strings"] = (lambda b: ops.rle_to_strings(slots, table, out=b), ops.rle_strings_bytes(S, cap), u8, (0, 1, 2), same_strings)

    fsw = world["n_counts"] if width == "default" else 2      # two words: the longer strings get code 1 and a row that says "no mask"
    from_strings = lambda out, status: ops.rle_from_strings(world["data"], world["offsets"], S, fsw, out=out, status=status)
    same_read = lambda g, w, lent: (_same_set(g[:2], w[:2], HW, False), equal(g[2:], w[2:], lent))
    cases["rle_from_strings out"] = (lambda b: from_strings(b, None), W("set", S, fsw), i32, (0, 1), same_read)
    cases["rle_from_strings status"] = (lambda b: from_strings(None, b), 4 * S, i32, (2,), same_read)

    cases["rle_decode"] = (lambda b: ops.rle_decode(s1, t1, 5, 3, out=b), 3 * 15, u8, (0,), equal)

    flat = lambda o: (*o[0], o[1], o[2])      # (masks of every image, boxes, status)
    cases["rle_decode_group out"] = (lambda b: flat(ops.rle_decode_group(slots, table, SIZES, COUNTS, out=b)), 2 * 16 + 3 * 15, u8, (0, 1, 2), equal)
    cases["rle_decode_group aux"] = (lambda b: flat(ops.rle_decode_group(slots, table, SIZES, COUNTS, aux=b)), W("aux", S), i32, (3, 4), equal)

    def same_nms(g, w, lent):      # (out_idx, out_n, result): of out_idx an image's first out_n entries are defined
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2])
        e = 0
        for n, k in zip(COUNTS, w[1].tolist()):
            assert torch.equal(g[0][e:e + k], w[0][e:e + k])
            e += n
    cases["rle_nms"] = (lambda b: ops.rle_nms(slots, table, SIZES, COUNTS, None, 0.5, out=b), W("nms", S, G=G), i32, (0, 1, 2), same_nms)

    keep = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=cuda)
    cols = torch.arange(2 * S, dtype=torch.float32, device=cuda).reshape(2, S) + 0.5
    select = lambda out, back: ops.rle_select(slots, table, SIZES, COUNTS, keep=keep, cols=cols, out=out, back=back)
    cases["rle_select out"] = (lambda b: select(b, None), W("select", S, sw, C=2), i32, (0, 1, 2),
                               lambda g, w, lent: (_same_set(g[:2], w[:2], HW, lent), equal(g[2:], w[2:], lent)))
    cases["rle_select back"] = (lambda b: select(None, b), W("back", S, G=G), i32, (3, 4),
                                lambda g, w, lent: (_same_set(g[:2], w[:2], HW, False), equal(g[2:], w[2:], lent)))

    wslots, wtable = world["sets"]["default"]      # the clean-up narrows its output: the default is the width of the set it is given
    osw = None if width == "default" else 1
    cases["rle_remove_small_regions"] = (lambda b: ops.rle_remove_small_regions(wslots, wtable, SIZES, COUNTS, 2, "both", slot_words=osw, out=b),
                                         W("clean", S, osw or int(wslots.shape[1])), i32, (0, 1, 2, 3),
                                         lambda g, w, lent: (_same_set(g[:2], w[:2], HW, False), equal(g[2:], w[2:], lent)))

    cases["rle_from_polygons"] = (lambda b: ops.rle_from_polygons(POLYGONS, SIZES, COUNTS, slot_words=wider, device=cuda, out=b),
                                  W("status", S, wider or 1), i32, (0, 1, 2),
                                  lambda g, w, lent: (_same_set(g[:2], w[:2], HW, False), equal(g[2:], w[2:], lent)))

    merge = lambda b: ops.rle_merge(slots, table, SIZES, COUNTS, [[0, 1], [2, 3, 4]], None,
                                    [ops.rle_merge_rule("union", 2), ops.rle_merge_rule("majority", 3)], [1, 1, 0], slot_words=wider, out=b)
    cases["rle_merge"] = (merge, W("status", 2, wider or 1), i32, (0, 1, 2),
                          lambda g, w, lent: (_same_set(g[:2], w[:2], [16, 15], False), equal(g[2:], w[2:], lent)))
    return cases


NAMES = ["rle_encode", "rle_to_strings", "rle_from_strings out", "rle_from_strings status", "rle_decode", "rle_decode_group out",
         "rle_decode_group aux", "rle_nms", "rle_select out", "rle_select back", "rle_remove_small_regions", "rle_from_polygons",
         "rle_merge"]


def _fill(numel, dtype, cuda):
    return torch.full((numel,), SENT if dtype == torch.int32 else SENT & 0xFF, dtype=dtype, device=cuda)


@pytest.mark.parametrize("width", ["default", "explicit"])
@pytest.mark.parametrize("name", NAMES)
def test_a_lent_buffer_holds_what_the_default_call_returns(world, cuda, name, width):
    cases = _cases(world, width, cuda)
    assert sorted(cases) == sorted(NAMES)
    call, numel, dtype, inside, same = cases[name]
    want = call(None)
    buf = _fill(numel, dtype, cuda)
    got = call(buf)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, k
        mine = g.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        assert mine == (k in inside), k      # the views of that very buffer, and nothing else
    begins = sorted((g.data_ptr(), g.numel() * g.element_size()) for k, g in enumerate(got) if k in inside and g.numel())
    assert begins[0][0] == buf.data_ptr() and begins[-1][0] + begins[-1][1] == buf.data_ptr() + numel * buf.element_size()
    assert all(a + n <= b for (a, n), (b, _) in zip(begins, begins[1:]))      # from its first byte to its last, no overlap
    same(got, want, True)
    same(want, want, False)      # (the comparison reads what the default call defines)


@pytest.mark.parametrize("width", ["default", "explicit"])
@pytest.mark.parametrize("name", NAMES)
def test_a_buffer_of_the_wrong_kind_is_refused_and_left_alone(world, cuda, name, width):
    call, numel, dtype, _, _ = _cases(world, width, cuda)[name]
    word = "int32" if dtype == torch.int32 else "uint8"
    other = torch.float32 if dtype == torch.int32 else torch.int8
    short, wrong, wide = _fill(numel - 1, dtype, cuda), torch.full((numel,), 3, dtype=other, device=cuda), _fill(2 * numel, dtype, cuda)
    for bad in (short, wrong, wide[::2]):
        with pytest.raises(ValueError, match=f"expected {numel} {word} elements"):
            call(bad)
    torch.cuda.synchronize()
    fill = SENT if dtype == torch.int32 else SENT & 0xFF
    assert bool((short == fill).all()) and bool((wrong == 3).all()) and bool((wide == fill).all())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="a buffer on another device needs a second device")
@pytest.mark.parametrize("name", NAMES)
def test_a_buffer_on_another_device_is_refused(world, cuda, name):
    call, numel, dtype, _, _ = _cases(world, "default", cuda)[name]
    far = _fill(numel, dtype, torch.device("cuda", 1))
    with pytest.raises(ValueError, match=f"expected {numel} .* elements"):
        call(far)
    torch.cuda.synchronize(1)
    assert bool((far == (SENT if dtype == torch.int32 else SENT & 0xFF)).all())
