"""hgl_rle_nms_device (csrc/rle.hip) through ops.rle_nms: greedy suppression by mask overlap inside an encoded set, image by image.
Equality, no tolerance: the kept flags equal what the reference's rleNms stored (tests/golden/rle_nms_fuzz.npz, pinned on the host
by tests/test_rle_nms_abi.py) for every threshold and order; out_idx / out_n, rank, by and area equal the greedy numpy walk over
dense float64 ratios (tests/rle_nms_cases.py) -- on both slot forms, every list alone and the lists of several shapes in one call;
the second metric, an entry that holds no mask, determinism, containment with guard words, the refusals."""
import numpy as np
import pytest
import torch

from hybridgl_amd import _lib, ops

import rle_nms_cases as NC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
_enc, _cnt = {}, {}


def counts_of(name, masks):
    if name not in _cnt:
        _cnt[name] = NC.counts(masks)
    return _cnt[name]


def encoded(name, masks, form, device):
    """(slots, table) of a list as ops.rle_encode hands it out; form 0: slots that hold any run list; form 1: slots of
    ceil(H*W/32) words, so a mask with more runs than that comes as its bit plane"""
    key = (name, form)
    if key not in _enc:
        n, H, W = masks.shape
        s, t = ops.rle_encode(torch.from_numpy(masks).to(device), slot_words=H * W + 1 if form == 0 else ops.rle_slot_words(H, W))
        forms = t[:, 1].cpu().numpy()
        assert (forms == 0).all() if form == 0 else set(forms.tolist()) <= {0, 1}
        _enc[key] = (s.contiguous(), t.contiguous())
    return _enc[key]


def join(sets, device):
    """per-image (slots, table) sets of their own slot sizes -> one set of the widest slot"""
    sw = max([int(s.shape[1]) for s, _ in sets] + [1])
    slots = [torch.cat([s, torch.full((s.shape[0], sw - s.shape[1]), POISON, dtype=torch.int32, device=device)], 1) for s, _ in sets]
    return torch.cat(slots).contiguous(), torch.cat([t for _, t in sets]).contiguous()


def check(got, lists, thr, scored, metric, dead=None):
    """got = (out_idx, out_n, result) on the host against the numpy walk of every image; lists: [(name, masks, scores) or None
    for an image without an entry]; -> the kept flags per image"""
    out_idx, out_n, result = got
    e, flags = 0, []
    for g, item in enumerate(lists):
        if item is None:
            assert out_n[g] == 0
            flags.append(np.zeros(0, np.uint8))
            continue
        name, masks, scores = item
        n = len(masks)
        inter, area = counts_of(name, masks)
        gone = set(dead.get(g, ())) if dead else set()
        kept, rank, by = NC.greedy(inter, area, NC.walk_order(scores if scored else None, n), thr, metric, gone)
        where = (name, thr, scored, metric)
        assert out_n[g] == len(kept) and out_idx[e:e + len(kept)].tolist() == kept, where
        r = result[e:e + n]
        assert r[:, 2].tolist() == rank.tolist(), where
        assert r[:, 3].tolist() == by.tolist(), where
        assert r[:, 0].tolist() == [2 if i in gone else 0 for i in range(n)], where
        assert r[:, 1].tolist() == [0 if i in gone else int(area[i]) for i in range(n)], where
        f = np.zeros(n, np.uint8)
        f[kept] = 1
        flags.append(f)
        e += n
    return flags


def call(slots, table, lists, thr, scored, metric="iou"):
    sizes = [item[1].shape[1:] if item else (5, 7) for item in lists]
    counts = [len(item[1]) if item else 0 for item in lists]
    scores = None
    if scored:
        scores = torch.from_numpy(np.concatenate([item[2] for item in lists if item])).to(slots.device)
    return tuple(x.cpu().numpy() for x in ops.rle_nms(slots, table, sizes, counts, scores, thr, metric))


def stored_flags(name, thr, scored):
    """rleNms's keep vector for this list, threshold and order, or None when the file holds none"""
    z = NC.golden()
    if name + "_thr" not in z:
        return None
    hit = np.flatnonzero(z[name + "_thr"] == thr)
    return z[name + "_keep"][hit[0], int(scored)] if len(hit) else None


ALONE = [(name, form) for name, *_ in NC.sets() for form in (0, 1)]


@pytest.mark.parametrize("name,form", ALONE, ids=[f"{n}-form{f}" for n, f in ALONE])
def test_a_list_alone_against_rlenms_and_the_numpy_walk(name, form, cuda):
    device = cuda
    _, H, W, masks, scores = next(s for s in NC.sets() if s[0] == name)
    slots, table = encoded(name, masks, form, device)
    z = NC.golden()
    thresholds = z[name + "_thr"].tolist() if name + "_thr" in z else NC.BASE_THR
    compared = 0
    for thr in thresholds:
        for scored in (False, True):
            got = call(slots, table, [(name, masks, scores)], thr, scored)
            flags = check(got, [(name, masks, scores)], thr, scored, 0)[0]
            want = stored_flags(name, thr, scored)
            if want is not None:
                assert np.array_equal(flags, want), (name, thr, scored)
                compared += 1
    assert compared == (22 if name[0] in "sc" else 0)
    if form == 1 and name[0] in "se" and H * W >= 2000:      # the noise masks of the larger shapes come as bit planes
        assert (table[:, 1] == 1).any()


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("form", [0, 1])
def test_the_lists_of_two_shapes_in_one_call_of_eight_images(half, form, cuda):
    """six lists and two images without an entry, one of them between two shapes and one at the end"""
    device = cuda
    mine = [s for s in NC.sets() if int(s[0][1]) // 2 == half]
    lists = [(name, masks, scores) for name, _, _, masks, scores in mine]
    lists = lists[:3] + [None] + lists[3:] + [None]
    assert len(lists) == 8
    slots, table = join([encoded(it[0], it[1], form, device) for it in lists if it], device)
    z = NC.golden()
    extra = sorted({float(t) for it in lists if it and it[0] + "_thr" in z for t in z[it[0] + "_thr"][5:]})
    compared = 0
    for thr in sorted(set(NC.BASE_THR + extra)):      # a pair's exact ratio may be a base threshold: the chains meet 0.5
        for scored in (False, True):
            flags = check(call(slots, table, lists, thr, scored), lists, thr, scored, 0)
            for it, f in zip(lists, flags):
                want = stored_flags(it[0], thr, scored) if it else None
                if want is not None:
                    assert np.array_equal(f, want), (it[0], thr, scored)
                    compared += 1
    # every stored vector of the call's four lists was met (two lists may share a threshold: the chains' ratios are the same)
    assert compared == sum(2 * len(np.unique(z[it[0] + "_thr"])) for it in lists if it and it[0] + "_thr" in z) >= 4 * 2 * 8


def test_containment_and_the_edge_lists_against_the_numpy_walk(cuda):
    device = cuda
    fell = 0
    for name, H, W, masks, scores in NC.sets():
        slots, table = encoded(name, masks, 1, device)
        for thr in NC.BASE_THR:
            for scored in (False, True):
                flags = check(call(slots, table, [(name, masks, scores)], thr, scored, "containment"),
                              [(name, masks, scores)], thr, scored, 1)[0]
                fell += int(len(masks) - flags.sum())
    assert fell > 0
    # a part nested in a whole falls to it, and the whole to the part when the part ranks first; IoU keeps both
    H, W = 20, 12
    m = np.zeros((2, H, W), np.uint8)
    m[0, 2:18, 1:11] = 1
    m[1, 5:9, 3:6] = 1
    s, t = ops.rle_encode(torch.from_numpy(m).to(device))
    for sc, kept in ((None, [0]), ([0.1, 0.9], [1])):
        sc = None if sc is None else torch.tensor(sc, device=device)
        out_idx, out_n, result = (x.cpu().numpy() for x in ops.rle_nms(s, t, [(H, W)], [2], sc, 0.9, "containment"))
        assert out_n.tolist() == [1] and out_idx[:1].tolist() == kept and result[1 - kept[0], 3] == kept[0]
        assert ops.rle_nms(s, t, [(H, W)], [2], sc, 0.9, "iou")[1].cpu().tolist() == [2]


def test_an_entry_that_holds_no_mask(cuda):
    """form 2 in the middle of a list: not kept, suppresses nobody, its neighbours' results are those of the list without it; the
    words behind an entry's counts are not read"""
    device = cuda
    name, H, W, masks, scores = NC.sets("s")[0]
    slots, table = encoded(name, masks, 0, device)
    n = len(masks)
    dead = 7
    slots, table = slots.clone(), table.clone()
    cols = torch.arange(slots.shape[1], device=device)[None, :]
    slots[cols >= table[:, :1]] = POISON      # every word behind the counts
    table[dead, 1] = 2
    slots[dead] = POISON
    rest = [i for i in range(n) if i != dead]
    sub = (name + "-without", masks[rest], scores[rest])
    idx = torch.tensor(rest, device=device)
    for thr in (0.0, 0.3, 0.7):
        for scored in (False, True):
            got = call(slots, table, [(name, masks, scores)], thr, scored)
            check(got, [(name, masks, scores)], thr, scored, 0, dead={0: [dead]})
            assert got[2][dead].tolist() == [2, 0, -1, -1] and dead not in got[0][:got[1][0]].tolist()
            less = call(slots[idx].contiguous(), table[idx].contiguous(), [sub], thr, scored)
            check(less, [sub], thr, scored, 0)
            back = np.asarray(rest)
            assert less[1][0] == got[1][0] and back[less[0][:less[1][0]]].tolist() == got[0][:got[1][0]].tolist()
            assert np.array_equal(less[2][:, :3], got[2][rest][:, :3])
            assert np.where(less[2][:, 3] >= 0, back[less[2][:, 3]], -1).tolist() == got[2][rest][:, 3].tolist()


def raw(lib, slots, table, images, scores, thr, metric, fill, device, guard=64):
    """the C entry on buffers pre-filled with `fill` and fenced by guard words; -> (rc, out_idx, out_n, result, fences intact)"""
    S, G = int(slots.shape[0]), len(images)
    images = np.ascontiguousarray(images, dtype=np.int64)
    bufs = [torch.full((n + 2 * guard,), fill, dtype=torch.int32, device=device) for n in (S, G, 4 * S)]
    need = lib.hgl_rle_nms_workspace_bytes(images.ctypes.data, G, S, int(slots.shape[1]))
    ws = torch.full((max(need, 1),), fill & 0xFF, dtype=torch.uint8, device=device)
    rc = lib.hgl_rle_nms_device(slots.data_ptr(), int(slots.shape[1]), table.data_ptr(), S, images.ctypes.data, G,
                                scores.data_ptr() if scores is not None else None, thr, metric,
                                *[b.data_ptr() + 4 * guard for b in bufs], ws.data_ptr() if need else None, need,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    fences = all((h[:guard] == fill).all() and (h[-guard:] == fill).all() for h in host)
    return (rc, *[h[guard:-guard] for h in host], fences)


def test_determinism_containment_and_refusals_on_the_c_entry(cuda):
    device = cuda
    lib = _lib.load()
    mine = [s for s in NC.sets("sc") if s[0][1] in "02"]      # 70 x 37 and 3 x 50: s0 c0 s2 c2
    slots, table = join([encoded(s[0], s[3], 1, device) for s in mine], device)
    images = ops.rle_nms_layout([s[3].shape[1:] for s in mine], [len(s[3]) for s in mine])
    scores = torch.from_numpy(np.concatenate([s[4] for s in mine])).to(device)
    counts = [len(s[3]) for s in mine]
    a = raw(lib, slots, table, images, scores, 0.5, 0, 0x11111111, device)
    b = raw(lib, slots, table, images, scores, 0.5, 0, 0x77777777, device)
    assert a[0] == b[0] == 0 and a[4] and b[4]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    e = 0
    for g, n in enumerate(counts):      # the kept part is the same; what lies behind it keeps the caller's bytes
        k = int(a[2][g])
        assert np.array_equal(a[1][e:e + k], b[1][e:e + k])
        assert (a[1][e + k:e + n] == 0x11111111).all() and (b[1][e + k:e + n] == 0x77777777).all()
        e += n
    lists = [(s[0], s[3], s[4]) for s in mine]
    check((a[1], a[2], a[3].reshape(-1, 4)), lists, 0.5, True, 0)
    # scores = None is the walk of scores that fall strictly in the stored order
    falling = torch.cat([torch.arange(n, 0, -1, dtype=torch.float32) for n in counts]).to(device)
    c = raw(lib, slots, table, images, None, 0.3, 0, 0, device)
    d = raw(lib, slots, table, images, falling, 0.3, 0, 0, device)
    assert c[0] == d[0] == 0 and all(np.array_equal(x, y) for x, y in zip(c[1:4], d[1:4]))
    # refused: nothing is enqueued, so nothing is written
    many = torch.zeros((4097, 1), dtype=torch.int32, device=device), torch.zeros((4097, 4), dtype=torch.int32, device=device)
    for what, args in {"NaN thr": (slots, table, images, scores, float("nan"), 0), "metric 2": (slots, table, images, scores, 0.5, 2),
                       "metric -1": (slots, table, images, None, 0.5, -1),
                       "4097 entries": (*many, np.asarray([[4, 4, 0]]), None, 0.5, 0),
                       "entries step back": (slots, table, images[[0, 2, 1, 3]], None, 0.5, 0)}.items():
        rc, oi, on, res, fences = raw(lib, *args, 0x33333333, device)
        assert rc == -1 and fences, what
        assert (oi == 0x33333333).all() and (on == 0x33333333).all() and (res == 0x33333333).all(), what
    with pytest.raises(ValueError):
        ops.rle_nms(slots, table, [s[3].shape[1:] for s in mine], counts, None, 0.5, "dice")
    with pytest.raises(ValueError):
        ops.rle_nms(slots, table, [s[3].shape[1:] for s in mine], counts, None, float("nan"))
    # no entry: no launch, no workspace; ops hands out zero counts
    oi, on, res = ops.rle_nms(slots[:0], table[:0], [(4, 4), (5, 5)], [0, 0])
    assert oi.numel() == 0 and on.cpu().tolist() == [0, 0] and tuple(res.shape) == (0, 4)
