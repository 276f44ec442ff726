"""The greedy box NMS (csrc/sam_nms.hip) on every kernel route against the float32 reference of tests/nms_cases.py, on dense,
chained inputs: hgl_nms (the segment kernel on one list: its LDS body up to 512 candidates, its serial body for 513 .. 1024 and
for an unaligned box pointer), hgl_nms_segments (both bodies, one workgroup a list) and hgl_nms_large (rank / mask / scan, any K
up to 32768).

K: 1, 2, around every multiple of 64 that starts a new word of the LDS kernel up to its eighth (448 | 449, 511 | 512), 513 /
1023 / 1024 (serial kernel), 1025 / 4097 / 16390 (W = 17, 65 and 257 words a row: the 256-thread stride loops over removed[]
make a second trip).  At each K every family that fits (clusters at thresholds 0.5 and 0.7, chains at chosen ranks, one chain
as long as K, exact-threshold pairs, ties, degenerate boxes, keep patterns).  Everything is compared exactly, as index lists;
every call is made twice and must repeat itself; routes that take the same input must agree with each other.

Also here, as neighbours of the NMS without a direct test: hgl_gather_masks and hgl_box_near_crop_edge.
"""
import ctypes

import numpy as np
import pytest
import torch

import nms_cases as N
from hybridgl_amd import _lib, ops
from hybridgl_amd import sam as hsam

pytestmark = pytest.mark.gpu
SENTINEL = -7
_REF = {}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def refs(K, thr=None):
    """[(case, the reference's kept list)] of cases_for(K, thr), computed once"""
    if (K, thr) not in _REF:
        _REF[K, thr] = [(c, N.run(c)) for c in N.cases_for(K, thr)]
    return _REF[K, thr]


def twice(fn, *args):
    """-> the kept list; the call is made twice and must repeat itself"""
    (i1, n1), (i2, n2) = fn(*args), fn(*args)
    n = n1.cpu().tolist()
    assert n == n2.cpu().tolist() and len(n) == 1 and 0 <= n[0] <= i1.shape[0], (fn.__name__, n)
    got = i1[:n[0]].cpu().tolist()
    assert got == i2[:n[0]].cpu().tolist(), f"{fn.__name__} is not reproducible"
    return got


def one_segment(b, s, k, thr):
    K = b.shape[0]
    return hsam.nms_segments(b, s, k, torch.tensor([0, K], dtype=torch.int32, device=b.device), K, thr)


def routes_of(K):
    small = [hsam.nms, one_segment] if K <= 1024 else []
    return small + [hsam.nms_large]


@pytest.mark.parametrize("K", N.K_BITS + N.K_SERIAL + N.K_LARGE)
def test_every_route_equals_the_reference(cuda, K):
    bad = []
    for c, ref in refs(K):
        b, s, k = T(c.boxes, cuda), T(c.scores, cuda), T(c.keep, cuda)
        assert b.data_ptr() % 16 == 0
        for fn in routes_of(K):
            got = twice(fn, b, s, k, c.thr)
            if got != ref:
                first = next((i for i, (x, y) in enumerate(zip(got, ref)) if x != y), min(len(got), len(ref)))
                bad.append((c.name, fn.__name__, len(got), len(ref), first))
    assert not bad, f"K={K}: {len(bad)} (case, route, kept, reference kept, first difference) differ: {bad[:12]}"


@pytest.mark.parametrize("K", [1, 2, 64, 65, 192, 449, 512])
def test_serial_kernel_below_513_through_an_unaligned_box_pointer(cuda, K):
    """hgl_nms sends boxes that are not 16-byte aligned (the LDS body loads them as int4) to the serial body: the same lists as
    the aligned call.  hgl_nms_segments and hgl_nms_large refuse such a pointer and launch nothing."""
    lib = _lib.load()
    for c, ref in refs(K):
        flat = torch.zeros(4 * K + 1, dtype=torch.int32, device=cuda)
        flat[1:] = T(c.boxes.reshape(-1), cuda)
        ub = flat[1:].view(K, 4)
        assert ub.data_ptr() % 16 == 4 and ub.is_contiguous()
        s, k = T(c.scores, cuda), T(c.keep, cuda)
        got = twice(hsam.nms, ub, s, k, c.thr)
        assert got == twice(hsam.nms, T(c.boxes, cuda), s, k, c.thr) == ref, (K, c.name)
    idx = torch.full((K,), SENTINEL, dtype=torch.int32, device=cuda)
    n = torch.full((1,), SENTINEL, dtype=torch.int32, device=cuda)
    offs = torch.tensor([0, K], dtype=torch.int32, device=cuda)
    rc = lib.hgl_nms_segments(ub.data_ptr(), s.data_ptr(), k.data_ptr(), offs.data_ptr(), 1, K, 0.7, idx.data_ptr(), n.data_ptr(),
                              ops._stream())
    assert rc != 0 and b"nms_segments: boxes must be 16-byte aligned" in lib.hgl_last_error()
    ws = ops.workspace(lib.hgl_nms_large_workspace_bytes(K), cuda, "nms_large")
    rc = lib.hgl_nms_large(ub.data_ptr(), s.data_ptr(), k.data_ptr(), K, 0.7, idx.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(),
                           ops._stream())
    assert rc != 0 and b"nms_large: boxes must be 16-byte aligned" in lib.hgl_last_error()
    torch.cuda.synchronize()
    assert bool((idx == SENTINEL).all()) and int(n.item()) == SENTINEL
    with pytest.raises(_lib.HybridGLError, match="16-byte aligned"):
        hsam.nms_large(ub, s, k, 0.7)
    with pytest.raises(_lib.HybridGLError, match="16-byte aligned"):
        one_segment(ub, s, k, 0.7)


PICKS = ["clusters", "chain", "ties_zero_one", "keep_none", "long_chain", "degenerate", "ties_nan_inf", "exact_threshold",
         "keep_invalid", "ties_duplicates", "keep_valid", "ties_seam", "ties_all_equal", "keep_last", "ties_signed", "ties_inf"]


def pick(L, i, thr):
    """the case of family PICKS[i] at L candidates (clusters where that family does not fit), with its reference"""
    cs = refs(L, thr)
    return next((cr for cr in cs if cr[0].name.startswith(PICKS[i % len(PICKS)])), cs[0])


def segmented(cuda, lens, max_len, thr=0.7, shift=0):
    """one hgl_nms_segments call over lists of the given lengths, out_idx and out_n pre-filled with a sentinel -> nothing;
    a list longer than max_len admits must keep nothing, every other one equal its reference, and no position at or beyond
    a list's count may be written"""
    lib = _lib.load()
    parts = [pick(L, i + shift, thr) if L else None for i, L in enumerate(lens)]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cat = lambda f: np.concatenate([getattr(p[0], f).reshape(-1) for p in parts if p])
    b, s, k = T(cat("boxes"), cuda), T(cat("scores"), cuda), T(cat("keep"), cuda)
    total = int(offs[-1])
    assert b.numel() == 4 * total and b.data_ptr() % 16 == 0
    results, doffs = [], T(offs, cuda)
    for _ in range(2):
        idx = torch.full((total + 8,), SENTINEL, dtype=torch.int32, device=cuda)
        n = torch.full((len(lens) + 8,), SENTINEL, dtype=torch.int32, device=cuda)
        _lib.check(lib.hgl_nms_segments(b.data_ptr(), s.data_ptr(), k.data_ptr(), doffs.data_ptr(), len(lens), max_len, thr,
                                        idx.data_ptr(), n.data_ptr(), ops._stream()), "hgl_nms_segments")
        results.append((idx.cpu().numpy(), n.cpu().numpy()))
    (idx, n), (idx2, n2) = results
    assert np.array_equal(idx, idx2) and np.array_equal(n, n2), "hgl_nms_segments is not reproducible"
    assert (idx[total:] == SENTINEL).all() and (n[len(lens):] == SENTINEL).all()
    flavours = set()
    for i, L in enumerate(lens):
        o, name = int(offs[i]), parts[i][0].name if parts[i] else "empty"
        want = [] if L == 0 or L > max_len or L > 1024 else parts[i][1]
        assert n[i] == len(want), (i, L, name, int(n[i]), len(want))
        assert idx[o:o + n[i]].tolist() == want, (i, L, name)
        assert (idx[o + n[i]:o + L] == SENTINEL).all(), (i, L, name, "written beyond its count")
        if 0 < L <= max_len:
            flavours.add(L <= 512)
    return flavours


def test_segments_dense_lists_of_both_flavours_in_one_call(cuda):
    assert segmented(cuda, [192] * 16, 192) == {True}
    assert segmented(cuda, [192] * 16, 192, shift=5) == {True}
    assert segmented(cuda, [512, 513, 0, 1, 1024, 64], 1024) == {True, False}
    assert segmented(cuda, [512, 513, 0, 1, 1024, 64], 1024, shift=1) == {True, False}
    assert segmented(cuda, [449, 0, 0, 511], 511) == {True}
    assert segmented(cuda, [1024, 513, 1023], 1024) == {False}


def test_segments_longer_than_max_len_keep_nothing(cuda):
    """nms_segments_kernel: `a list that is empty, or longer than the caller's max_len admits, keeps nothing`"""
    assert segmented(cuda, [600], 512) == set()
    assert segmented(cuda, [1025], 1024) == set()
    assert segmented(cuda, [64, 600, 65], 512) == {True}                # the neighbours of such a list are served as ever
    assert segmented(cuda, [3, 1025, 700, 512], 1024) == {True, False}


def test_nms_large_workspace_reuse(cuda):
    """one stream, one grow-only workspace: 16390 candidates, then 65, then 1 with nothing valid, then 4097.  order[] and
    the mask words of the larger call lie under the smaller one's"""
    seq = [(16390, "clusters@0.7"), (65, "clusters@0.5"), (65, "chain"), (1, "keep_none"), (4097, "clusters@0.7"), (2, "long_chain"),
           (16390, "clusters@0.5")]
    for K, name in seq:
        c, ref = next(cr for cr in refs(K) if cr[0].name.startswith(name))
        got = twice(hsam.nms_large, T(c.boxes, cuda), T(c.scores, cuda), T(c.keep, cuda), c.thr)
        assert got == ref, (K, name)
    ws = ops.workspace(1, cuda, "nms_large")
    assert ws.numel() >= _lib.load().hgl_nms_large_workspace_bytes(16390)     # the large call's buffer serves the small ones
    ws.fill_(0xff)
    for K, name in seq[1:4]:
        c, ref = next(cr for cr in refs(K) if cr[0].name.startswith(name))
        assert twice(hsam.nms_large, T(c.boxes, cuda), T(c.scores, cuda), T(c.keep, cuda), c.thr) == ref, (K, name)


@pytest.mark.parametrize("K", [1, 65, 513, 1025])
def test_nms_large_stays_inside_the_workspace_it_asks_for(cuda, K):
    """a workspace of exactly hgl_nms_large_workspace_bytes(K) in front of guard bytes: the mask has K rows, and
    nms_mask_kernel once wrote all 64 rows of the last row block -- up to 63 x W words beyond the workspace, into whatever
    tensor lay behind it (found by test_every_route_equals_the_reference[513], chain[0-64-128 ...]@0.5 on nms_large: the
    second of the two calls ran on inputs the first had zeroed)"""
    lib = _lib.load()
    need = lib.hgl_nms_large_workspace_bytes(K)
    guard = 64 * ((K + 63) // 64) * 8 + 4096             # a whole row block of W words, and a page
    c, ref = refs(K)[0]
    b, s, k = T(c.boxes, cuda), T(c.scores, cuda), T(c.keep, cuda)
    for _ in range(2):
        buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=cuda)
        assert buf.data_ptr() % 256 == 0
        idx = torch.full((K,), SENTINEL, dtype=torch.int32, device=cuda)
        n = torch.full((1,), SENTINEL, dtype=torch.int32, device=cuda)
        _lib.check(lib.hgl_nms_large(b.data_ptr(), s.data_ptr(), k.data_ptr(), K, c.thr, idx.data_ptr(), n.data_ptr(), buf.data_ptr(),
                                     need, ops._stream()), "hgl_nms_large")
        assert idx[:int(n.item())].cpu().tolist() == ref and bool((idx[int(n.item()):] == SENTINEL).all())
        assert bool((buf[need:] == 0xA5).all()), f"{int((buf[need:] != 0xA5).sum())} bytes written beyond the workspace"
    assert lib.hgl_nms_large(b.data_ptr(), s.data_ptr(), k.data_ptr(), K, c.thr, idx.data_ptr(), n.data_ptr(), buf.data_ptr(),
                             need - 1, ops._stream()) != 0 and b"workspace too small" in lib.hgl_last_error()


def test_the_second_nms_as_the_generator_composes_it(cuda):
    """SamAutomaticMaskGenerator._cleanup: scores `unchanged` in {0, 1}, keep all ones, threshold max(box_nms_thresh,
    crop_nms_thresh) -- through nms_segments with the packed offsets and through nms list by list (above 1024: nms_large)"""
    gen = dict(box_nms_thresh=0.7, crop_nms_thresh=0.7)
    thr = max(gen["box_nms_thresh"], gen["crop_nms_thresh"])
    counts = [192, 64, 700, 0, 5, 1024, 513]
    rng = np.random.default_rng(21)
    lists = []
    for i, c in enumerate(counts):
        boxes = N.cluster_boxes(c, 30 + i) if c else np.zeros((0, 4), np.int32)
        unchanged = (rng.random(c) < 0.8).astype(np.float32)
        lists.append((boxes, unchanged, np.ones(c, np.uint8)))
    want = [N.greedy_nms(b, s, k, thr) for b, s, k in lists]
    assert all(len(w) < 0.6 * c for w, c in zip(want, counts) if c >= 64)
    offs = T(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), cuda)
    nb, sc, kp = (T(np.concatenate([l[j] for l in lists]), cuda) for j in range(3))
    for _ in range(2):
        order, n = hsam.nms_segments(nb, sc, kp, offs, max(counts), thr)
        order, n, o = order.cpu().numpy(), n.cpu().numpy(), 0
        for i, c in enumerate(counts):
            assert order[o:o + n[i]].tolist() == want[i], (i, c)
            o += c
    for (b, s, k), w in zip(lists, want):
        if len(b):
            assert twice(hsam.nms, T(b, cuda), T(s, cuda), T(k, cuda), thr) == w
    b = N.cluster_boxes(1500, 40)
    s = (rng.random(1500) < 0.8).astype(np.float32)
    assert twice(hsam.nms, T(b, cuda), T(s, cuda), torch.ones(1500, dtype=torch.uint8, device=cuda), thr) \
        == N.greedy_nms(b, s, np.ones(1500, np.uint8), thr)


def test_launches(cuda):
    """a single list is one segment: hgl_nms launches the segment kernel of hgl_nms_segments, the same function and
    instantiation, once -- the LDS body for up to 512 aligned candidates, the serial body above and for an unaligned box
    pointer; hgl_nms_large launches its three passes.  No kernel of a single list's own exists."""
    import abi_ref
    thr = 0.7
    case = {K: N.clusters(K, thr) for K in (2, 3, 65, 513)}
    ref = {K: N.run(c) for K, c in case.items()}
    dev = {K: (T(c.boxes, cuda), T(c.scores, cuda), T(c.keep, cuda)) for K, c in case.items()}
    flat = torch.zeros(4 * 3 + 1, dtype=torch.int32, device=cuda)
    flat[1:] = dev[3][0].reshape(-1)
    off4 = flat[1:].view(3, 4)
    assert off4.data_ptr() % 16 == 4
    seen = []

    def launches(call, lens):
        """the kernels of one call (made once before, so that nothing is allocated under the profiler); every list's kept
        candidates must equal the reference"""
        call()
        got = []
        ks = abi_ref.nms_kernels(lambda: got.append(call()))
        idx, n = (x.cpu().numpy() for x in got[0])
        for i, L in enumerate(lens):
            o = sum(lens[:i])
            assert idx[o:o + n[i]].tolist() == ref[L], (lens, i)
        seen.extend(ks)
        return ks

    def single(fn, K, boxes=None):
        b, s, k = dev[K]
        return launches(lambda: fn(b if boxes is None else boxes, s, k, thr), [K])

    def segments(lens, max_len):
        b, s, k = (torch.cat([dev[L][j] for L in lens]) for j in range(3))
        offs = T(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), cuda)
        return launches(lambda: hsam.nms_segments(b, s, k, offs, max_len, thr), lens)

    lds = single(hsam.nms, 3)
    assert len(lds) == 1 and lds == segments([3, 2], 3), lds
    both = segments([3, 513], 513)
    assert len(both) == 2 and both[0] == lds[0] and both[1] != lds[0], (lds, both)
    assert single(hsam.nms, 513) == both[1:] and single(hsam.nms, 3, off4) == both[1:]
    assert lds[0][0] == both[1][0] and {lds[0][1], both[1][1]} == {"0", "1"}, (lds, both)     # one function, its two bodies
    large = single(hsam.nms_large, 65)
    assert len(large) == 3 and len({k for k, _ in large}) == 3 and all(k.startswith("nms_") for k, _ in large), large
    assert not [k for k in seen if k[0] in ("nms_kernel", "nms_bits_kernel")], seen


# ------------------------------------------------------------------------------------------- the NMS's small neighbours
@pytest.mark.parametrize("HW", [16, 16 * 16385])
def test_gather_masks(cuda, HW):
    """out[i] = masks[idx[i]] for i < *n; HW = 16 * 16385: one more 16-byte chunk than the 64 x 256 threads of a row, so
    thread 0 copies twice.  Rows of `out` at and beyond n keep what they held."""
    lib = _lib.load()
    rng = np.random.default_rng(HW)
    src = rng.integers(0, 256, size=(6, HW), dtype=np.uint8)
    src[:, -16:] = np.arange(6, dtype=np.uint8)[:, None] + 200            # the last chunk of every row is its own
    s = T(src, cuda)
    for idx, n, max_n in [([0], 1, 1), ([5, 4, 3, 2, 1, 0], 6, 6), ([3, 3, 0, 3, 5, 5, 1], 7, 7), ([2, 5, 1, 4], 0, 4),
                          ([2, 5, 1, 4], 1, 4), ([5, 0, 5, 2, 4], 3, 5)]:
        di, dn = T(np.array(idx, np.int32), cuda), T(np.array([n], np.int32), cuda)
        for _ in range(2):
            out = torch.full((max_n, HW), 0xA5, dtype=torch.uint8, device=cuda)
            _lib.check(lib.hgl_gather_masks(s.data_ptr(), di.data_ptr(), dn.data_ptr(), max_n, HW, out.data_ptr(), ops._stream()),
                       "hgl_gather_masks")
            out = out.cpu().numpy()
            assert np.array_equal(out[:n], src[idx[:n]]), (idx, n)
            assert (out[n:] == 0xA5).all(), (idx, n, "rows beyond n written")
    assert lib.hgl_gather_masks(s.data_ptr(), s.data_ptr(), s.data_ptr(), 1, 24, s.data_ptr(), ops._stream()) != 0
    assert b"multiple of 16" in lib.hgl_last_error()


def near_crop_edge(boxes, crop, orig, atol):
    """is_box_near_crop_edge (utils/amg.py:78-88) in float32 numpy: isclose with rtol = 0 is |a - b| <= atol"""
    crop, orig = np.asarray(crop, np.float32), np.asarray(orig, np.float32)
    b = (boxes + np.array([crop[0], crop[1], crop[0], crop[1]], boxes.dtype)).astype(np.float32)     # uncrop_boxes_xyxy
    near_crop = np.abs(b - crop[None]) <= np.float32(atol)
    near_image = np.abs(b - orig[None]) <= np.float32(atol)
    return (near_crop & ~near_image).any(1)


def edge_boxes(crop):
    """boxes in crop coordinates with ONE edge 19, 20 or 21 from its crop edge, inside and outside, the other three 60 away
    from theirs; and one box far from every edge"""
    cw, ch = crop[2] - crop[0], crop[3] - crop[1]
    far = [60, 60, cw - 60, ch - 60]
    out = [far]
    for e, at in enumerate([0, 0, cw, ch]):
        for d in (19, 20, 21, -19, -20, -21):
            b = list(far)
            b[e] = at + d
            out.append(b)
    return np.array(out, np.int32)


@pytest.mark.parametrize("K", [1, 256, 257])
def test_box_near_crop_edge(cuda, K):
    orig = [0, 0, 1000, 800]
    crops = [[200, 150, 700, 600],                      # every crop edge inside the image
             [0, 0, 500, 400], [500, 400, 1000, 800],   # two crop edges ARE image edges: exempt
             [10, 15, 985, 790], [20, 21, 979, 780]]    # crop edges within 20 of the image's, and at 20 | 21 from them
    seen = set()
    for ci, crop in enumerate(crops):
        base = edge_boxes(crop)
        boxes = base[(np.arange(K) + ci) % len(base)]
        keep0 = np.ones(K, np.uint8)
        keep0[2::5] = 0                                 # keep already 0 stays 0
        want = keep0 & ~near_crop_edge(boxes.astype(np.int64), crop, orig, 20.0)
        for _ in range(2):
            keep = T(keep0, cuda)
            got = hsam.box_near_crop_edge(T(boxes, cuda), keep, crop, orig, atol=20.0)
            assert got.data_ptr() == keep.data_ptr()
            assert np.array_equal(got.cpu().numpy(), want), (K, crop, np.nonzero(got.cpu().numpy() != want)[0][:8])
        seen |= {(ci, bool(w)) for w in want[keep0 == 1]}
    if K >= 256:
        assert seen == {(ci, w) for ci in range(len(crops)) for w in (False, True)}
    # the reference itself: 19 and 20 are near, 21 is not; an edge that is the image's is exempt
    b = edge_boxes(crops[0])
    assert near_crop_edge(b, crops[0], orig, 20.0).tolist() == [False] + [True, True, False] * 8
    assert not near_crop_edge(edge_boxes(crops[1])[1:7], crops[1], orig, 20.0).any()
