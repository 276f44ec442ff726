"""What the clean-up of encoded sets (hgl_rle_clean_device, csrc/rle_clean.hip) is judged on, plain numpy, no GPU code: the
contract -- host codec -> flood fill holes -> flood fill islands -> host encode -> box -- and the case list: every pattern of
ccl_cases.cases(H, W) AND ITS TRANSPOSE (the seams of the byte kernels are row strips; this kernel's are column boundaries and
64-row words) at shapes around one and two column words, with ccl_cases.thresholds at each, and the hand-built bridges.  The
oracle is ccl_cases.flood_components / flood_remove_small_regions; rle_clean_plan (csrc/rle_group.h) and the workspace
arithmetic of csrc/rle_clean.hip are restated in Python."""
import numpy as np

import ccl_cases as CC
import rle_nms_cases as NC

SHAPES = [(1, 1), (1, 70), (70, 1), (2, 37), (63, 17), (64, 64), (65, 33), (129, 65), (37, 130), (128, 24)]
MODES = {"holes": 1, "islands": 2, "both": 3}


# ---------------------------------------------------------------------------------------------------------- the host codec
def counts_of(mask):
    """column-major run lengths of a bool [H,W] mask, zeros first (utils/amg.py:107-136) -> uint32 array"""
    f = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.flatnonzero(f[1:] != f[:-1]) + 1
    c = np.diff(np.concatenate([[0], edges, [f.size]]))
    return (np.concatenate([[0], c]) if f[0] else c).astype(np.uint32)


def mask_of(counts, H, W):
    """the inverse, clipped at H*W as the decoders clip -> (bool [H,W], the counts sum to H*W)"""
    f = np.zeros(H * W, dtype=bool)
    p = 0
    for k, c in enumerate(np.asarray(counts, dtype=np.uint64).tolist()):
        q = min(p + c, H * W)
        if k & 1:
            f[p:q] = True
        p += c
    return f.reshape(W, H).T.copy(), p == H * W


def plane_of(mask):
    """form 1: the column-major bit plane, bit p % 32 of word p / 32 -> uint32 array of ceil(H*W/32) words"""
    f = np.asarray(mask, dtype=bool).T.reshape(-1)
    b = np.packbits(f, bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)])
    return b.view("<u4").astype(np.uint32)


def column_words(mask):
    """the kernels' plane: word x*HW64 + j = rows 64j .. 64j+63 of column x -> list of ints"""
    H, W = mask.shape
    HW64 = (H + 63) // 64
    pad = np.zeros((HW64 * 64, W), dtype=bool)
    pad[:H] = mask
    b = np.packbits(pad.T.reshape(W * HW64, 64), axis=1, bitorder="little")
    return [int.from_bytes(r.tobytes(), "little") for r in b]


def mask_of_words(words, H, W):
    HW64 = (H + 63) // 64
    b = np.frombuffer(b"".join(int(w).to_bytes(8, "little") for w in words), dtype=np.uint8)
    return np.unpackbits(b, bitorder="little").reshape(W, HW64 * 64).T[:H].astype(bool)


def encoded(mask, slot_words):
    """what hgl_rle_encode_device writes for a mask: (table row, the slot words its form defines)"""
    H, W = mask.shape
    c = counts_of(mask)
    area = int(np.asarray(mask, dtype=bool).sum())
    if len(c) <= slot_words:
        return (len(c), 0, area, 0), c
    if (H * W + 31) // 32 <= slot_words:
        return (len(c), 1, area, 0), plane_of(mask)
    return (len(c), 2, area, 0), np.zeros(0, np.uint32)


def box_of(mask):
    """batched_mask_to_box (utils/amg.py:303-346): inclusive XYXY, zeros for an empty mask"""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def segments(mask, holes):
    """the column segments of one colour an H x W mask has (what seg_cap is compared with)"""
    w = np.asarray(mask, dtype=bool) != holes
    return int(w[0].sum() + (w[1:] & ~w[:-1]).sum())


# ---------------------------------------------------------------------------------------------------------- the rule
_components = {}


def components(work):
    """ccl_cases.flood_components, once per distinct mask"""
    key = (work.shape, np.packbits(work).tobytes())
    if key not in _components:
        _components[key] = CC.flood_components(work)
    return _components[key]


def remove(mask, thresh, mode):
    """ccl_cases.flood_remove_small_regions with the flood fill shared between thresholds (test_rle_clean_host.py holds the two
    against each other) -> (bool mask, changed)"""
    holes = mode == "holes"
    lab, sizes = components(mask != holes)
    small = [i + 1 for i, s in enumerate(sizes) if s < thresh]
    if not small:
        return mask, False
    if holes:
        return mask | np.isin(lab, small), True
    keep = [i + 1 for i, s in enumerate(sizes) if s >= thresh] or [sizes.index(max(sizes)) + 1]
    return np.isin(lab, keep), True


def clean(mask, thresh, mode="both", out_slot_words=None, seg_cap=None):
    """The contract for one decoded bool mask: dict(code, mask, row, words, box, result).  mode both: holes, then islands on the
    result.  seg_cap: code 3 when a pass that runs meets more segments of its colour."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    m, changed = mask, 0
    over = False
    if MODES[mode] & 1:
        over = seg_cap is not None and segments(m, True) > seg_cap
        m, c = remove(m, thresh, "holes")
        changed |= int(c)
    if MODES[mode] & 2 and not over:
        over = seg_cap is not None and segments(m, False) > seg_cap
        m, c = remove(m, thresh, "islands")
        changed |= int(c) << 1
    if over:
        return dict(code=3, mask=None, row=(0, 3, 0, 0), words=np.zeros(0, np.uint32), box=(0, 0, 0, 0), result=(3, 0, 0, 0))
    row, words = encoded(m, (H * W + 31) // 32 if out_slot_words is None else out_slot_words)
    return dict(code=0, mask=m, row=row, words=words, box=box_of(m), result=(0, int(m.sum()), changed, int(mask.sum())))


REFUSED = dict(mask=None, row=(0, 3, 0, 0), words=np.zeros(0, np.uint32), box=(0, 0, 0, 0))


# ---------------------------------------------------------------------------------------------------------- the cases
def bridges():
    """[(name, bool mask, threshold)]: the middle pixel of 0000110110000 is a border-touching hole of one pixel; filled, it makes
    ONE island of 5, which stays at threshold 3 -- a pass that drops islands from the unfilled mask keeps nothing but two pixels.
    As a row and as a column; and in 2-D, three rows of it: the hole is a bar of 3 from border to border (a hole that can join
    two islands always touches the border: an enclosed one is ringed by one island already), the islands have 6 pixels each and
    the threshold is 7 -- filled, one island of 15 stays; unfilled, both are small and only the first survives."""
    row = np.array([[c == "1" for c in "0000110110000"]])
    two = np.repeat(row, 3, axis=0)
    return [("bridge_row", row, 3), ("bridge_col", row.T.copy(), 3), ("bridge_2d", two, 7), ("bridge_2d_t", two.T.copy(), 7)]


_pairs = None


def pairs():
    """[(name, bool mask, threshold)]: every pattern and its transpose at every shape and threshold, then the bridges"""
    global _pairs
    if _pairs is None:
        out = []
        for H, W in SHAPES:
            for name, m in CC.cases(H, W):
                for tag, mm in (("", m != 0), ("_T", (m != 0).T.copy())):
                    for t in sorted(set(CC.thresholds(H, W))):
                        out.append((f"{H}x{W}_{name}{tag}_t{t}", mm, t))
        _pairs = out + bridges()
    return _pairs


_wants = {}


def wants(mode):
    """[clean(mask, t, mode)] over pairs(), computed once per mode"""
    if mode not in _wants:
        _wants[mode] = [clean(m, t, mode) for _, m, t in pairs()]
    return _wants[mode]


# ---------------------------------------------------------------------------------------------------------- the plan
ARRAYS = 5


def plan(images, S, slot_words, out_slot_words, area_thresh, modes, seg_cap):
    """rle_clean_plan in Python: None when the call is refused, else (cap, plane words)"""
    if not 1 <= len(images) <= 64:
        return None
    if not (0 <= slot_words < 2 ** 31 and 0 <= out_slot_words < 2 ** 31 and area_thresh >= 0 and 1 <= modes <= 3 and 1 <= seg_cap < 2 ** 31):
        return None
    p = NC.plan([list(r) for r in images], S)
    if p is None:
        return None
    most = 1
    for g, (H, W, e) in enumerate(images):
        n = (images[g + 1][2] if g + 1 < len(images) else S) - e
        if n > 0:
            most = max(most, W * ((H + 1) // 2))
    return min(seg_cap, most), p[0][2]


def workspace_bytes(images, S, slot_words, seg_cap):
    """hgl_rle_clean_workspace_bytes: run starts, status, planes, a rank per plane word, the segment arrays"""
    p = plan(images, S, slot_words, 0, 0, 3, seg_cap)
    if p is None or S <= 0:
        return 0
    cap, words = p
    up = lambda v: (v + 255) // 256 * 256
    return up(S * (slot_words + 1) * 4) + up(S * 16) + up(8 * words) + up(4 * words) + up(4 * ARRAYS * S * cap)


def packed(sizes, counts):
    images, e = [], 0
    for (H, W), n in zip(sizes, counts):
        images.append([H, W, e])
        e += n
    return images, e


def case(images, S, sw=8, osw=8, thresh=20, modes=3, cap=100):
    return dict(images=images, S=S, sw=sw, osw=osw, thresh=thresh, modes=modes, cap=cap)


def line_of(c):
    head = ["plan", len(c["images"]), c["S"], c["sw"], c["osw"], c["thresh"], c["modes"], c["cap"]]
    return " ".join(str(v) for v in head + [x for row in c["images"] for x in row])


def want_of(c):
    return plan(c["images"], c["S"], c["sw"], c["osw"], c["thresh"], c["modes"], c["cap"])


def mask_line(mask, thresh, mode, cap):
    H, W = mask.shape
    return " ".join(["mask", str(H), str(W), str(thresh), str(MODES[mode]), str(cap)] + [format(w, "x") for w in column_words(mask)])


SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (70, 37), (640, 640)]
N = [4, 33, 0, 65, 5, 129, 70, 512]


def refusals():
    """(why, case): one case per check of the contract"""
    images, S = packed(SIZES, N)

    def edit(g, col, value, S=S):
        im = [list(r) for r in images]
        im[g][col] = value
        return case(im, S)

    return [
        ("65 images", case([[4, 4, 0]] * 65, 0)),
        ("0 images", case([], 0)),
        ("-1 entries", case(images[:1], -1)),
        ("bad size", edit(1, 0, 0)),
        ("bad size", edit(1, 1, -3)),
        ("bad size", case([[1 << 16, 1 << 15, 0]], 1)),              # H*W = 2^31
        ("entries", edit(0, 2, 1)),                                  # does not start at 0
        ("entries", edit(3, 2, images[2][2] - 1)),                   # steps back
        ("entries", case(images, S - 513)),                          # the last image starts beyond S
        ("owns 4097 entries", case([[4, 4, 0]], 4097)),
        ("plane words", case([[64, 1 << 20, 0]], 4096)),             # the NMS's own limit
        ("slot_words -1", case(images, S, sw=-1)),
        ("slot_words 2147483648", case(images, S, sw=1 << 31)),
        ("out_slot_words -1", case(images, S, osw=-1)),
        ("out_slot_words 2147483648", case(images, S, osw=1 << 31)),
        ("area_thresh -1", case(images, S, thresh=-1)),
        ("modes 0", case(images, S, modes=0)),
        ("modes 4", case(images, S, modes=4)),
        ("seg_cap 0", case(images, S, cap=0)),
        ("seg_cap 2147483648", case(images, S, cap=1 << 31)),
    ]
