"""What the compaction of an encoded set (hgl_rle_select_device) is judged on, plain numpy, no GPU code: the contract's
statement -- the stable per-image compaction, max_keep, the placeholder, the "words not written" rule -- over host arrays, who
survives an NMS result, and rle_select_plan (csrc/rle_group.h) restated in Python."""
import numpy as np

import rle_nms_cases as NC

COLS_MAX, WAVES, CHUNK = 8, 4, 2048


def defined_words(row, H, W, slot_words):
    """the slot words the table row (n_counts, form, ., .) defines for an H x W entry, or None when it describes no mask (the
    decoder's code 2)"""
    n, form = int(row[0]), int(row[1])
    plane = (H * W + 31) // 32
    if n < 0:
        return None
    if form == 0:
        return n if n <= slot_words else None
    if form == 1:
        return plane if plane <= slot_words else None
    return None


def kept_from_nms(result):
    """the keep flags an NMS result [S,4] = (code, area, rank, by) stands for: code 0 or 1 and by == -1"""
    result = np.asarray(result)
    return ((result[:, 0] == 0) | (result[:, 0] == 1)) & (result[:, 3] == -1)


def select(slots, table, images, keep, cols, out_slots, out_table, out_cols, out_src, out_n):
    """The contract on host arrays.  slots [S,sw] uint32, table [S,4] int32, images: rows (H, W, first entry, max_keep), keep [S]
    (nonzero = kept), cols [C,S] of 4-byte words; the out_* arrays hold what the destination held before the call and are
    returned as the call leaves them (copies): so a word the call does not write keeps its value."""
    slots, table, keep = np.asarray(slots), np.asarray(table), np.asarray(keep) != 0
    S, sw = slots.shape
    out_slots, out_table, out_cols, out_src, out_n = (np.array(a, copy=True) for a in (out_slots, out_table, out_cols, out_src, out_n))
    if S == 0:
        return out_slots, out_table, out_cols, out_src, out_n      # nothing is launched: out_n is the caller's
    for g, (H, W, e, mk) in enumerate(images):
        e_next = images[g + 1][2] if g + 1 < len(images) else S
        n = e_next - e
        alive = np.flatnonzero(keep[e:e_next])      # stored order
        if mk >= 0:
            alive = alive[:mk]
        k = len(alive)
        out_n[g] = k
        out_src[e:e + k] = alive
        out_src[e + k:e_next] = -1
        out_table[e:e + k] = table[e + alive]
        out_cols[:, e:e + k] = cols[:, e + alive]
        for p, i in enumerate(alive):
            w = defined_words(table[e + i], H, W, sw)
            if w:
                out_slots[e + p, :w] = slots[e + i, :w]
        out_table[e + k:e_next] = (1, 0, 0, 0)
        out_slots[e + k:e_next, 0] = H * W
        out_cols[:, e + k:e_next] = 0
    return out_slots, out_table, out_cols, out_src, out_n


def plan(images, S, slot_words, C, has_keep, has_nms, slots=0, out_slots=1 << 40, table=1 << 41, out_table=1 << 42):
    """rle_select_plan in Python: None when the call is refused, else ((chunks, blocks, wide), rows (H, W, first, max_keep as
    the kernels take it)); the four addresses as numbers"""
    G = len(images)
    if not 1 <= G <= 64 or not 0 <= slot_words < 2 ** 31 or not 0 <= C <= COLS_MAX or bool(has_keep) == bool(has_nms):
        return None
    if NC.plan([list(r[:3]) for r in images], S) is None:
        return None
    if S > 0 and slot_words < 1:
        return None
    sb, tb = S * slot_words * 4, S * 16
    if sb and not (slots + sb <= out_slots or out_slots + sb <= slots):
        return None
    if tb and not (table + tb <= out_table or out_table + tb <= table):
        return None
    chunks = (slot_words + CHUNK - 1) // CHUNK if slot_words else 1
    blocks = (S + WAVES - 1) // WAVES * chunks
    if blocks >= 2 ** 31:
        return None
    rows = []
    for g, (H, W, e, mk) in enumerate(images):
        n = (images[g + 1][2] if g + 1 < G else S) - e
        rows.append((H, W, e, n if mk < 0 or mk > n else mk))
    return (chunks, blocks, int(slot_words % 4 == 0 and (slots | out_slots) % 16 == 0)), rows


# ---- cases of the plan, shared by the sanitizer harness's test and the ABI test
A = dict(slots=1 << 30, out_slots=1 << 40, table=1 << 41, out_table=1 << 42)      # four buffers far apart, 16-byte aligned


def packed(sizes, counts, limits):
    images, e = [], 0
    for (H, W), n, mk in zip(sizes, counts, limits):
        images.append([H, W, e, mk])
        e += n
    return images, e


def case(images, S, sw=8, C=2, has_keep=1, has_nms=0, **addr):
    return dict(images=images, S=S, sw=sw, C=C, has_keep=has_keep, has_nms=has_nms, **dict(A, **addr))


def line_of(c):
    head = [len(c["images"]), c["S"], c["sw"], c["C"], c["has_keep"], c["has_nms"], c["slots"], c["out_slots"], c["table"], c["out_table"]]
    return " ".join(str(v) for v in head + [x for row in c["images"] for x in row])


def want_of(c):
    return plan(c["images"], c["S"], c["sw"], c["C"], c["has_keep"], c["has_nms"], c["slots"], c["out_slots"], c["table"], c["out_table"])


SIZES = [(1, 1), (64, 64), (65, 63), (63, 260), (130, 4), (3, 5), (70, 37), (640, 640)]
N = [4, 33, 0, 65, 5, 129, 70, 512]
LIMITS = [-1, 0, 5, 65, 66, 1, -7, 511]


def refusals():
    """(why, case): one case per check of the contract"""
    images, S = packed(SIZES, N, LIMITS)

    def edit(g, col, value, S=S):
        im = [list(r) for r in images]
        im[g][col] = value
        return case(im, S)

    return [
        ("65 images", case([[4, 4, 0, -1]] * 65, 0)),
        ("0 images", case([], 0)),
        ("-1 entries", case(images[:1], -1)),
        ("bad size", edit(1, 0, 0)),
        ("bad size", edit(1, 1, -3)),
        ("bad size", case([[1 << 16, 1 << 15, 0, -1]], 1)),          # H*W = 2^31
        ("entries", edit(0, 2, 1)),                                  # does not start at 0
        ("entries", edit(3, 2, images[2][2] - 1)),                   # steps back
        ("entries", case(images, S - 513)),                          # the last image starts beyond S
        ("owns 4097 entries", case([[4, 4, 0, 3]], 4097)),
        ("plane words", case([[64, 1 << 20, 0, -1]], 4096)),         # the NMS's own limit
        ("slot_words -1", case(images, S, sw=-1)),
        ("slot_words 2147483648", case(images, S, sw=1 << 31)),
        ("slot_words 0", case(images, S, sw=0)),                     # a placeholder needs one word
        ("-1 side columns", case(images, S, C=-1)),
        ("9 side columns", case(images, S, C=9)),
        ("both given", case(images, S, has_keep=1, has_nms=1)),
        ("neither given", case(images, S, has_keep=0, has_nms=0)),
        ("out_slots overlaps slots", case(images, S, out_slots=A["slots"])),
        ("out_slots overlaps slots", case(images, S, out_slots=A["slots"] + S * 8 * 4 - 4)),      # the last word
        ("out_slots overlaps slots", case(images, S, out_slots=A["slots"] - S * 8 * 4 + 4)),      # the first
        ("out_table overlaps table", case(images, S, out_table=A["table"] + 16 * S - 16)),
        ("out_table overlaps table", case(images, S, out_table=A["table"] - 16)),
        ("for one launch", case([[2, 2, 4096 * g, -1] for g in range(64)], 64 * 4096, sw=(1 << 31) - 1, out_slots=1 << 60)),
    ]
