"""What the tests of hgl_rle_merge_device share: the golden file's cases, the run lengths of a dense mask in numpy, the vote in
numpy, and rle_merge_plan (csrc/rle_group.h) with the workspace arithmetic of csrc/rle.hip restated in Python."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rle_merge_fuzz.npz")


def golden_cases():
    """[(H, W, masks [n,H,W] uint8, union counts, intersection counts)] in the order the generator wrote them"""
    z = np.load(GOLDEN)
    V = int(z["variants"])
    out, at, i = [], {"union": 0, "inter": 0}, 0
    for k, (H, W) in enumerate(z["shapes"].tolist()):
        for n in z["members"].tolist():
            sets = np.unpackbits(z[f"m{k}_{n}"])[:V * n * H * W].reshape(V, n, H, W)
            for v in range(V):
                got = {}
                for name in ("union", "inter"):
                    m = int(z[name + "_len"][i])
                    got[name] = z[name][at[name]:at[name] + m].astype(np.int64)
                    at[name] += m
                out.append((H, W, sets[v], got["union"], got["inter"]))
                i += 1
    assert at["union"] == len(z["union"]) and at["inter"] == len(z["inter"])
    return out


def counts_of(mask):
    """column-major run lengths of a dense [H,W] mask, zeros first (maskApi.c rleEncode)"""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.flatnonzero(flat != np.concatenate([[False], flat[:-1]]))      # a pixel that differs from its predecessor (0 before p = 0)
    return np.diff(np.concatenate([[0], edges, [flat.size]])).astype(np.int64)


def vote(masks, members, lo, hi):
    """the dense rule: pixels whose count over members (indices into masks, repeats count) lies in [lo, hi]"""
    H, W = masks.shape[1:]
    count = np.zeros((H, W), np.int64)
    for m in members:
        count += masks[m] != 0
    return ((count >= lo) & (count <= hi)).astype(np.uint8)


def plan(images, Ssrc, S, M):
    """rle_merge_plan in Python: None when the geometry is refused, else ((blocks_src, words_src, words_out), rows)"""
    G = len(images)
    if not 1 <= G <= 64:
        return None
    if Ssrc < 0 or S < 0 or M < 0:
        return None
    blocks = words_src = words_out = 0
    rows = []
    for g, (H, W, es, eo) in enumerate(images):
        es_next = images[g + 1][2] if g + 1 < G else Ssrc
        eo_next = images[g + 1][3] if g + 1 < G else S
        if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31 and H * W < 2 ** 31):
            return None
        if not (0 <= es <= es_next <= Ssrc and (g > 0 or es == 0)):
            return None
        if not (0 <= eo <= eo_next <= S and (g > 0 or eo == 0)):
            return None
        Q = W * ((H + 63) // 64)
        rows.append((H, W, es, eo, words_src, words_out, blocks))
        words_src += (es_next - es) * Q
        words_out += (eo_next - eo) * Q
        blocks += (es_next - es) * ((Q + 255) // 256)
        if words_src >= 2 ** 32 or words_out >= 2 ** 32 or blocks >= 2 ** 31:
            return None
    return (blocks, words_src, words_out), rows


def workspace_bytes(images, Ssrc, slot_words_src, S, M):
    """hgl_rle_merge_workspace_bytes in Python: run starts, status and planes of the source set, the merged planes"""
    p = plan(images, Ssrc, S, M)
    if p is None or S == 0 or slot_words_src < 0:
        return 0
    up = lambda n: (n + 255) // 256 * 256
    (_, words_src, words_out), _ = p
    return up(Ssrc * (slot_words_src + 1) * 4) + up(Ssrc * 16) + up(words_src * 8) + up(words_out * 8)
