"""Planes, masks, heat-maps, launch routes, reference and checker for the coherence pooling (csrc/scoring.hip: pool_block under
masked_pool_kernel, grp_masked_pool_kernel and grp_masked_pool_last_kernel, the min / max of minmax_kernel and ref_minmax_body,
the final reductions coherence_final_kernel and ref_coherence_body), plain numpy, no GPU code.

The operation is Hybridgl_main.py:203-223: min-max normalisation of the heat-map, the direction ramp of gen_dir_mask
(utils.py:135-161), the division by the mean, and per mask the blend
    score = (2 - black) * mean over the mask's pixels  -  black * mean over the other pixels.

`reference` is the yardstick.  Min, max, (a - min) / (max - min), the ramp and the division by the mean are float32 operations:
they are part of the operation's definition (the ramp is oracle.clip_oracle.gen_dir_mask, held bit for bit against
torch.linspace by tests/golden/scoring.npz).  The mean itself is the float64 mean of the float32 values rounded once to float32,
and both side means are float64 sums over the side's OWN pixels: no total, no subtraction.  `black` is the float32 the C ABI
carries, so 2 - black is exact (Sterbenz: 1 <= black <= 4).

`routes` restates the host's launch decisions (hgl_coherence_scores, tail_launch / tail_launch_pool) with the constants read
from scoring.hip, so a retune moves the expectations of tests/test_coherence_cases_host.py instead of silently moving the cases
to other paths.

`check` -- the tolerance.  NaN positions must be equal (empty mask, full mask, flat heat-map, a ramp that is zero on the whole
plane: the NaN goldens demand the same).  Elsewhere, with u = 2^-24 and in_n = (2 - black) mean_in, out_n = black mean_out,
    |got - ref| <= C u (|in_n| + |out_n|),   C = 64.
C counts the roundings of an implementation that sums each side DIRECTLY in float32 trees, as the reference program's
torch.sum does.  Every term of every sum is >= 0 (normalised value times a ramp in [0, 1]), so a rounding of a partial sum is
at most u times the final sum and relative errors add.  Per side, relative to that side's term:
    4   per pixel value: the reference's own rounding of a / mean, and an implementation's a / mean (its mean has other bits,
        so the two roundings are independent), * (2 - black) or * black, / count (Hybridgl_main.py:221 does all three per pixel;
        the device code does none of them per pixel)
   27   the mean: 22 for a 1024-term float32 tree (16 terms in sequence in a lane -- 15 roundings, the first add is exact --
        then 6 levels over 64 lanes, counted as 22), 4 for the levels that join the at most sixteen such trees of the planes
        below (<= 16384 pixels) when they too are joined in float32, 1 for the reference's rounding of its mean
   26   the side's sum: the same 22 + 4
    1   the blend: the result rounded to float32 (|score| <= |in_n| + |out_n|)
   58 in all; the six left to 64 cover the second-order terms ((1 + u)^58) and an implementation that keeps the count in float32.
C is a bound for the operation: it is not fitted to the device code and has no term in HW / (HW - c).  An implementation that
takes the outside sum as total - inside from float32 partials does not meet it on masks that leave few pixels outside:
`planted` below holds such an implementation and tests/test_coherence_cases_host.py shows it rejected.

tests/test_coherence_cases_host.py checks this module on the CPU, tests/test_gpu_coherence_paths.py runs the device code.
"""
import os
import re
from collections import namedtuple

import numpy as np

from oracle.clip_oracle import gen_dir_mask

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORING_HIP = os.path.join(ROOT, "hybridgl_amd", "csrc", "scoring.hip")

C_BOUND = 64
U = 2.0 ** -24
DIRFLAGS = ("none", "left", "right", "middle")
BLACKS = (1.8, 1.95, 1.5)           # relaflag none / "big" / "small" (Hybridgl_main.py:212-217)
ENTRIES = ("coherence_scores", "score_ref", "score_group")


# ------------------------------------------------------------------------------------------------------------- the constants
def constants(path=SCORING_HIP):
    """PX_LANE, PIX_PER_BLOCK, MASK_GROUP, REF_MASK_GROUP, REF_MAXS, REF_MM_BLOCKS as csrc/scoring.hip declares them (a
    declaration may be a product or sum of integers and of constants declared above it)"""
    src = open(path).read()
    out = {}
    for name in ("PX_LANE", "PIX_PER_BLOCK", "MASK_GROUP", "REF_MASK_GROUP", "REF_MAXS", "REF_MM_BLOCKS"):
        m = re.findall(r"^constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", src, flags=re.M)
        if len(m) != 1:
            raise ValueError(f"{path}: {len(m)} declarations of {name}")
        expr = m[0].strip()
        if not re.fullmatch(r"[\w\s*+()]+", expr):
            raise ValueError(f"{path}: cannot read {name} = {expr}")
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


CONST = constants()
PX_LANE, PIX_PER_BLOCK = CONST["PX_LANE"], CONST["PIX_PER_BLOCK"]
WAVE_PIX = 64 * PX_LANE             # pixels of one wave partial


# ------------------------------------------------------------------------------------------------------------------ the routes
def routes(H, W, N, S, entry, call_S=None):
    """The launches one call of `entry` makes for a plane of H x W, N masks and a ref of S sentences (S is 1 for
    coherence_scores).  call_S: the sentence counts of ALL refs of a score_group call of at most sixteen rows (default: this ref
    alone) -- the maps per pass, CH, are chosen per launch from the longest row.
      launches   subset of {"full", "partial"}: the FULL instantiation over HW // PIX_PER_BLOCK blocks, the !FULL one over the rest
      NS         the pool_block<NS, true> instantiations the full launch runs for this ref (empty without a full launch);
                 the partial launch always runs pool_block<1, false>
      MG, CH     masks per pooling workgroup; maps per pass (None for coherence_scores: one map, no passes)
      groups     mask groups = blockIdx.y extent that does work
      rows       sentences per row of the descriptor table"""
    if entry not in ENTRIES:
        raise ValueError(entry)
    HW = H * W
    launches = set()
    if HW // PIX_PER_BLOCK > 0:
        launches.add("full")
    if HW % PIX_PER_BLOCK:
        launches.add("partial")
    if entry == "coherence_scores":
        MG, CH, rows = CONST["MASK_GROUP"], None, [1]
        NS = {1} if "full" in launches else set()
    else:
        MG = CONST["MASK_GROUP"] if entry == "score_ref" else CONST["REF_MASK_GROUP"]
        maxs = CONST["REF_MAXS"]
        every = [S] if call_S is None or entry == "score_ref" else list(call_S)
        CH = 3 if min(max(every), maxs) <= 3 else 4
        rows = [min(maxs, S - s0) for s0 in range(0, S, maxs)]
        NS = set()
        if "full" in launches:
            for sr in rows:
                NS |= {min(CH, sr - s0) for s0 in range(0, sr, CH)}
    return dict(launches=launches, NS=NS, MG=MG, CH=CH, groups=-(-N // MG), rows=rows)


# ------------------------------------------------------------------------------------------------------------------- the cases
# mask kinds; "hole" = all pixels but ...
KINDS = ("empty", "full", "hole_max", "hole_min", "first_px", "last_px", "hole_two", "hole_last_row", "full_blocks", "partial_block",
         "one_wave", "one_lane", "checker", "blob", "blob_02", "blob_7f", "blob_80", "blob_ff")
EXTRA = ("hole_first", "hole_last", "blob", "checker", "one_wave", "one_lane", "blob_80", "hole_two")   # second helpings for N > 18
HEATS = ("smooth", "signed", "peaked", "ends", "negzero", "constant")

Case = namedtuple("Case", "H W N note")
CASES = [
    Case(3, 7, 8, "partial block only, W < 16; N fills one group of 8"),
    Case(40, 50, 9, "partial block only"),
    Case(64, 64, 9, "exactly one full block"),
    Case(128, 128, 9, "four full blocks, no partial"),
    Case(64, 65, 40, "one full block + 64 px, odd W, unaligned planes; five groups of 8, two of 32"),
    Case(97, 131, 33, "three full blocks + partial; 32 | 33"),
    Case(1, 4097, 9, "one block + 1 px, W larger than a block"),
    Case(4097, 1, 9, "W = 1: wrap at every pixel; `middle` has an empty first ramp"),
    Case(33, 2, 9, "`middle` with two one-step ramps"),
    Case(5, 15, 9, "`middle` at odd W below a lane's 16 pixels"),
]


def case_id(c):
    return f"{c.H}x{c.W}-N{c.N}"


def _seed(c, salt):
    return (c.H * 100003 + c.W * 1009 + salt) % (2 ** 31)


def extremes(c):
    """(pmax, pmin): flat indices where every heat-map of the case but "ends" and "constant" has its maximum / minimum:
    neither the first nor the last pixel, not the same pixel"""
    HW = c.H * c.W
    rng = np.random.default_rng(_seed(c, 1))
    pmax = int(rng.integers(1, HW - 1))
    pmin = pmax
    while pmin == pmax:
        pmin = int(rng.integers(1, HW - 1))
    return pmax, pmin


def mask_kinds(c):
    """the N kinds of the case's masks: empty, full and the two single-pixel holes everywhere, the other kinds in rotation over
    the cases with N = 9, all of them (and second helpings) where N >= 18"""
    if c.N >= len(KINDS):
        more = [EXTRA[i % len(EXTRA)] for i in range(c.N - len(KINDS))]
        return list(KINDS) + more
    k = CASES.index(c)
    rest = KINDS[4:]
    return list(KINDS[:4]) + [rest[(5 * k + i) % len(rest)] for i in range(c.N - 4)]


def masks_for(c):
    """uint8 [N, H, W]; true bytes are 1 but for the blob_XX kinds"""
    H, W, HW = c.H, c.W, c.H * c.W
    pmax, pmin = extremes(c)
    nfull = HW // PIX_PER_BLOCK * PIX_PER_BLOCK
    rng = np.random.default_rng(_seed(c, 2))
    out = np.zeros((c.N, HW), dtype=np.uint8)
    for n, kind in enumerate(mask_kinds(c)):
        m = out[n]
        if kind == "full":
            m[:] = 1
        elif kind == "hole_max":
            m[:] = 1; m[pmax] = 0
        elif kind == "hole_min":
            m[:] = 1; m[pmin] = 0
        elif kind == "hole_first":
            m[1:] = 1
        elif kind == "hole_last":
            m[:-1] = 1
        elif kind == "first_px":
            m[0] = 1
        elif kind == "last_px":
            m[-1] = 1
        elif kind == "hole_two":
            m[:] = 1; m[rng.choice(HW, 2, replace=False)] = 0
        elif kind == "hole_last_row":
            m[:HW - W] = 1
        elif kind == "full_blocks":
            m[:nfull] = 1
        elif kind == "partial_block":
            m[nfull:] = 1
        elif kind == "one_wave":      # a wave's pixels: the second wave of the plane where there is one
            w0 = WAVE_PIX if HW >= 2 * WAVE_PIX else 0
            m[w0:w0 + WAVE_PIX] = 1
        elif kind == "one_lane":
            l0 = int(rng.integers(0, max(1, HW // PX_LANE))) * PX_LANE
            m[l0:l0 + PX_LANE] = 1
        elif kind == "checker":
            yy, xx = np.mgrid[0:H, 0:W]
            m[:] = ((yy + xx + n) & 1).reshape(-1)
        elif kind.startswith("blob"):
            byte = int(kind[5:], 16) if len(kind) > 4 else 1
            if min(H, W) >= 8:        # an ellipse of 20 % .. 60 % of the plane
                yy, xx = np.mgrid[0:H, 0:W]
                area = rng.uniform(0.2, 0.6) * HW
                a = min(np.sqrt(area / np.pi * rng.uniform(0.7, 1.4)), W / 2)
                b = min(area / (np.pi * a), H / 2)
                cy, cx = rng.uniform(b, H - b), rng.uniform(a, W - a)
                inside = (((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0).reshape(-1)
            else:                     # a run of the flat plane: it crosses lanes, waves and blocks
                n0 = int(rng.integers(0, HW // 2))
                inside = np.zeros(HW, dtype=bool)
                inside[n0:n0 + int(rng.integers(HW // 5 + 1, HW // 2 + 1))] = True
            m[inside] = byte
        elif kind != "empty":
            raise ValueError(kind)
    return out.reshape(c.N, H, W)


def heat_for(c, kind):
    """float32 [H, W]"""
    H, W, HW = c.H, c.W, c.H * c.W
    pmax, pmin = extremes(c)
    rng = np.random.default_rng(_seed(c, 3 + HEATS.index(kind)))
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    f = np.zeros((H, W))
    for _ in range(4):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        s = rng.uniform(0.1, 0.4) * max(H, W)
        f += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    f = (f + rng.uniform(0.01, 0.06, size=f.shape)).reshape(-1)
    if kind == "constant":
        return np.full((H, W), 0.37, dtype=F32)
    if kind == "ends":            # maximum at pixel 0, minimum at the last pixel
        f[0], f[-1] = f.max() * 1.25, f.min() * 0.5
        return f.reshape(H, W).astype(F32)
    if kind == "peaked":          # one pixel at 1, the others near 1e-3
        f = 1e-3 * (1.0 + 0.1 * rng.uniform(size=HW))
        f[pmax], f[pmin] = 1.0, 0.9e-3
        return f.reshape(H, W).astype(F32)
    f[pmax], f[pmin] = f.max() * 1.25, f.min() * 0.5
    if kind == "signed":          # min < 0 < max
        f -= 0.5 * (f.max() + f.min())
    if kind == "negzero":         # minimum -0.0 (also elsewhere, and +0.0 beside it)
        f -= f[pmin]
        z = rng.choice(HW, max(2, HW // 16), replace=False)
        f[z[::2]], f[z[1::2]] = -0.0, 0.0
        f[pmin] = -0.0
        f[pmax] = max(f[pmax], 1.0)
    return f.reshape(H, W).astype(F32)


def sentences_for(c):
    """the 24 (heat kind, dirflag, black) of the case: every heat-map under every dirflag, black in rotation"""
    return [(h, d, BLACKS[(i + j) % 3]) for i, h in enumerate(HEATS) for j, d in enumerate(DIRFLAGS)]


# --------------------------------------------------------------------------------------------------------------- the reference
def normalised(attn, dirflag):
    """(a - min) / (max - min) * ramp in float32: the operation's definition up to the division by the mean"""
    a = np.asarray(attn, dtype=F32)
    with np.errstate(all="ignore"):
        a = (a - a.min()) / (a.max() - a.min())
        return (a * gen_dir_mask(dirflag, a.shape[0], a.shape[1])).astype(F32)


def reference(attn, masks, dirflag, black):
    """(score, in_n, out_n), float64 [N] each: in_n = (2 - black) mean_in, out_n = black mean_out, score = in_n - out_n"""
    with np.errstate(all="ignore"):
        v = normalised(attn, dirflag)
        mean = F32(v.astype(F64).sum() / v.size)
        a = (v / mean).astype(F32).astype(F64).reshape(-1)
        b = F32(black)
        two, bl = F64(F32(2) - b), F64(b)
        N = len(masks)
        in_n, out_n = np.empty(N), np.empty(N)
        for n, m in enumerate(masks):
            inside = (np.asarray(m).reshape(-1) != 0)
            c = int(inside.sum())
            in_n[n] = two * (a[inside].sum() / c) if c else np.nan
            out_n[n] = bl * (a[~inside].sum() / (a.size - c)) if c < a.size else np.nan
        return in_n - out_n, in_n, out_n


# ----------------------------------------------------------------------------------------------------------------- the checker
def ratios(got, ref):
    """|got - ref| / (C u (|in_n| + |out_n|)) per mask; 0 where both are NaN, inf where one is"""
    score, in_n, out_n = ref
    got = np.asarray(got, dtype=F64)
    assert got.shape == score.shape
    gn, rn = np.isnan(got), np.isnan(score)
    with np.errstate(all="ignore"):
        err = np.abs(got - score)
        bound = C_BOUND * U * (np.abs(in_n) + np.abs(out_n))
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(gn & rn, 0.0, r)
    return np.where(gn != rn, np.inf, r)


def check(got, ref, what=""):
    """asserts the bound of the module's docstring; returns the worst ratio to it"""
    r = ratios(got, ref)
    bad = np.flatnonzero(~(r <= 1.0))
    assert bad.size == 0, (f"{what}: masks {bad.tolist()} miss the bound: ratio {r[bad].tolist()}, got "
                           f"{np.asarray(got, dtype=F64)[bad].tolist()}, reference {ref[0][bad].tolist()}")
    return float(r.max())


# --------------------------------------------------------------------------------------------- a float32 implementation, planted
def _tree32(x):
    """float32 sum of a 1-D array as the device sums a wave's 1024 products: 16 in sequence per lane, a pairwise tree over 64
    lanes; the waves' sums are added in float64"""
    n = -(-x.size // WAVE_PIX) * WAVE_PIX
    p = np.zeros(n, dtype=F32)
    p[:x.size] = x
    p = p.reshape(-1, 64, PX_LANE)
    acc = np.zeros(p.shape[:2], dtype=F32)
    for e in range(PX_LANE):
        acc = (acc + p[:, :, e]).astype(F32)
    while acc.shape[1] > 1:
        acc = (acc[:, 0::2] + acc[:, 1::2]).astype(F32)
    return acc[:, 0].astype(F64)          # one partial per wave


DEFECTS = ("wave_dropped", "count_off_by_one", "ramp_shifted", "byte_80_false", "padded_mean", "tot_minus_s_f32")


def planted(attn, masks, dirflag, black, defect=None):
    """score [N] float32 of a float32-tree implementation with both sides summed directly -- and, per `defect`, one of the
    errors a pooling kernel can make"""
    with np.errstate(all="ignore"):
        a = np.asarray(attn, dtype=F32)
        H, W = a.shape
        ramp = gen_dir_mask(dirflag, H, W)
        if defect == "ramp_shifted":
            ramp = np.roll(ramp, 1, axis=1)
        v = (((a - a.min()) / (a.max() - a.min())) * ramp).astype(F32).reshape(-1)
        HW = v.size
        tot_w = _tree32(v)
        tot = tot_w.sum()
        mean = tot / (-(-HW // PIX_PER_BLOCK) * PIX_PER_BLOCK if defect == "padded_mean" else HW)
        b = F32(black)
        out = np.empty(len(masks), dtype=F32)
        for n, m in enumerate(masks):
            mb = np.asarray(m).reshape(-1)
            inside = (mb & 0x7f) != 0 if defect == "byte_80_false" else mb != 0
            c = int(inside.sum())
            s_w = _tree32(np.where(inside, v, F32(0)))
            if defect == "wave_dropped":
                s_w[-1] = 0.0
            s = s_w.sum()
            if defect == "tot_minus_s_f32":
                o = F64(F32(tot) - F32(s))
            else:
                o = _tree32(np.where(inside, F32(0), v)).sum()
            if defect == "count_off_by_one":
                c += 1
            if c == HW:
                o = tot - s          # 0 / 0 for the full mask
            out[n] = F32(F64(F32(2) - b) * (s / mean) / c - F64(b) * (o / mean) / (HW - c))
        return out
