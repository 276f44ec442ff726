"""Cases, inputs, float64 reference and checkers for the rel-pos producers of the SAM image encoder (csrc/sam_api.hip:
enc_relpos_tables behind hgl_sam_relpos_tables; csrc/sam_glue.hip: relpos_direct_kernel, relpos_mfma_kernel, relpos_gather_kernel),
plain numpy, no GPU code.

The operation is the pair of einsums of add_decomposed_rel_pos (modeling/image_encoder.py:325-361) on the UNSCALED q of B
windows (or whole grids) of S = size x size tokens:

    rel_h[bh, q, k] = q_vec . Rh[q // size - k + size - 1]          bh = b * heads + h
    rel_w[bh, q, k] = q_vec . Rw[q %  size - k + size - 1]          q_vec = the hd columns of head h in row b * S + q

`reference` evaluates that in float64 (for q given as fp16 planes: of hi + lo).  tests/test_relpos_cases_host.py holds it against
oracle/sam_oracle.py (get_rel_pos + the einsums of encoder_attention) without a GPU; tests/test_gpu_relpos_tables.py runs the
device code on CASES.

Two kinds of input.

Index probes (`probe_inputs`), asserted EXACTLY: q is one-hot per query -- query q of item bh has its 1.0 at channel
(7 * q + bh) % hd -- and the tables are Rh[r, c] = r + c / 128, Rw[r, c] = 256 + r + c / 128 (the offset tells the two tables
apart; r <= 130 and c <= 79, so every entry has at most 9 + 7 bits: exact in fp32 and exact as an fp16 hi + lo pair).  Every
output is then ONE table entry, 1.0 * x plus zeros, on every kernel, the matrix-core ones included, and a wrong (bh, q, k)
index, head, axis or table row shows as a different value.  `probe_mismatches` names the entries that differ.

Random data (`random_inputs`): q ~ N(0, 1) with token rows 0..3 of every item scaled by 30 and rows 4..7 by 0.01, R ~ N(0, 0.1),
judged per entry against a bound derived from the arithmetic, with A = sum_c |q_c| |R_c| in float64 (`bound`):

  "f32"  the VALU kernel (a sequential fp32 dot product with fused multiply-adds) and the fp32 matrix-core GEMM of the generic
         path (exact products, fp32 accumulation in some order): hd roundings of at most 2^-24 of the running sum, which never
         exceeds A:  hd * 2^-24 * A.
  "x3"   the split-fp16 matrix-core kernels: hi + lo represents a value to 2^-22, two operands and the dropped lo * lo product
         give about 2^-20 of each term, the accumulation is fp32 as above, and the absolute term covers the fp16 subnormal
         spacing of lo:  (2^-20 + hd * 2^-24) * A + 1e-7.

The bounds come from the arithmetic, not from a run.
"""
import re
from collections import namedtuple

import numpy as np

F32 = np.float32
B, HEADS = 2, 3                 # a batch index and a head count that is no power of two: b / h mix-ups show
SENTINEL = -7777.25             # fill of the output buffers and their guard zones (no table entry, no plausible dot product)
GUARD = 4096                    # floats in front of, between and behind the two outputs

# precision: the library mode; q: "fp32" rows or fp16 "planes"; kernels: what the call must launch, in order (kernel_id);
# bound: the error bound of the kernel that computes the products
Case = namedtuple("Case", "precision q hd size kernels bound note")

GEMM = "gemm_f32_kernel"        # the fp32 matrix-core tile kernel (its template arguments are tuning, not route: compared by name)
GENERIC = (GEMM, GEMM, "relpos_gather_kernel", "relpos_gather_kernel")


def _cases():
    out = []
    for hd in (64, 80):
        for size in (2, 14, 28, 64):
            out.append(Case("f32", "fp32", hd, size, (f"relpos_direct_kernel<{hd}>",), "f32", "VALU kernel, fp32 mode"))
    for hd in (64, 80):
        out.append(Case("f16x3", "fp32", hd, 14, (f"relpos_mfma_kernel<{hd},1,0>",), "x3", "S = 196: a 68-query tail block"))
        out.append(Case("f16x3", "fp32", hd, 64, (f"relpos_mfma_kernel<{hd},4,0>",), "x3", "row-store path"))
    for size in (8, 28):
        out.append(Case("f16x3", "fp32", 64, size, ("relpos_direct_kernel<64>",), "f32", "VALU kernel under the split layout"))
    for hd in (64, 80):
        out.append(Case("f16x3", "planes", hd, 14, (f"relpos_mfma_kernel<{hd},1,1>",), "x3", "q as planes, windows"))
        out.append(Case("f16x3", "planes", hd, 64, (f"relpos_mfma_kernel<{hd},4,1>",), "x3", "q as planes, four query blocks per workgroup"))
    for prec in ("f32", "f16x3"):
        for hd in (16, 32):
            for size in (14, 16):
                out.append(Case(prec, "fp32", hd, size, GENERIC, "f32", "generic producer: head dim without a direct kernel"))
        for size in (7, 13, 66):
            out.append(Case(prec, "fp32", 64, size, GENERIC, "f32", "generic producer: size the direct kernels refuse"))
    # the opt-in fp16 mode keeps the split layout: the fp32-q launches above are reachable in it, with the same kernels
    out.append(Case("f16", "fp32", 64, 14, ("relpos_mfma_kernel<64,1,0>",), "x3", "fp16 mode: the three-term kernel all the same"))
    out.append(Case("f16", "fp32", 80, 64, ("relpos_mfma_kernel<80,4,0>",), "x3", "fp16 mode, row-store path"))
    out.append(Case("f16", "fp32", 64, 8, ("relpos_direct_kernel<64>",), "f32", "fp16 mode, VALU kernel"))
    out.append(Case("f16", "fp32", 32, 14, GENERIC, "f32", "fp16 mode, generic producer"))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.precision}-{c.q}-hd{c.hd}-s{c.size}"


def ldq(hd, heads=HEADS):
    """the packed q | k | v row of the encoder: q in the first third"""
    return 3 * heads * hd


# ------------------------------------------------------------------------------------------------------------------ inputs
def probe_inputs(hd, size, nb=B, heads=HEADS):
    """-> q [nb * S, ldq] fp32, Rh, Rw [2 * size - 1, hd] fp32 (module docstring); the k | v columns hold 3.0"""
    S, L = size * size, 2 * size - 1
    q = np.zeros((nb * S, ldq(hd, heads)), dtype=F32)
    q[:, heads * hd:] = 3.0
    tok = np.arange(S)
    for b in range(nb):
        for h in range(heads):
            q[b * S + tok, h * hd + (7 * tok + b * heads + h) % hd] = 1.0
    Rh = (np.arange(L, dtype=np.float64)[:, None] + np.arange(hd, dtype=np.float64)[None, :] / 128.0).astype(F32)
    Rw = (Rh.astype(np.float64) + 256.0).astype(F32)
    return q, Rh, Rw


def random_inputs(hd, size, seed, nb=B, heads=HEADS):
    """-> q [nb * S, ldq] fp32 (the k | v columns random as well), Rh, Rw [2 * size - 1, hd] fp32 (module docstring)"""
    S, L = size * size, 2 * size - 1
    rng = np.random.default_rng([seed, hd, size])
    q = rng.standard_normal((nb, S, ldq(hd, heads))).astype(F32)
    q[:, 0:4] *= F32(30.0)
    q[:, 4:8] *= F32(0.01)
    Rh = (0.1 * rng.standard_normal((L, hd))).astype(F32)
    Rw = (0.1 * rng.standard_normal((L, hd))).astype(F32)
    return q.reshape(nb * S, -1), Rh, Rw


def split_planes(q):
    """the planes the GPU test hands over: hi = fp16(q), lo = fp16(q - hi)"""
    hi = q.astype(np.float16)
    lo = (q - hi.astype(F32)).astype(np.float16)
    return hi, lo


# --------------------------------------------------------------------------------------------------------------- reference
def rel_index(size):
    """-> (ih, iw) [S, size]: the table row of entry (q, k) on the height and on the width axis"""
    tok, k = np.arange(size * size)[:, None], np.arange(size)[None, :]
    return tok // size - k + size - 1, tok % size - k + size - 1


def _heads_of(q, nb, heads, hd, S):
    return q[:, :heads * hd].reshape(nb, S, heads, hd).transpose(0, 2, 1, 3).reshape(nb * heads, S, hd)


def _gathered(T, size):
    ih, iw = rel_index(size)
    return (np.take_along_axis(T[0], np.broadcast_to(ih, (T[0].shape[0],) + ih.shape), axis=2),
            np.take_along_axis(T[1], np.broadcast_to(iw, (T[1].shape[0],) + iw.shape), axis=2))


def reference(q, Rh, Rw, size, nb=B, heads=HEADS, magnitude=False):
    """-> rel_h, rel_w [nb * heads, S, size] in float64.  q: [nb * S, ldq] (any float type; planes: pass hi + lo in float64).
    magnitude=True: A = sum_c |q_c| |R_c| of every entry instead (the scale of `bound`)."""
    S, hd = size * size, Rh.shape[1]
    qv = _heads_of(np.asarray(q, dtype=np.float64), nb, heads, hd, S)
    rh, rw = np.asarray(Rh, dtype=np.float64), np.asarray(Rw, dtype=np.float64)
    if magnitude:
        qv, rh, rw = np.abs(qv), np.abs(rh), np.abs(rw)
    return _gathered((qv @ rh.T, qv @ rw.T), size)       # [BH, S, L] products of every table row, then the (q, k) entries


def bound(kind, hd, A):
    """the per-entry error bound of a kernel family (module docstring); A from reference(..., magnitude=True)"""
    if kind == "f32":
        return hd * 2.0 ** -24 * A
    assert kind == "x3", kind
    return (2.0 ** -20 + hd * 2.0 ** -24) * A + 1e-7


# ---------------------------------------------------------------------------------------------------------------- checkers
def probe_mismatches(got, want, limit=12):
    """-> ['rel_h[bh 1, q 13, k 0]: got 26.0546875, want 27.0546875', ...] for the entries of (rel_h, rel_w) that are not
    bit-equal to the reference (at most `limit` per tensor, in index order) and the total count"""
    lines, total = [], 0
    for name, g, w in zip(("rel_h", "rel_w"), got, want):
        bad = np.argwhere(np.asarray(g, dtype=np.float64) != w)
        total += len(bad)
        for bh, tok, k in bad[:limit]:
            lines.append(f"{name}[bh {bh}, q {tok}, k {k}]: got {float(g[bh, tok, k])!r}, want {float(w[bh, tok, k])!r}")
    return lines, total


def worst_ratio(got, want, bnd):
    """-> (max over both tensors of |got - want| / bound, 'rel_w[bh, q, k]' of that entry, its |error|)"""
    best = (-1.0, "", 0.0)
    for name, g, w, b in zip(("rel_h", "rel_w"), got, want, bnd):
        err = np.abs(np.asarray(g, dtype=np.float64) - w)
        ratio = np.where(np.isfinite(err), err / b, np.inf)
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        if ratio[i] > best[0]:
            best = (float(ratio[i]), f"{name}[bh {i[0]}, q {i[1]}, k {i[2]}]", float(err[i]))
    return best


# ------------------------------------------------------------------------------------------------------------ kernel names
_KERNELS = (r"(relpos_(?:gather|direct|mfma)_kernel|win_maps_kernel|win_partition(?:_split)?_kernel|win_unpartition_add_kernel|"
            r"fill_rows(?:_split)?_kernel|layernorm_(?:split|vec|any)_kernel|gemm_f32_kernel)")


def kernel_id(name):
    """'relpos_mfma_kernel<64,1,0>' from a demangled ('... relpos_mfma_kernel<64, 1, false>(float const*, ...)') or an
    Itanium-mangled ('..._118relpos_mfma_kernelILi64ELi1ELb0EEEvPKf...') kernel name of the encoder's glue, booleans as 0 / 1;
    the bare name for a non-template and for GEMM (a GEMM's template arguments are tuning); None for any other kernel"""
    m = re.search(_KERNELS + r"(?:<([^()]*)>|I((?:L[ib]-?\d+E)+)E)?", name)
    if not m:
        return None
    if m.group(1) == GEMM:
        return GEMM
    if m.group(2) is not None:
        args = [a.strip() for a in m.group(2).split(",")]
    else:
        args = re.findall(r"L[ib](-?\d+)E", m.group(3) or "")
    args = [{"true": "1", "false": "0"}.get(a, a) for a in args]
    return m.group(1) + (f"<{','.join(args)}>" if args else "")


def kernel_ids(names):
    """kernel_id of every name, a foreign kernel under its own name (so that it cannot hide in a comparison)"""
    return [kernel_id(n) or n for n in names]
