"""GPU: every branch of the attention dispatcher (hgl_attention_route / hgl_launch_attention, csrc/attention.hip) against a
float64 reference, at the layouts the model code hands it and at the lengths where tiles end.

Each row of CASES names the kernel it must reach in the split-fp16 modes ({T}: TERMS = 3 in f16x3, 1 in f16); in f32 mode
every row except those of the two fp32-only kernels reaches attn_f32_kernel<hd>.  Sibling kernels give bit-identical
outputs by design, so the kernel that ran is read from the profiler (abi_ref.launched_kernels), not inferred from results.

Every row writes through ldo > D at an element offset with a batch stride beyond Sq * ldo into a buffer pre-filled with a
sentinel, which must survive outside the output view.  Input elements outside the operands' views are NaN: a kernel that
reads beyond its rows or head columns turns its output into NaN.

attn_smallk_kernel and attn_fewq_kernel have no TERMS flavour: they evaluate scores, soft-max and P V in fp32 on the vector
ALUs in every mode (the split modes only change the output format of the model's internal calls, not of this ABI), so they
are held to the fp32 bound in f16 mode too.  attn_x3_kernel<64,0,8,T> is not reachable in the production build: head
dim 64 at 129..256 queries takes attn_x3q_kernel (HGL_ATTN_DUAL is a diagnostic-build switch).
"""
from collections import namedtuple

import pytest
import torch

import abi_ref as R
from hybridgl_amd import ops

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x3", "f16"]
FP32_ONLY = ("attn_smallk_kernel", "attn_fewq_kernel")
SENTINEL = -7.25e30

Row = namedtuple("Row", "name kernel B H Sq Sk hd layout mask keep_b0 keep_n rel")


def row(name, kernel, B, H, Sq, Sk, hd, layout="dense", mask="none", keep_b0=0, keep_n=0, rel=None):
    return Row(name, kernel, B, H, Sq, Sk, hd, layout, mask, keep_b0, keep_n, rel)


X3 = "attn_x3_kernel<{hd},0,4,{T}>"
CASES = [
    # attn_x3_kernel<HD,0,4,T> (f32: attn_f32_kernel<HD>): short / ragged sequences, causal, CLS-keep, rel-pos tensors
    row("h16_q1_k33", X3, 3, 2, 1, 33, 16),
    row("h16_q31_k1_vshared", X3, 2, 4, 31, 1, 16, "v_shared"),
    row("h16_causal300_packed_xcd", X3, 2, 4, 300, 300, 16, "packed", "causal"),           # B*H = 8, 3 query blocks
    row("h16_q2048_k32_qshared", X3, 1, 3, 2048, 32, 16, "q_shared"),
    row("h32_q127_k129_vshared", X3, 3, 2, 127, 129, 32, "v_shared"),
    row("h32_q257_k255_qshared_xcd", X3, 2, 4, 257, 255, 32, "q_shared"),
    row("h32_cls_b0_1_n0", X3, 4, 2, 197, 197, 32, "dense", "cls_keep", 1, 0),             # keep_n <= 0: B rows
    row("h32_q1_packed", X3, 2, 3, 1, 1, 32, "packed"),
    row("h64_q128_k2047", X3, 2, 2, 128, 2047, 64),
    row("h64_causal256_packed_xcd", X3, 1, 8, 256, 256, 64, "packed", "causal"),
    row("h64_cls_q1", X3, 3, 2, 1, 197, 64, "dense", "cls_keep", 1, 2),
    row("h64_rel_6x10_vshared", X3, 2, 3, 60, 60, 64, "v_shared", rel=(6, 10)),
    row("h64_q33_k2100_qshared", X3, 2, 2, 33, 2100, 64, "q_shared"),
    row("h80_q33_k32_vshared", X3, 2, 3, 33, 32, 80, "v_shared"),
    row("h80_causal129", X3, 2, 2, 129, 129, 80, "dense", "causal"),
    row("h80_causal300_qshared_xcd", X3, 1, 8, 300, 300, 80, "q_shared", "causal"),
    row("h80_s1_packed", X3, 2, 2, 1, 1, 80, "packed"),
    row("h80_rel_4x32", X3, 2, 2, 40, 128, 80, "dense", rel=(4, 32)),
    row("h80_q2100_k31_qshared_xcd", X3, 2, 4, 2100, 31, 80, "q_shared"),
    row("h80_rel_48x48_no_pp", X3, 1, 2, 2304, 2304, 80, "dense", rel=(48, 48)),           # kw % 32 != 0: not ping-pong
    # attn_x3_kernel<80,0,8,T>: head dim 80, 129..256 queries, no causal mask / rel-pos, CLS-keep only up to 257 keys
    row("w8_cls_b0_1_n2", "attn_x3_kernel<80,0,8,{T}>", 4, 3, 197, 197, 80, "dense", "cls_keep", 1, 2),
    row("w8_q256_k1_qshared", "attn_x3_kernel<80,0,8,{T}>", 2, 2, 256, 1, 80, "q_shared"),
    row("w8_s129_packed", "attn_x3_kernel<80,0,8,{T}>", 2, 2, 129, 129, 80, "packed"),
    row("w8_q200_k300_vshared", "attn_x3_kernel<80,0,8,{T}>", 2, 2, 200, 300, 80, "v_shared"),
    # attn_x3q_kernel<64,2,T>: head dim 64, 129..256 queries (the CLIP sequences)
    row("x3q_cls_b0_0_n0", "attn_x3q_kernel<64,2,{T}>", 3, 4, 197, 197, 64, "dense", "cls_keep", 0, 0),
    row("x3q_q129_k33_qshared", "attn_x3q_kernel<64,2,{T}>", 2, 3, 129, 33, 64, "q_shared"),
    row("x3q_s256_packed", "attn_x3q_kernel<64,2,{T}>", 2, 2, 256, 256, 64, "packed"),
    row("x3q_q255_k2100_vshared", "attn_x3q_kernel<64,2,{T}>", 2, 2, 255, 2100, 64, "v_shared"),
    row("x3q_cls_k257_qshared", "attn_x3q_kernel<64,2,{T}>", 2, 2, 200, 257, 64, "q_shared", "cls_keep", 0, 1),
    # attn_x3_kernel<80,14,4,T>: SAM's 14 x 14 windows, rel-pos on the matrix cores
    row("w14_packed", "attn_x3_kernel<80,14,4,{T}>", 2, 2, 196, 196, 80, "packed", rel=(14, 14)),
    row("w14_q1", "attn_x3_kernel<80,14,4,{T}>", 2, 2, 1, 196, 80, "dense", rel=(14, 14)),
    row("w14_q300_qshared_xcd", "attn_x3_kernel<80,14,4,{T}>", 2, 4, 300, 196, 80, "q_shared", rel=(14, 14)),
    row("w14_vshared", "attn_x3_kernel<80,14,4,{T}>", 2, 2, 196, 196, 80, "v_shared", rel=(14, 14)),
    # attn_x3pp_kernel<HD,T>: >= 2048 queries and keys, no mask; with rel-pos only for kw % 32 == 0
    row("pp_h64_s2048_packed_xcd", "attn_x3pp_kernel<64,{T}>", 1, 8, 2048, 2048, 64, "packed"),
    row("pp_h80_s2100_qshared", "attn_x3pp_kernel<80,{T}>", 2, 1, 2100, 2100, 80, "q_shared"),
    row("pp_h80_rel_36x64_vshared", "attn_x3pp_kernel<80,{T}>", 1, 2, 2048, 2304, 80, "v_shared", rel=(36, 64)),
    row("pp_h64_rel_64x32", "attn_x3pp_kernel<64,{T}>", 1, 2, 2049, 2048, 64, "dense", rel=(64, 32)),
    # attn_smallk_kernel (no TERMS flavour): head dim 16, <= 8 keys, >= 256 queries, 256 % H == 0
    row("smallk_q256_k8", "attn_smallk_kernel", 2, 8, 256, 8, 16),
    row("smallk_q1000_k1_qshared", "attn_smallk_kernel", 2, 4, 1000, 1, 16, "q_shared"),
    row("smallk_q300_k5_vshared", "attn_smallk_kernel", 2, 16, 300, 5, 16, "v_shared"),
    # attn_fewq_kernel (no TERMS flavour): head dim 16, <= 8 queries, >= 1024 keys
    row("fewq_q1_k1024", "attn_fewq_kernel", 2, 8, 1, 1024, 16),
    row("fewq_q8_k4097_vshared", "attn_fewq_kernel", 3, 8, 8, 4097, 16, "v_shared"),
    row("fewq_q7_k2100_qshared", "attn_fewq_kernel", 2, 2, 7, 2100, 16, "q_shared"),
]
# Layouts no row of a family can have: packed q | k | v needs Sq == Sk (never for the few-key / few-query kernels), and the
# kernels chosen for 129..256 queries, >= 2048 queries or >= 256 queries never see Sq = 1.
assert all(r.rel is None or r.rel[0] * r.rel[1] == r.Sk for r in CASES)


def expected_kernel(r, mode):
    if r.kernel in FP32_ONLY:
        return r.kernel
    if mode == "f32":
        return f"attn_f32_kernel<{r.hd}>"
    return r.kernel.format(hd=r.hd, T=3 if mode == "f16x3" else 1)


def _operand(S, D, ld, sb, off, B, g, dev):
    """a flat buffer holding one operand (NaN outside its view; one shared copy when the batch stride is 0)"""
    buf = torch.full((R.extent(off, B, S, ld, sb, D),), float("nan"), device=dev)
    nb = B if sb else 1
    R.view(buf, off, nb, S, ld, sb, D).copy_(torch.randn((nb, S, D), device=dev, generator=g))
    return buf


def _inputs(r, dev, seed):
    """(call kwargs, reference kwargs, value tensor view) of a row"""
    g = torch.Generator(device=dev).manual_seed(seed)
    B, H, Sq, Sk, hd = r.B, r.H, r.Sq, r.Sk, r.hd
    D = H * hd
    if r.layout == "packed":
        assert Sq == Sk
        qkv = torch.randn((B * Sq * 3 * D,), device=dev, generator=g)
        q = k = v = qkv
        lay = dict(ldq=3 * D, ldk=3 * D, ldv=3 * D, sqb=Sq * 3 * D, skb=Sk * 3 * D, svb=Sk * 3 * D, oq=0, ok=D, ov=2 * D)
    else:
        wide = D + 8                                   # the operands that are not shared: padded rows and batch gaps
        st = {"q": (D, Sq * D, 0), "k": (D, Sk * D, 0), "v": (D, Sk * D, 0)}
        if r.layout in ("q_shared", "v_shared"):
            st = {"q": (wide, Sq * wide + 4, 4), "k": (wide, Sk * wide + 12, 8), "v": (wide, Sk * wide + 4, 4)}
            shared = r.layout[0]
            st[shared] = (D, 0, 4)
        else:
            assert r.layout == "dense", r.layout
        (ldq, sqb, oq), (ldk, skb, ok), (ldv, svb, ov) = st["q"], st["k"], st["v"]
        q = _operand(Sq, D, ldq, sqb, oq, B, g, dev)
        k = _operand(Sk, D, ldk, skb, ok, B, g, dev)
        v = _operand(Sk, D, ldv, svb, ov, B, g, dev)
        lay = dict(ldq=ldq, ldk=ldk, ldv=ldv, sqb=sqb, skb=skb, svb=svb, oq=oq, ok=ok, ov=ov)
    extra = dict(mask=r.mask)
    if r.mask == "cls_keep":
        n = r.keep_n if r.keep_n > 0 else B
        keep = torch.rand((n, Sk - 1), device=dev, generator=g) > 0.5
        keep[n - 1] = False                            # an all-zero keep row: the CLS query sees itself only
        extra.update(keep=keep.to(torch.uint8), keep_b0=r.keep_b0, keep_n=r.keep_n)
    if r.rel is not None:
        kh, kw = r.rel
        extra.update(rel_h=0.5 * torch.randn((B * H, Sq, kh), device=dev, generator=g),
                     rel_w=0.5 * torch.randn((B * H, Sq, kw), device=dev, generator=g))
    common = dict(B=B, H=H, Sq=Sq, Sk=Sk, hd=hd)
    return q, k, v, common, lay, extra


def _output(r, dev):
    D = r.H * r.hd
    ldo, oo = D + 8, 4
    sob = r.Sq * ldo + 8
    n = R.extent(oo, r.B, r.Sq, ldo, sob, D)
    return torch.full((n,), SENTINEL, device=dev), dict(ldo=ldo, sob=sob, oo=oo)


@pytest.fixture(scope="module")
def dispatch_results(cuda):
    """the whole table in each mode: one profiled pass of hgl_attention_f32 calls per mode, then the float64 checks"""
    results = {}
    try:
        for mode in MODES:
            ops.set_precision(mode)
            calls = []
            for i, r in enumerate(CASES):
                q, k, v, common, lay, extra = _inputs(r, cuda, 1000 + i)
                out, olay = _output(r, cuda)
                calls.append((r, q, k, v, common, lay, extra, out, olay))

            def run():
                for r, q, k, v, common, lay, extra, out, olay in calls:
                    R.attention(q, k, v, out, **common, **lay, **olay, **extra)

            names = R.launched_kernels(run)
            assert len(names) == len(calls), (
                f"{mode}: the profiler listed {len(names)} kernels for {len(calls)} attention calls: {names[:8]}")
            for (r, q, k, v, common, lay, extra, out, olay), name in zip(calls, names):
                ref_lay = {key: lay[key] for key in ("ldq", "ldk", "ldv", "sqb", "skb", "svb", "oq", "ok", "ov")}
                f16 = mode == "f16" and r.kernel not in FP32_ONLY
                ref = R.attention_reference(q, k, v, **common, **ref_lay, **extra, fp16_operands=f16)
                D = r.H * r.hd
                y = R.view(out, olay["oo"], r.B, r.Sq, olay["ldo"], olay["sob"], D)
                vv = R.view(v, lay["ov"], r.B, r.Sk, lay["ldv"], lay["svb"], D)
                bound = R.attention_f16_bound(vv) if f16 else (3e-5 if r.rel else 2e-5)
                inside = R.written_mask(out.numel(), olay["oo"], r.B, r.Sq, olay["ldo"], olay["sob"], D, cuda)
                results[(mode, r.name)] = dict(
                    kernel=name, finite=bool(torch.isfinite(y).all()), err=float((y.double() - ref).abs().max()), bound=bound,
                    sentinel=bool((out[~inside] == SENTINEL).all()))
            del calls
            torch.cuda.empty_cache()
    finally:
        ops.set_precision(ops.default_precision())
    return results


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", CASES, ids=[r.name for r in CASES])
def test_dispatch_row(dispatch_results, mode, r):
    res = dispatch_results[(mode, r.name)]
    assert res["kernel"] == expected_kernel(r, mode), res
    assert res["finite"], res
    assert res["err"] <= res["bound"], res
    assert res["sentinel"], f"the kernel wrote outside its output view: {res}"


# the families and flavours the table must reach, each with at least one row that is right in every respect
REQUIRED = ([f"attn_f32_kernel<{hd}>" for hd in (16, 32, 64, 80)]
            + [f"attn_x3_kernel<{hd},0,4,{t}>" for hd in (16, 32, 64, 80) for t in (1, 3)]
            + [f"attn_x3_kernel<80,0,8,{t}>" for t in (1, 3)] + [f"attn_x3q_kernel<64,2,{t}>" for t in (1, 3)]
            + [f"attn_x3_kernel<80,14,4,{t}>" for t in (1, 3)]
            + [f"attn_x3pp_kernel<{hd},{t}>" for hd in (64, 80) for t in (1, 3)] + list(FP32_ONLY))


def test_dispatch_reach_report(dispatch_results):
    """print which kernel families and flavours the table reached (rows right in kernel, numbers and sentinel), per mode;
    the ping-pong kernel must be reached with and without rel-pos"""
    ok = {}
    for r in CASES:
        for mode in MODES:
            res = dispatch_results[(mode, r.name)]
            good = (res["kernel"] == expected_kernel(r, mode) and res["finite"] and res["err"] <= res["bound"]
                    and res["sentinel"])
            if good:
                ok.setdefault(res["kernel"], []).append((mode, r.name, r.rel is not None))
    print("\nattention dispatch reach (kernel: verified rows per mode)")
    for name in sorted(ok):
        per_mode = {m: sum(1 for mm, _, _ in ok[name] if mm == m) for m in MODES}
        print(f"  {name:32s} " + "  ".join(f"{m} {per_mode[m]:2d}" for m in MODES))
    print("  attn_x3_kernel<64,0,8,*>        not reachable: head dim 64 at 129..256 queries runs attn_x3q_kernel")
    missing = [k for k in REQUIRED if k not in ok]
    assert not missing, missing
    for hd in (64, 80):
        for t in (1, 3):
            rels = {rel for _, _, rel in ok[f"attn_x3pp_kernel<{hd},{t}>"]}
            assert rels == {True, False}, (hd, t, rels)
