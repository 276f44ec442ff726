"""GPU: hgl_gemm_f32 through the C ABI at the layouts the model code uses and ops.gemm never produces -- batches with a
shared weight (sW = 0) and a shared residual (sR = 0), wide leading dims, the residual aliasing the output, no bias, K not a
multiple of the 32-wide K tile, edge tiles of one row or column -- with every activation, in all three precision modes,
with and without a registered fp16 split of the weight.  In the split modes a registered weight with M <= 1024, batch 1,
ldw == K and K % 16 == 0 takes the split-fp16 skinny kernel (gemm_f16x3.hip); everything else stays on the fp32 kernel.
The kernel that ran is read from the profiler.

Outputs are written into buffers pre-filled with a sentinel: elements outside the output view must keep it; input elements
outside the operands' views are NaN.  (Only a dense [N, K] weight with K % 8 == 0 can be registered: the other rows of the
"registered" variant run unregistered.)"""
import numpy as np
import pytest
import torch

import abi_ref as R
from hybridgl_amd import ops

pytestmark = pytest.mark.gpu

ACTS = ["none", "quickgelu", "gelu", "relu"]
SENTINEL = -7.25e30

# name, M, N, K, batch, wide (lda / ldw / ldc / ldr), wide_c (ldc / ldr only), shared W and R (sW = sR = 0), R aliases C, bias
CASES = [
    ("m1_n129_k36", 1, 129, 36, 1, False, False, False, False, True),
    ("m127_n128_k64_wide", 127, 128, 64, 1, True, False, False, False, True),
    ("m128_n127_k48_alias_widec", 128, 127, 48, 1, False, True, False, True, False),
    ("m129_n1_k100_nobias", 129, 1, 100, 1, False, False, False, False, False),
    ("b3_m129_n128_k96_shared", 129, 128, 96, 3, False, False, True, False, True),
    ("b3_m127_n129_k68_wide_alias_shared", 127, 129, 68, 3, True, False, True, True, True),
    ("m1_n128_k32_widec", 1, 128, 32, 1, False, True, False, False, True),
    ("m129_n129_k160_alias_widec", 129, 129, 160, 1, False, True, False, True, True),
    ("m127_n1_k256_widec", 127, 1, 256, 1, False, True, False, False, False),
]


def _buf(nb, rows, ld, sb, width, off, g, dev, scale=1.0):
    """flat buffer, NaN outside the view (a kernel that reads beyond its rows / columns turns its output into NaN)"""
    buf = torch.full((R.extent(off, nb, rows, ld, sb, width),), float("nan"), device=dev)
    n = nb if sb else 1
    R.view(buf, off, n, rows, ld, sb, width).copy_(torch.randn((n, rows, width), device=dev, generator=g) * scale)
    return buf


@pytest.mark.parametrize("registered", [False, True], ids=["plain", "registered"])
@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16"])
@pytest.mark.parametrize("name,M,N,K,batch,wide,wide_c,shared,alias,has_bias", CASES, ids=[c[0] for c in CASES])
def test_gemm_layout(cuda, mode, registered, name, M, N, K, batch, wide, wide_c, shared, alias, has_bias):
    g = torch.Generator(device=cuda).manual_seed(M * 131 + N * 7 + K + batch)
    lda, oa = (K + 8, 4) if wide else (K, 0)
    ldw, ow = (K + 4, 8) if wide else (K, 0)
    ldc, oc = (N + 3, 4) if (wide or wide_c) else (N, 0)
    ldr, orr = (N + 7, 8) if (wide or wide_c) else (N, 0)
    sA = M * lda + (4 if wide else 0)
    sW = 0 if shared else N * ldw
    sC = M * ldc + (5 if wide else 0)
    sR = 0 if shared else M * ldr + 4
    A = _buf(batch, M, lda, sA, K, oa, g, cuda)
    W = _buf(batch, N, ldw, sW, K, ow, g, cuda, K ** -0.5)
    bias = torch.randn((N,), device=cuda, generator=g) if has_bias else None
    skinny = mode != "f32" and registered and batch == 1 and M <= 1024 and ldw == K and K % 16 == 0
    outs, refs, resid = [], [], []
    for act in ACTS:
        C = torch.full((R.extent(oc, batch, M, ldc, sC, N),), SENTINEL, device=cuda)
        if alias:       # the residual is the output buffer itself, at the output's leading dim and batch stride
            R.view(C, oc, batch, M, ldc, sC, N).copy_(torch.randn((batch, M, N), device=cuda, generator=g))
            Rb, ldr_, sR_, orr_ = C, ldc, sC, oc
        else:
            Rb, ldr_, sR_, orr_ = _buf(batch, M, ldr, sR, N, orr, g, cuda), ldr, sR, orr
        refs.append(R.gemm_reference(A, W, bias, Rb, M, N, K, lda, ldw, ldr_, batch, sA, sW, sR_, oa, ow, orr_, act))
        resid.append(R.view(Rb, orr_, batch, M, ldr_, sR_, N)[0].cpu().numpy().copy())
        outs.append((C, Rb, ldr_, sR_, orr_))
    key = None
    try:
        ops.set_precision(mode)
        if registered and ldw == K and K % 8 == 0:
            key = ops.register_split_weight(torch.as_strided(W, (N, K), (K, 1), ow))

        def run():
            for act, (C, Rb, ldr_, sR_, orr_) in zip(ACTS, outs):
                R.gemm(A, W, bias, Rb, C, M, N, K, lda, ldw, ldr_, ldc, batch, sA, sW, sR_, sC, oa, ow, orr_, oc, act)

        names = R.launched_kernels(run)
        assert ops.split_overflow_count() == 0
    finally:
        if key is not None:
            ops.release_split_weights([key])
        ops.set_precision(ops.default_precision())
    T = 1 if mode == "f16" else 3
    for act, (C, *_), ref, res, kname in zip(ACTS, outs, refs, resid, names):
        a_ = ops.ACT[act]
        assert kname == (f"gemm_x3_skinny_kernel<{a_},{T}>" if skinny else f"gemm_f32_kernel<{a_},32,1,3>"), (act, names)
        y = R.view(C, oc, batch, M, ldc, sC, N)
        assert torch.isfinite(y).all(), act
        inside = R.written_mask(C.numel(), oc, batch, M, ldc, sC, N, cuda)
        assert (C[~inside] == SENTINEL).all(), f"{act}: written outside the output view"
        if skinny and mode == "f16":
            a = R.view(A, oa, 1, M, lda, sA, K)[0].cpu().numpy()
            w = R.view(W, ow, 1, N, ldw, sW, K)[0].cpu().numpy()
            z, bound = R.gemm_f16_reference(a, w, bias.cpu().numpy() if has_bias else None, res, act)
            ratio = np.abs(y[0].double().cpu().numpy() - z) / bound
            assert ratio.max() <= 1.0, (act, ratio.max())
        else:
            # f16x3 skinny kernel: fp32-class, 1.5x the fp32 kernel's tolerance (test_gemm_f16x3)
            tol = 3e-5 if skinny else 2e-5
            err = float((y.double() - ref).abs().max())
            assert err <= tol, (act, err)
