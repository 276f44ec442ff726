"""GPU: the split-fp16 GEMM dispatch (hgl_gemm_route / hgl_launch_gemm, csrc/gemm_f16x3.hip) pinned by kernel name.

Every row calls ops.gemm_f16x3 (the exported hgl_gemm_f16x3: A split on the fly, then the launch the model code's plane
GEMMs take) and names, literally, the kernels it must enqueue after the split:
  gemm_f16x3_kernel<ACT,64,2,NT>   register-staged 128 x 128 tiling; NT products per step (3 f16x3, 1 f16)
  gemm_x3p_kernel<ACT,WLOADS,NT>   ping-pong 256 x 256 tiling; WLOADS the write-out flavour (0 reads nothing, 1 residual rows);
                                   NT = 3, 2 for an fp16-valued weight (all-zero lo plane; 3 again with HGL_X3_TERMS=3), 1 in f16 mode
  splitk_reduce_kernel             behind the split-K tail of the row-balanced launch
ACT is the HGL_ACT_* number (none 0, quickgelu 1, gelu 2, relu 3).  The tilings give bit-identical outputs by design, so
the kernel that ran is read from the profiler (abi_ref.launched_kernels), not inferred from results.  The automatic rows
sit far from the cost model's crossover at the MI355X's 256 CUs (300 x 200 x 64: 10 against 23 us; 4096 x 4096 x 64
without a residual: 32 against 23 us); the row-balanced rows are the shapes of test_gemm_f16x3_row_balanced_launch
(800 tiles = 3.125 rounds: 153 row tiles of whole rounds + a 3-slice split-K tail; 1280 tiles = 5 rounds: one launch).

Each result is held to a float64 product: 3e-5 relative to max(1, |z|) (test_gemm_f16x3's bound), in f16 mode
abi_ref.gemm_f16_reference's.  Row maps, rmod, gathered A rows and plane outputs are not reachable through the exported ABI:
the model-level tests cover them.
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import abi_ref as R
from hybridgl_amd import ops

pytestmark = pytest.mark.gpu

Row = namedtuple("Row", "name select mode shape weight res act terms balanced kernels")


def row(name, select, kernels, shape=(300, 200, 64), mode="f16x3", weight="fp32", res=True, act="none", terms=None,
        balanced=False):
    return Row(name, select, mode, shape, weight, res, act, terms, balanced, kernels)


V1, P = "gemm_f16x3_kernel", "gemm_x3p_kernel"
REDUCE = "splitk_reduce_kernel"
CASES = [
    # forced register-staged
    row("v1_f16x3", "v1", [V1 + "<0,64,2,3>"]),
    row("v1_f16", "v1", [V1 + "<0,64,2,1>"], mode="f16"),
    # forced ping-pong: write-out flavour x products
    row("p_fp32w", "P", [P + "<0,0,3>"], res=False),
    row("p_fp32w_res", "P", [P + "<0,1,3>"]),
    row("p_fp16w", "P", [P + "<0,0,2>"], weight="fp16", res=False),
    row("p_fp16w_res", "P", [P + "<0,1,2>"], weight="fp16"),
    row("p_fp16w_res_terms3", "P", [P + "<0,1,3>"], weight="fp16", terms="3"),
    row("p_fp16w_terms3", "P", [P + "<0,0,3>"], weight="fp16", res=False, terms="3"),
    row("p_f16", "P", [P + "<0,0,1>"], mode="f16", res=False),
    row("p_f16_res", "P", [P + "<0,1,1>"], mode="f16"),
    row("p_f16_fp16w_res", "P", [P + "<0,1,1>"], mode="f16", weight="fp16"),
    # forced ping-pong, N % 4 != 0: no 16-byte write-out, the register-staged kernel runs
    row("p_n202", "P", [V1 + "<0,64,2,3>"], shape=(300, 202, 64)),
    row("p_n202_f16", "P", [V1 + "<0,64,2,1>"], shape=(300, 202, 64), mode="f16"),
    # automatic
    row("auto_small", "auto", [V1 + "<0,64,2,3>"]),
    row("auto_4096", "auto", [P + "<0,0,3>"], shape=(4096, 4096, 64), res=False),
    # the activations
    row("p_quickgelu", "P", [P + "<1,1,3>"], act="quickgelu"),
    row("p_gelu", "P", [P + "<2,1,3>"], act="gelu"),
    row("p_relu", "P", [P + "<3,1,3>"], act="relu"),
    row("v1_quickgelu", "v1", [V1 + "<1,64,2,3>"], act="quickgelu"),
    row("v1_gelu", "v1", [V1 + "<2,64,2,3>"], act="gelu"),
    row("v1_relu", "v1", [V1 + "<3,64,2,3>"], act="relu"),
    # row-balanced: whole rounds (residual write-out) + split-K tail (raw partial sums) + reduce; exactly 5 rounds: one launch
    row("balanced_tail", "auto", [P + "<0,1,3>", P + "<0,0,3>", REDUCE], shape=(160 * 256, 1280, 1280), balanced=True),
    row("balanced_whole_rounds", "auto", [P + "<0,1,3>"], shape=(256 * 256, 1280, 1280), balanced=True),
]
SAMPLE_ROWS = 64      # rows of the two large shapes that are compared (first, last -- the tail's -- and spread)


def _short(name):
    for raw in ("split_f16_kernel", REDUCE):
        if raw in name:
            return raw
    return name


@pytest.fixture(scope="module")
def dispatch_results(cuda):
    """the whole table in ONE profiled pass, then the float64 checks"""
    g = torch.Generator(device=cuda).manual_seed(20)
    weights, acts = {}, {}
    for r in CASES:
        M, N, K = r.shape
        if (r.weight, N, K) not in weights:
            w = torch.randn((N, K), device=cuda, generator=g) / K ** 0.5
            weights[(r.weight, N, K)] = w.half().float() if r.weight == "fp16" else w
            ops.register_split_weight(weights[(r.weight, N, K)])       # (its kernels stay out of the profiled pass)
        if r.shape not in acts:
            acts[r.shape] = (torch.randn((M, K), device=cuda, generator=g), torch.randn((N,), device=cuda, generator=g),
                             torch.randn((M, N), device=cuda, generator=g))
    outs = {}

    def run():
        for r in CASES:
            M, N, K = r.shape
            a, b, res = acts[r.shape]
            ops.set_precision(r.mode)
            ops.select_x3_kernel(r.select)
            if r.terms:
                os.environ["HGL_X3_TERMS"] = r.terms
            else:
                os.environ.pop("HGL_X3_TERMS", None)
            outs[r.name] = ops.gemm_f16x3(a, weights[(r.weight, N, K)], b, res if r.res else None, r.act,
                                          balanced=r.balanced)

    results = {}
    try:
        names = [_short(n) for n in R.launched_kernels(run)]
        starts = [i for i, n in enumerate(names) if n == "split_f16_kernel"]     # every call splits A first
        assert len(starts) == len(CASES) and starts[0] == 0, names
        for i, r in enumerate(CASES):
            M, N, K = r.shape
            a, b, res = acts[r.shape]
            w = weights[(r.weight, N, K)]
            rows = (torch.arange(M, device=cuda) if M <= 4096 else
                    torch.cat([torch.arange(8, device=cuda), torch.arange(M - 8, M, device=cuda),
                               torch.linspace(8, M - 9, SAMPLE_ROWS - 16, device=cuda).long()]))
            y = outs[r.name][rows].double()
            if r.mode == "f16":
                z, bound = R.gemm_f16_reference(a.cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(),
                                                res.cpu().numpy() if r.res else None, r.act, rows=rows.cpu().numpy())
                ratio = float((np.abs(y.cpu().numpy() - z) / bound).max())
            else:
                z = R.activation64(a[rows].double() @ w.double().T + b.double(), r.act)
                if r.res:
                    z = z + res[rows].double()
                ratio = float(((y - z).abs() / torch.clamp(z.abs(), min=1.0)).max()) / 3e-5
            end = starts[i + 1] if i + 1 < len(starts) else len(names)
            results[r.name] = dict(kernels=names[starts[i] + 1:end], finite=bool(torch.isfinite(y).all()), ratio=ratio)
    finally:
        os.environ.pop("HGL_X3_TERMS", None)
        ops.select_x3_kernel("auto")
        ops.set_precision(ops.default_precision())
        torch.cuda.synchronize()
        ops.release_split_weights([w.data_ptr() for w in weights.values()])
    return results


@pytest.mark.parametrize("r", CASES, ids=[r.name for r in CASES])
def test_dispatch_row(dispatch_results, r):
    res = dispatch_results[r.name]
    print(r.name, res)
    assert res["kernels"] == r.kernels, res
    assert res["finite"], res
    assert res["ratio"] <= 1.0, res       # error / bound
