"""GPU: the rel-pos producers of the SAM image encoder, kernel by kernel, through hgl_sam_relpos_tables -- the exported face of the
function the encoder itself calls to pick a producer (csrc/sam_api.hip: enc_relpos_tables).

Every row of tests/relpos_cases.py:CASES (the reference, the inputs, the bounds and their derivation live there, checked on the
CPU by tests/test_relpos_cases_host.py) runs B = 2 items of 3 heads, q packed as the encoder packs it (rows of 3 * heads * hd,
q in the first third), under the library precision of the row, and is held to four things:

* the kernels the call launches are the row's, in order (torch.profiler: abi_ref.launched_kernels);
* the index probes come out bit-equal to the float64 reference, every entry of both tensors -- a failure lists the (bh, q, k)
  that differ;
* on random data every entry is within the bound of the kernel that multiplied ("f32": hd * 2^-24 * A; "x3": (2^-20 + hd *
  2^-24) * A + 1e-7; A = sum |q_c| |R_c|); the worst ratio of error to bound is printed;
* rel_h / rel_w live inside a larger buffer filled with a sentinel: every output entry is written, nothing around them is.

The generic producer (two GEMMs + two gathers) multiplies with the fp32 matrix-core GEMM in EVERY precision mode -- one batch
per head, and the split-fp16 small-tile GEMM serves single batches only -- so its rows carry the tighter "f32" bound in f16x3 and
f16 mode as well; the kernel-name assertion is what licenses that.

Measured on an MI355X (every row: kernels as listed in CASES, probes exact); worst |error| / bound on the random data:

  relpos_direct_kernel ("f32")        hd 64: 0.032 (size 2), 0.052 (8), 0.079 (14), 0.084 (28), 0.090 (64)
                                      hd 80: 0.018 (2), 0.043 (14), 0.061 (28), 0.068 (64); the same bits in f32, f16x3 and f16 mode
  relpos_mfma_kernel, fp32 q ("x3")   <64,1> 0.147, <64,4> 0.189, <80,1> 0.125, <80,4> 0.145 (f16x3 and f16 mode alike)
  relpos_mfma_kernel, planes ("x3")   <64,1> 0.040, <64,4> 0.052, <80,1> 0.036, <80,4> 0.046
  GEMM + gather ("f32")               hd 16: 0.202 (14), 0.268 (16); hd 32: 0.109 (14), 0.110 (16); hd 64: 0.050 (7), 0.053 (13),
                                      0.090 (66); the same in every mode (the same fp32 GEMM)

No kernel comes near its bound: a worst-case bound over hd roundings against errors that add up like a random walk.
"""
import numpy as np
import pytest
import torch

import abi_ref
import relpos_cases as R
from hybridgl_amd import _lib, ops

pytestmark = pytest.mark.gpu


def _outputs(size, dev):
    """-> (buf, rel_h, rel_w, inside): the two outputs as views into one sentinel-filled buffer, guard zones in front of, between
    and behind them; inside = bool mask of the output elements"""
    n = R.B * R.HEADS * size * size * size
    step = (n + 63) // 64 * 64                     # both outputs 256-byte aligned
    oh, ow = R.GUARD, 2 * R.GUARD + step
    buf = torch.full((ow + step + R.GUARD,), R.SENTINEL, dtype=torch.float32, device=dev)
    shape = (R.B * R.HEADS, size * size, size)
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=dev)
    inside[oh:oh + n] = True
    inside[ow:ow + n] = True
    return buf, buf[oh:oh + n].view(shape), buf[ow:ow + n].view(shape), inside


def _call(case, q, Rh, Rw, dev, profiled):
    """one call of the entry on numpy inputs -> (rel_h, rel_w as numpy, the float64 q the kernel was given, kernel ids or None)"""
    qd = torch.from_numpy(q).to(dev)
    if case.q == "planes":
        hi = qd.half()
        lo = (qd - hi.float()).half()
        qarg, q64 = (hi, lo), hi.double().cpu().numpy() + lo.double().cpu().numpy()
    else:
        qarg, q64 = qd, q.astype(np.float64)
    th, tw = torch.from_numpy(Rh).to(dev), torch.from_numpy(Rw).to(dev)
    buf, rel_h, rel_w, inside = _outputs(case.size, dev)

    def run():
        ops.sam_relpos_tables(qarg, th, tw, R.B, R.HEADS, case.size, rel_h=rel_h, rel_w=rel_w)

    names = None
    if profiled:
        names = R.kernel_ids(abi_ref.launched_kernels(run))
    else:
        run()
    torch.cuda.synchronize()
    assert bool((buf[~inside] == R.SENTINEL).all()), "the call wrote outside rel_h / rel_w"
    assert not bool((buf[inside] == R.SENTINEL).any()), "entries of rel_h / rel_w were left unwritten"
    return (rel_h.cpu().numpy(), rel_w.cpu().numpy()), q64, names


@pytest.mark.parametrize("cid", [R.case_id(c) for c in R.CASES])
def test_relpos_tables_case(cuda, cid):
    case = {R.case_id(c): c for c in R.CASES}[cid]
    try:
        ops.set_precision(case.precision)
        # index probes: the kernels of the row, every entry exact
        q, Rh, Rw = R.probe_inputs(case.hd, case.size)
        got, q64, names = _call(case, q, Rh, Rw, cuda, profiled=True)
        assert tuple(names) == case.kernels, (names, case.kernels)
        lines, total = R.probe_mismatches(got, R.reference(q64, Rh, Rw, case.size))
        assert total == 0, f"{total} entries differ from the reference:\n" + "\n".join(lines)
        # random data: every entry within the bound of the kernel that multiplied
        q, Rh, Rw = R.random_inputs(case.hd, case.size, 1)
        got, q64, _ = _call(case, q, Rh, Rw, cuda, profiled=False)
        want = R.reference(q64, Rh, Rw, case.size)
        A = R.reference(q64, Rh, Rw, case.size, magnitude=True)
        ratio, where, err = R.worst_ratio(got, want, [R.bound(case.bound, case.hd, a) for a in A])
        print(f"relpos {cid}: {' + '.join(names)}; probes exact; worst error / bound({case.bound}) = {ratio:.3f} at {where} "
              f"(|error| {err:.3e})")
        assert ratio <= 1.0, (ratio, where, err)
    finally:
        ops.set_precision(ops.default_precision())


def test_relpos_tables_refuses_what_no_producer_serves(cuda):
    """loud failures, nothing enqueued: q as planes outside f16x3 mode, planes at a shape the plane kernel does not take, a head dim
    the attention dispatcher does not know, S that is not size * size, a workspace that is too small"""
    lib = _lib.load()
    hd, size = 64, 14
    q, Rh, Rw = R.probe_inputs(hd, size)
    qd, th, tw = (torch.from_numpy(x).to(cuda) for x in (q, Rh, Rw))
    planes = (qd.half(), torch.zeros_like(qd, dtype=torch.float16))
    try:
        for mode in ("f32", "f16"):
            ops.set_precision(mode)
            with pytest.raises(_lib.HybridGLError, match="f16x3 mode only"):
                ops.sam_relpos_tables(planes, th, tw, R.B, R.HEADS, size)
        ops.set_precision("f16x3")
        q8, Rh8, Rw8 = R.probe_inputs(hd, 8)
        q8 = torch.from_numpy(q8).to(cuda)
        with pytest.raises(_lib.HybridGLError, match="relpos_split: unsupported shape"):
            ops.sam_relpos_tables((q8.half(), q8.half()), torch.from_numpy(Rh8).to(cuda), torch.from_numpy(Rw8).to(cuda), R.B, R.HEADS, 8)
        out = torch.empty((R.B * R.HEADS, size * size, size), dtype=torch.float32, device=cuda)
        need = lib.hgl_sam_relpos_tables_workspace_bytes(R.B, R.HEADS, size * size, size)
        assert need >= 2 * 4 * R.HEADS * R.B * size * size * (2 * size - 1)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)

        def raw(S=size * size, hd_=hd, nbytes=need):
            return lib.hgl_sam_relpos_tables(qd.data_ptr(), None, None, qd.shape[1], R.B, R.HEADS, S, size, hd_, th.data_ptr(),
                                             tw.data_ptr(), out.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, None)
        assert raw(hd_=48) == -1 and b"unsupported head dim 48" in lib.hgl_last_error()
        assert raw(S=size * size + 1) == -1 and b"bad shape" in lib.hgl_last_error()
        assert raw(nbytes=need - 256) == -3 and b"workspace too small" in lib.hgl_last_error()
    finally:
        ops.set_precision(ops.default_precision())
