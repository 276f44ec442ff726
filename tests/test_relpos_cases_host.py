"""CPU checks of the rel-pos cases (tests/relpos_cases.py): the reference, the probes, the bounds and the checkers.

* the float64 reference equals oracle/sam_oracle.py's statement of the operation -- get_rel_pos plus the two einsums of
  encoder_attention -- evaluated in float64, to 1e-12, on three small shapes (even, odd, single-row windows; B = 2, 3 heads);
* the probe inputs are what the exactness argument needs: one 1.0 per query and head, tables exact in fp32 and exact as the
  fp16 hi + lo pair of the kernels' split; every reference entry of a probe is then one table entry, and a float32 evaluation
  in any order and the three-term split-fp16 evaluation both give it bit for bit;
* the bounds hold for CPU restatements of the two arithmetics on the random inputs -- a sequential float32 dot product with fused
  multiply-adds against "f32", the three-product fp16 hi / lo scheme with float32 accumulation against "x3" -- so a correct
  kernel passes, and the one-product fp16 scheme (what a kernel that dropped its lo terms would compute) does not;
* the checkers see planted errors and name the entry: an index off by one at a table edge, b and h swapped, the two tables
  swapped, one entry of the random data moved by twice its bound;
* the case table holds every row the GPU test is to run, under unique ids, and kernel_id reads both spellings of a kernel name.
"""
import numpy as np
import pytest

import relpos_cases as R
from oracle import sam_oracle as S


def oracle_tables(q, Rh, Rw, size, nb, heads):
    """the reference's formulation (get_rel_pos + einsum over the q grid), float64"""
    hd = Rh.shape[1]
    rq = R._heads_of(q.astype(np.float64), nb, heads, hd, size * size).reshape(nb * heads, size, size, hd)
    th = S.get_rel_pos(size, size, Rh.astype(np.float64))
    tw = S.get_rel_pos(size, size, Rw.astype(np.float64))
    rel_h = np.einsum("bhwc,hkc->bhwk", rq, th).reshape(nb * heads, size * size, size)
    rel_w = np.einsum("bhwc,wkc->bhwk", rq, tw).reshape(nb * heads, size * size, size)
    return rel_h, rel_w


@pytest.mark.parametrize("hd,size", [(16, 4), (32, 7), (80, 1)])
def test_reference_equals_the_oracles_formulation(hd, size):
    q, Rh, Rw = R.random_inputs(hd, size, 3)
    got = R.reference(q, Rh, Rw, size)
    want = oracle_tables(q, Rh, Rw, size, R.B, R.HEADS)
    for g, w in zip(got, want):
        assert g.shape == w.shape == (R.B * R.HEADS, size * size, size)
        assert np.abs(g - w).max() <= 1e-12


def _seq_f32(qv, T, how):
    """[BH, S, L] products of every table row, float32 accumulation.  how: "fma" (sequential float32 fused multiply-adds), "x3"
    (the three products of the fp16 hi / lo scheme) or "x1" (fp16 operands, one product)"""
    acc = np.zeros(qv.shape[:2] + (T.shape[0],), dtype=np.float32)
    if how == "fma":
        for c in range(qv.shape[2]):
            acc = (acc.astype(np.float64) + qv[:, :, c:c + 1].astype(np.float64) * T[None, None, :, c].astype(np.float64)).astype(np.float32)
        return acc
    qh, ql = R.split_planes(qv)
    th, tl = R.split_planes(T)
    terms = [(tl, qh), (th, ql), (th, qh)] if how == "x3" else [(th, qh)]
    for c in range(qv.shape[2]):
        for t, x in terms:      # every product of two fp16 values is exact in float32
            acc = (acc.astype(np.float64) + x[:, :, c:c + 1].astype(np.float64) * t[None, None, :, c].astype(np.float64)).astype(np.float32)
    return acc


def cpu_tables(q, Rh, Rw, size, how):
    qv = R._heads_of(q, R.B, R.HEADS, Rh.shape[1], size * size)
    return R._gathered((_seq_f32(qv, Rh, how), _seq_f32(qv, Rw, how)), size)


@pytest.mark.parametrize("hd,size", [(64, 14), (80, 5), (32, 66)])
def test_probe_inputs_are_exact_in_every_arithmetic(hd, size):
    q, Rh, Rw = R.probe_inputs(hd, size)
    S_ = size * size
    qh = q[:, :R.HEADS * hd].reshape(R.B * S_, R.HEADS, hd)
    assert ((qh == 1).sum(-1) == 1).all() and ((qh == 0).sum(-1) == hd - 1).all()      # one-hot per query and head
    bh, tok = 4, min(S_ - 1, 9)                                                            # b = 1, h = 1
    assert q[1 * S_ + tok, 1 * hd + (7 * tok + bh) % hd] == 1
    for T in (Rh, Rw):
        hi, lo = R.split_planes(T)
        assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), T.astype(np.float64))    # exact as hi + lo
    L = 2 * size - 1
    assert np.array_equal(Rh.astype(np.float64), np.arange(L)[:, None] + np.arange(hd)[None, :] / 128.0)
    assert np.array_equal(Rw.astype(np.float64), Rh.astype(np.float64) + 256.0)
    want = R.reference(q, Rh, Rw, size)
    ih, iw = R.rel_index(size)
    for w, T, idx in zip(want, (Rh, Rw), (ih, iw)):
        ch = (7 * np.arange(S_)[None, :, None] + np.arange(R.B * R.HEADS)[:, None, None]) % hd
        assert np.array_equal(w, T.astype(np.float64)[idx[None], ch])                     # every entry is ONE table entry
    if size <= 14:
        for how in ("fma", "x3"):
            lines, total = R.probe_mismatches(cpu_tables(q, Rh, Rw, size, how), want)
            assert total == 0, lines


@pytest.mark.parametrize("hd,size", [(64, 6), (80, 4), (16, 5)])
def test_bounds_hold_for_cpu_restatements_of_both_arithmetics(hd, size):
    q, Rh, Rw = R.random_inputs(hd, size, 11)
    want = R.reference(q, Rh, Rw, size)
    A = R.reference(q, Rh, Rw, size, magnitude=True)
    r32, where, _ = R.worst_ratio(cpu_tables(q, Rh, Rw, size, "fma"), want, [R.bound("f32", hd, a) for a in A])
    rx3, _, _ = R.worst_ratio(cpu_tables(q, Rh, Rw, size, "x3"), want, [R.bound("x3", hd, a) for a in A])
    rx1, _, _ = R.worst_ratio(cpu_tables(q, Rh, Rw, size, "x1"), want, [R.bound("x3", hd, a) for a in A])
    print(f"hd {hd} size {size}: float32 fma {r32:.3f} of its bound ({where}), three-term split {rx3:.3f}, one-term {rx1:.1f}")
    assert r32 <= 1.0 and rx3 <= 1.0
    assert rx1 > 10.0                     # fp16 operands miss the fp32-class bound by far: the bound tells the two apart
    # planes: the reference of hi + lo is what a kernel on planes is held against
    hi, lo = R.split_planes(q)
    wp = R.reference(hi.astype(np.float64) + lo.astype(np.float64), Rh, Rw, size)
    assert np.abs(wp[0] - want[0]).max() <= 2.0 ** -21 * A[0].max() + 1e-6


def test_the_scaled_rows_of_the_random_inputs():
    q, _, _ = R.random_inputs(64, 4, 5)
    q = q.reshape(R.B, 16, -1)
    rms = np.sqrt((q.astype(np.float64) ** 2).mean(-1))
    assert (rms[:, 0:4] > 20).all() and (rms[:, 4:8] < 0.02).all() and (np.abs(rms[:, 8:] - 1) < 0.3).all()


def test_checkers_name_planted_errors():
    hd, size = 64, 14
    q, Rh, Rw = R.probe_inputs(hd, size)
    want = R.reference(q, Rh, Rw, size)
    S_ = size * size
    # qc - k + size - 1 off by one at a table edge (the last query row, k = 0: the table's last row)
    g = [w.astype(np.float32) for w in want]
    g[0][1, S_ - 1, 0] = Rh[2 * size - 3, (7 * (S_ - 1) + 1) % hd]
    lines, total = R.probe_mismatches(g, want)
    assert total == 1 and lines[0].startswith(f"rel_h[bh 1, q {S_ - 1}, k 0]: got 25.")
    # b and h swapped (bh = h * B + b), the two tables swapped
    perm = [(bh % R.HEADS) * R.B + bh // R.HEADS for bh in range(R.B * R.HEADS)]
    _, total = R.probe_mismatches([w[perm].astype(np.float32) for w in want], want)
    assert total > S_ * size
    sw = R.reference(q, Rw, Rh, size)
    _, total = R.probe_mismatches([sw[0].astype(np.float32), sw[1].astype(np.float32)], want)
    assert total == 2 * R.B * R.HEADS * S_ * size
    # random data: one entry moved by twice its bound
    q, Rh, Rw = R.random_inputs(hd, size, 2)
    want = R.reference(q, Rh, Rw, size)
    bnd = [R.bound("x3", hd, a) for a in R.reference(q, Rh, Rw, size, magnitude=True)]
    g = [w.copy() for w in want]
    assert R.worst_ratio(g, want, bnd)[0] == 0.0
    g[1][5, 77, 13] += 2.0 * bnd[1][5, 77, 13]
    ratio, where, _ = R.worst_ratio(g, want, bnd)
    assert abs(ratio - 2.0) < 1e-6 and where == "rel_w[bh 5, q 77, k 13]"
    g[0][0, 0, 0] = np.nan
    assert R.worst_ratio(g, want, bnd)[0] == np.inf


def test_case_table_and_kernel_names():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    rows = {(c.precision, c.q, c.hd, c.size): c for c in R.CASES}
    for hd in (64, 80):
        for size in (2, 14, 28, 64):
            assert rows[("f32", "fp32", hd, size)].kernels == (f"relpos_direct_kernel<{hd}>",)
        assert rows[("f16x3", "fp32", hd, 14)].kernels == (f"relpos_mfma_kernel<{hd},1,0>",)
        assert rows[("f16x3", "fp32", hd, 64)].kernels == (f"relpos_mfma_kernel<{hd},4,0>",)
        for size, nt in ((14, 1), (64, 4)):
            assert rows[("f16x3", "planes", hd, size)].kernels == (f"relpos_mfma_kernel<{hd},{nt},1>",)
    for size in (8, 28):
        assert rows[("f16x3", "fp32", 64, size)].kernels == ("relpos_direct_kernel<64>",)
    for prec in ("f32", "f16x3"):
        for hd, size in [(16, 14), (16, 16), (32, 14), (32, 16), (64, 7), (64, 13), (64, 66)]:
            assert rows[(prec, "fp32", hd, size)].kernels == R.GENERIC
    for c in R.CASES:      # the bound is the bound of the kernel that multiplies
        assert c.bound == ("x3" if "mfma" in c.kernels[0] else "f32")
    assert R.kernel_id("void (anonymous namespace)::relpos_mfma_kernel<64, 1, false>(float const*, int)") == "relpos_mfma_kernel<64,1,0>"
    assert R.kernel_id("_ZN12_GLOBAL__N_118relpos_mfma_kernelILi80ELi4ELb1EEEvPKfiiiiS2_S2_PfS3_PKDF16_S5_") == "relpos_mfma_kernel<80,4,1>"
    assert R.kernel_id("_ZN12_GLOBAL__N_120relpos_direct_kernelILi64EEEvPKfiiiiS2_S2_PfS3_") == "relpos_direct_kernel<64>"
    assert R.kernel_id("(anonymous namespace)::relpos_gather_kernel(float const*, int, int)") == "relpos_gather_kernel"
    assert R.kernel_id("void (anonymous namespace)::gemm_f32_kernel<0, 32, 1, 3>((anonymous namespace)::GemmArgs)") == R.GEMM
    assert R.kernel_id("_ZN12_GLOBAL__N_122layernorm_split_kernelILi1EEEvPKfS2_S2_PDF16_S4_ifPKiS6_") == "layernorm_split_kernel<1>"
    assert R.kernel_id("win_partition_split_kernel(float const*)") == "win_partition_split_kernel"
    assert R.kernel_id("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>()") is None
    assert R.kernel_ids(["foreign_kernel", "fill_rows_kernel(float*)"]) == ["foreign_kernel", "fill_rows_kernel"]
