"""CPU: the opt-in fp16 precision mode (HGL_PREC_F16) at the ABI and in the compiler's assembly.  The one-term GEMM
instantiations must issue a third of the MFMAs of the three-term ones, stage no lo plane and stay inside the register /
scratch budget of the kernels they sit beside (hipcc cross-compiles gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybridgl_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hybridgl.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

MFMA = r"v_mfma_f32_16x16x32_f16|v_mfma_f32_32x32x16_f16"


def test_header_defines_f16_mode_and_keeps_abi_version():
    h = open(HEADER).read()
    assert re.search(r"^#define HGL_PREC_F32 0$", h, flags=re.M)
    assert re.search(r"^#define HGL_PREC_F16X3 1$", h, flags=re.M)
    assert re.search(r"^#define HGL_PREC_F16 2$", h, flags=re.M)
    assert re.search(r"^#define HGL_ABI_VERSION 7$", h, flags=re.M)


def test_python_knows_the_mode():
    from hybridgl_amd import ops
    assert ops.PRECISIONS == {"f32": 0, "f16x3": 1, "f16": 2}
    assert ops.split_mode("f16") and ops.split_mode("f16x3") and not ops.split_mode("f32")
    with pytest.raises(ValueError):
        ops.set_precision("bf16")


@pytest.fixture(scope="module")
def gemm_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("asm") / "gemm_f16x3.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()      # the flags the library is built with
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    flags = [f for f in flags if f != "-fPIC"]
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "gemm_f16x3.hip")],
                   check=True, capture_output=True, timeout=900)
    return out.read_text()


def _kernels(asm, base, nargs):
    """{template args tuple: (body, vgprs, scratch bytes)} of every instantiation of `base` (mangled names)"""
    found = {}
    for name in re.findall(r"^(_Z\S*%s(I\S*E)E\S*):" % base, asm, flags=re.M):
        name = name[0]
        targs = tuple(int(v) for v in re.findall(r"Li(\d+)E", name[name.index(base):]))
        assert len(targs) == nargs, name
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        v = int(re.search(r"\.set %s\.num_vgpr, (\d+)" % re.escape(name), asm).group(1))
        s = int(re.search(r"\.set %s\.private_seg_size, (\d+)" % re.escape(name), asm).group(1))
        found[targs] = (body, v, s)
    return found


def test_pingpong_one_term_instantiations(gemm_asm):
    """gemm_x3p_kernel<ACT, WLOADS, 1>: every activation / write-out flavour exists, one MFMA per product (a third of the
    NT = 3 kernel's, K tile by K tile: the kernel body is fully unrolled per K tile), one LDS-DMA piece per staging unit
    (the lo planes are never fetched), no scratch, no more VGPRs than NT = 3."""
    k = _kernels(gemm_asm, "gemm_x3p_kernel", 3)
    for act in range(4):
        for wl in range(3):
            assert (act, wl, 1) in k and (act, wl, 3) in k, (act, wl)
            b1, v1, s1 = k[(act, wl, 1)]
            b3, v3, s3 = k[(act, wl, 3)]
            m1, m3 = len(re.findall(MFMA, b1)), len(re.findall(MFMA, b3))
            d1, d3 = b1.count("global_load_lds_dwordx4"), b3.count("global_load_lds_dwordx4")
            assert m1 > 0 and 3 * m1 == m3, (act, wl, m1, m3)
            assert d1 > 0 and 2 * d1 == d3, (act, wl, d1, d3)
            assert s1 == 0 and s3 == 0
            assert v1 <= v3 <= 256


def test_register_staged_and_skinny_one_term(gemm_asm):
    """gemm_f16x3_kernel<ACT, 64, 2, 1> and gemm_x3_skinny_kernel<ACT, 1>: a third of the MFMAs, fewer global loads (no lo
    halves), no scratch."""
    k = _kernels(gemm_asm, "gemm_f16x3_kernel", 4)
    for act in range(4):
        b1, v1, s1 = k[(act, 64, 2, 1)]
        b3, v3, s3 = k[(act, 64, 2, 3)]
        assert 3 * len(re.findall(MFMA, b1)) == len(re.findall(MFMA, b3)) > 0
        assert b1.count("global_load_dwordx4") < b3.count("global_load_dwordx4")
        assert s1 == 0 and v1 <= v3
    k = _kernels(gemm_asm, "gemm_x3_skinny_kernel", 2)
    for act in range(4):
        b1, v1, s1 = k[(act, 1)]
        b3, v3, s3 = k[(act, 3)]
        assert 3 * len(re.findall(MFMA, b1)) == len(re.findall(MFMA, b3)) > 0
        assert b1.count("global_load_dwordx4") < b3.count("global_load_dwordx4")
        assert s1 == 0 and v1 <= v3


def test_attention_one_term_flavours(tmp_path):
    """attn_x3_kernel / attn_x3q_kernel / attn_x3pp_kernel with TERMS = 1: a third of the MFMAs of TERMS = 3 for Q K^T and
    P V (the windowed kernels keep the two MFMAs of the rel-pos bias per k-step), no scratch, no more VGPRs."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / "attention.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    subprocess.run([HIPCC] + [f for f in flags if f != "-fPIC"] + ["-S", "--cuda-device-only", "-o", str(out),
                   os.path.join(CSRC, "attention.hip")], check=True, capture_output=True, timeout=900)
    asm = out.read_text()
    seen = 0
    for base, nargs in (("attn_x3_kernel", 4), ("attn_x3q_kernel", 3), ("attn_x3pp_kernel", 2)):
        k = _kernels(asm, base, nargs)
        for targs, (b1, v1, s1) in k.items():
            if targs[-1] != 1:
                continue
            b3, v3, s3 = k[targs[:-1] + (3,)]
            m1, m3 = len(re.findall(r"v_mfma", b1)), len(re.findall(r"v_mfma", b3))
            relw = base == "attn_x3_kernel" and targs[1] > 0
            assert (m1 < m3 / 2) if relw else (3 * m1 == m3), (base, targs, m1, m3)
            assert s1 == 0 and v1 <= v3, (base, targs, v1, v3)
            seen += 1
    assert seen >= 10, seen
