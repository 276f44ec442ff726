"""Direct callers of the primitive C ABI and float64 references of the same operations (a helper module of the layout
tests, not a conftest).

ops.attention / ops.gemm / ops.layernorm hand the kernels dense, contiguous layouts only.  The model code calls the same
launchers with packed q | k | v (ld = 3D and pointer offsets), batch strides of zero (keys, values or queries shared
across batches), wide leading dims and residuals that alias the output.  The callers here take flat torch buffers plus
explicit leading dims, batch strides and ELEMENT offsets into those buffers, so that a test can build any of them.

The references evaluate the same operation in float64 on the buffers' device (torch, not the library): every operand is
read through the same (offset, leading dim, batch stride) view that the kernel is handed.
"""
import math
import re

import numpy as np
import torch

from hybridgl_amd import _lib, ops

# ---- buffers and views -----------------------------------------------------------------------------------------------------


def view(buf, off, nb, rows, ld, sb, width):
    """[nb, rows, width] view of a flat buffer: element (b, r, c) at off + b * sb + r * ld + c"""
    return torch.as_strided(buf, (nb, rows, width), (sb, ld, 1), off)


def extent(off, nb, rows, ld, sb, width):
    """one past the last element that view(off, nb, rows, ld, sb, width) touches"""
    return off + (nb - 1) * sb + (rows - 1) * ld + width


def written_mask(numel, off, nb, rows, ld, sb, width, device):
    """bool [numel]: the elements of a flat buffer that belong to the view (what a kernel may write)"""
    m = torch.zeros(numel, dtype=torch.bool, device=device)
    view(m, off, nb, rows, ld, sb, width).fill_(True)
    return m


def _ptr(buf, off=0):
    return buf.data_ptr() + off * buf.element_size() if buf is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- attention -------------------------------------------------------------------------------------------------------------


def attention(q, k, v, out, B, H, Sq, Sk, hd, ldq, ldk, ldv, ldo, sqb, skb, svb, sob, oq=0, ok=0, ov=0, oo=0, scale=None,
              mask="none", keep=None, keep_b0=0, keep_n=0, rel_h=None, rel_w=None):
    """hgl_attention_f32 on flat float32 buffers (q, k, v and out may be the same tensor) at element offsets oq / ok / ov / oo"""
    lib = _lib.load()
    kh = kw = 0
    if rel_h is not None:
        kh, kw = rel_h.shape[-1], rel_w.shape[-1]
    kp = None
    if keep is not None:
        kp = (keep.view(torch.uint8) if keep.dtype == torch.bool else keep).data_ptr()
    _lib.check(lib.hgl_attention_f32(_ptr(q, oq), _ptr(k, ok), _ptr(v, ov), _ptr(out, oo), B, H, Sq, Sk, hd, ldq, ldk, ldv, ldo,
                                     sqb, skb, svb, sob, float(hd ** -0.5 if scale is None else scale), ops.MASK[mask], kp,
                                     keep_b0, keep_n, _ptr(rel_h), _ptr(rel_w), kh, kw, _stream()), "hgl_attention_f32")


def attention_reference(q, k, v, B, H, Sq, Sk, hd, ldq, ldk, ldv, sqb, skb, svb, oq=0, ok=0, ov=0, scale=None, mask="none",
                        keep=None, keep_b0=0, keep_n=0, rel_h=None, rel_w=None, fp16_operands=False):
    """softmax(scale q k^T + mask + bias) v in float64 -> [B, Sq, H * hd].

    mask: "causal" hides key j > query i; "cls_keep" hides, for batches b >= keep_b0, the keys j >= 1 of query 0 whose byte
    keep[(b - keep_b0) % n, j - 1] is zero (n = keep_n, or B when keep_n <= 0; include/hybridgl.h).  rel_h / rel_w
    [B * H, Sq, kh] / [B * H, Sq, kw]: bias[query, key] = rel_h[query, key // kw] + rel_w[query, key % kw].
    fp16_operands: the operands of the one-term (f16 mode) kernels -- fp16(q * scale), fp16(k), fp16(v) -- as in
    tests/test_gpu_f16_mode.py (test_attention_f16_is_the_fp16_operand_attention); see attention_f16_bound."""
    D = H * hd
    scale = hd ** -0.5 if scale is None else scale

    def heads(buf, off, S, ld, sb):
        return view(buf, off, B, S, ld, sb, D).reshape(B, S, H, hd).permute(0, 2, 1, 3)

    qf, kf, vf = heads(q, oq, Sq, ldq, sqb), heads(k, ok, Sk, ldk, skb), heads(v, ov, Sk, ldv, svb)
    if fp16_operands:
        qs = (qf * np.float32(scale)).half().double()
        sc = qs @ kf.half().double().transpose(-1, -2)
        vs = vf.half().double()
    else:
        sc = (qf.double() @ kf.double().transpose(-1, -2)) * scale
        vs = vf.double()
    if rel_h is not None:
        kh, kw = rel_h.shape[-1], rel_w.shape[-1]
        key = torch.arange(Sk, device=q.device)
        sc = sc + rel_h.double().reshape(B, H, Sq, kh)[..., key // kw] + rel_w.double().reshape(B, H, Sq, kw)[..., key % kw]
    hide = torch.zeros((B, 1, Sq, Sk), dtype=torch.bool, device=q.device)
    if mask == "causal":
        hide |= torch.ones((Sq, Sk), dtype=torch.bool, device=q.device).triu(1)
    elif mask == "cls_keep":
        n = keep_n if keep_n > 0 else B
        for b in range(keep_b0, B):
            hide[b, 0, 0, 1:] = keep[(b - keep_b0) % n] == 0
    sc = sc.masked_fill(hide, -math.inf)
    p = torch.softmax(sc, dim=-1)
    return (p @ vs).permute(0, 2, 1, 3).reshape(B, Sq, D)


def attention_f16_bound(v_values):
    """error bound of the one-term (f16 mode) attention against attention_reference(fp16_operands=True): the fp16 rounding
    of P (<= 2^-11 relative per probability: <= 2^-11 max|v| on the output; bound 2^-10 max|v|) and fp32 accumulation
    (tests/test_gpu_f16_mode.py)"""
    return 2.0 ** -10 * float(v_values.abs().max()) + 1e-5


# ---- GEMM and LayerNorm ----------------------------------------------------------------------------------------------------


def gemm(A, W, bias, R, Cbuf, M, N, K, lda, ldw, ldr, ldc, batch=1, sA=0, sW=0, sR=0, sC=0, oa=0, ow=0, orr=0, oc=0, act="none"):
    """hgl_gemm_f32 on flat float32 buffers at element offsets (R may be Cbuf: the residual then aliases the output)"""
    lib = _lib.load()
    _lib.check(lib.hgl_gemm_f32(_ptr(A, oa), _ptr(W, ow), _ptr(bias), _ptr(R, orr) if R is not None else None, _ptr(Cbuf, oc),
                                M, N, K, lda, ldw, ldr, ldc, batch, sA, sW, sR, sC, ops.ACT[act], _stream()), "hgl_gemm_f32")


def layernorm(x, w, b, y, rows, D, eps, ox=0, oy=0):
    """hgl_layernorm_f32 on flat float32 buffers at element offsets ox / oy (rows of D elements, dense)"""
    lib = _lib.load()
    _lib.check(lib.hgl_layernorm_f32(_ptr(x, ox), _ptr(w), _ptr(b), _ptr(y, oy), rows, D, float(eps), _stream()),
               "hgl_layernorm_f32")


def layernorm_reference(x, w, b, eps):
    """(x - mean) / sqrt(var + eps) * w + b over the last dim, in float64"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def activation64(z, act):
    """the four epilogue activations of hgl_gemm_f32 in float64 (include/hybridgl.h HGL_ACT_*)"""
    if act == "quickgelu":
        return z * torch.sigmoid(1.702 * z)
    if act == "gelu":
        return 0.5 * z * (1.0 + torch.special.erf(z / math.sqrt(2.0)))
    if act == "relu":
        return torch.clamp(z, min=0.0)
    assert act == "none", act
    return z


def gemm_reference(A, W, bias, R, M, N, K, lda, ldw, ldr, batch=1, sA=0, sW=0, sR=0, oa=0, ow=0, orr=0, act="none"):
    """act(A[b] W[b]^T + bias) + R[b] in float64 -> [batch, M, N] (read R BEFORE a call that overwrites it)"""
    a = view(A, oa, batch, M, lda, sA, K).double()
    w = view(W, ow, batch, N, ldw, sW, K).double()
    z = a @ w.transpose(-1, -2)
    if bias is not None:
        z = z + bias.double()
    z = activation64(z, act)
    if R is not None:
        z = z + view(R, orr, batch, M, ldr, sR, N).double()
    return z


def split_scale_log2(w):
    """the power-of-two pre-scale of a registered weight (ops.register_split_weight): max|w| * 2^s <= 2^14"""
    amax = float(np.abs(w).max())
    return 0 if amax == 0 else max(-24, min(24, 14 - math.ceil(math.log2(amax))))


def gemm_f16_reference(a, w, bias, res, act, rows=None):
    """float64 GEMM of the fp16-rounded operands (+ the fp32-accumulation error bound of each output): what the f16 mode's
    one-term kernels compute (numpy arrays; the activation rounded to fp16, the weight after its power-of-two pre-scale)"""
    s = split_scale_log2(w)
    a16 = a.astype(np.float16).astype(np.float64)
    w16 = (w.astype(np.float64) * 2.0 ** s).astype(np.float16).astype(np.float64)
    if rows is not None:
        a16 = a16[rows]
    acc = (a16 @ w16.T) * 2.0 ** -s
    mag = (np.abs(a16) @ np.abs(w16).T) * 2.0 ** -s
    K = a.shape[1]
    y = acc + (bias.astype(np.float64) if bias is not None else 0.0)
    # (|act'| <= 1.13 for GELU, 1.1 for QuickGELU, 1 for ReLU: the accumulation error passes through at most 1.2x)
    if act == "gelu":
        y = 0.5 * y * (1.0 + np.vectorize(math.erf)(y / math.sqrt(2.0)))
    elif act == "quickgelu":
        y = y / (1.0 + np.exp(-1.702 * y))
    elif act == "relu":
        y = np.maximum(y, 0.0)
    if res is not None:
        y = y + (res[rows] if rows is not None else res).astype(np.float64)
    # fp32 accumulation (K terms, each product exact) + the fp32 epilogue (scale, bias, activation, residual)
    bound = 1.2 * 2.0 * K * 2.0 ** -24 * mag + 8.0 * 2.0 ** -24 * (np.abs(acc) + np.abs(y) + 1.0)
    if act == "quickgelu":   # + the float evaluation of its exponential: 3e-6 relative (test_epilogue_activations_accuracy)
        bound = bound + 3e-6 * np.abs(y)
    return y, bound


# ---- which kernel ran --------------------------------------------------------------------------------------------------------


def kernel_key(name):
    """'attn_x3_kernel<80,0,4,3>' from a demangled ('... attn_x3_kernel<80, 0, 4, 3>(AttnArgs)') or an Itanium-mangled
    ('..._14attn_x3_kernelILi80ELi0ELi4ELi3EEEv...') kernel name; the bare name for non-templates; None for no match"""
    m = re.search(r"((?:attn|gemm|layernorm)_\w*?kernel)ILi(-?\d+)E((?:Li-?\d+E)*)E", name)
    if m:
        args = [m.group(2)] + re.findall(r"Li(-?\d+)E", m.group(3))
        return f"{m.group(1)}<{','.join(args)}>"
    m = re.search(r"((?:attn|gemm|layernorm)_\w*?kernel)(<[^()]*>)?", name)
    if not m:
        return None
    return m.group(1) + (m.group(2).replace(" ", "") if m.group(2) else "")


def launched_kernels(fn):
    """the GPU kernels fn() launches, in launch order (torch.profiler: Kineto's device activity, which lists the dispatches of
    the whole process -- libhybridgl.so's included); names as kernel_key gives them (the raw name when it finds none)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name for e in evs if not e.name.lower().startswith(("memcpy", "memset"))]
    return [kernel_key(n) or n for n in names]


def rle_kernels(fn):
    """launched_kernels(fn) for the kernels of csrc/rle.hip: [(function name, first template argument or None)] in launch order, from
    a demangled ('rle_rows_kernel<4>(...)') or an Itanium-mangled ('15rle_rows_kernelILi4EEEv...') name; any other kernel
    keeps its raw name"""
    out = []
    for n in launched_kernels(fn):
        m = re.search(r"(rle_[a-z]+_kernel)(?:<(\w+)[,>]|IL[ib](\d+)E)?", n)
        out.append((m.group(1), m.group(2) or m.group(3)) if m else (n, None))
    return out


def nms_kernels(fn):
    """launched_kernels(fn) for the kernels of csrc/sam_nms.hip: [(function name, template argument or None)] in launch order,
    from a demangled ('nms_segments_kernel<true>(...)') or an Itanium-mangled ('19nms_segments_kernelILb1EEEv...') name, the
    argument as the mangled form spells it ('1' for true); any other kernel keeps its raw name"""
    out = []
    for n in launched_kernels(fn):
        m = re.search(r"(nms_(?:[a-z]+_)?kernel)(?:<(\w+)[,>]|IL[ib](\d+)E)?", n)
        arg = m and (m.group(2) or m.group(3))
        out.append((m.group(1), {"true": "1", "false": "0"}.get(arg, arg)) if m else (n, None))
    return out
