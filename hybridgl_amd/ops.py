"""Torch-tensor front ends of the C-ABI operators (device memory + stream plumbing only).

Every function validates device/dtype/contiguity, then passes raw pointers to
libhybridgl.so.  Nothing here computes: a missing library or a CPU tensor raises.
"""
import ctypes as C
from itertools import accumulate, repeat
from math import prod

import torch

from . import _lib
from ._lib import check

ACT = {"none": 0, "quickgelu": 1, "gelu": 2, "relu": 3}
MASK = {"none": 0, "causal": 1, "cls_keep": 2}
DIRFLAG = {"none": 0, "left": 1, "right": 2, "middle": 3}
# utils.py:240-268 relation words; anything else falls through to "none" semantics there
RELAWORD = {"none": 0, "left": 1, "right": 2, "up": 3, "down": 4, "big": 5, "small": 6, "within": 7}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise _lib.HybridGLError(f"{name}: tensor must live on the GPU (no CPU path exists)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _u8(t, name):
    """bool / uint8 mask tensor -> pointer (torch.bool is one byte, 0/1)."""
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return _dev(t, torch.uint8, name), t


def gemm(a, w, bias=None, residual=None, act="none", out=None):
    """out = act(a @ w.T + bias) + residual   (torch.nn.functional.linear semantics)."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.hgl_gemm_f32(_dev(a, torch.float32, "a"), _dev(w, torch.float32, "w"),
                           _dev(bias, torch.float32, "bias") if bias is not None else None,
                           _dev(residual, torch.float32, "residual") if residual is not None else None,
                           _dev(out, torch.float32, "out"), M, N, K, K, K, N, N, 1, 0, 0, 0, 0,
                           ACT[act], _stream()), "hgl_gemm_f32")
    return out


_split_cache = {}  # fp32 weight data_ptr -> (weight, hi, lo): keeps the registered halves alive while a model owns them


def register_split_weight(w, scale_log2=None):
    """Register the fp16 hi/lo split of a [N,K] fp32 weight for the HGL_PREC_F16X3 GEMM path.
    The power-of-two scale puts max|w| at <= 2^14 (lo halves stay normal fp16); scale_log2=0 registers the UNSCALED split (the
    values a kernel's own hgl_split_hi_lo gives: SAM's rel-pos tables for the windowed attention).  Returns the registry key;
    the owner hands its keys to release_split_weights when it dies (the models do that through weakref.finalize)."""
    import math
    lib = _lib.load()
    key = w.data_ptr()
    if key in _split_cache:
        return key
    N, K = w.shape
    amax = float(w.abs().max().item())
    s = 0 if amax == 0 else max(-24, min(24, 14 - math.ceil(math.log2(amax))))
    if scale_log2 is not None:
        s = int(scale_log2)
    hi = torch.empty((N, K), dtype=torch.float16, device=w.device)
    lo = torch.empty((N, K), dtype=torch.float16, device=w.device)
    check(lib.hgl_register_split_weight(_dev(w, torch.float32, "w"), N, K, s, hi.data_ptr(), lo.data_ptr(),
                                        _stream()), "hgl_register_split_weight")
    _split_cache[key] = (w, hi, lo)
    return key


def release_split_weights(keys):
    """Drop the registered splits of `keys` (library registry + the hi/lo tensors): called when their model dies."""
    try:
        lib = _lib.load()
    except Exception:   # interpreter shutdown
        return
    for key in keys:
        if _split_cache.pop(key, None) is not None:
            lib.hgl_unregister_split_weight(key)


def split_weight_keys_since(before):
    """keys registered after the snapshot `before` (= set(_split_cache)): what a constructor has added"""
    return [k for k in _split_cache if k not in before]


PRECISIONS = {"f32": 0, "f16x3": 1, "f16": 2}


def default_precision():
    """'f16x3' unless HYBRIDGL_PRECISION says otherwise: 'f32' and 'f16x3' meet the parity bar (tests run both); 'f16' is
    the opt-in half-precision mode (fp16 operands, fp32 accumulation)."""
    import os
    mode = os.environ.get("HYBRIDGL_PRECISION", "f16x3")
    if mode not in PRECISIONS:
        raise ValueError(f"HYBRIDGL_PRECISION={mode!r}: expected one of {sorted(PRECISIONS)}")
    return mode


def split_mode(mode):
    """True for the modes that keep fp16 hi | lo planes of weights and activations ('f16x3' and 'f16')"""
    return mode in ("f16x3", "f16")


_precision_now = None
_precision_forced = None


def effective_precision(mode):
    """the precision a model that carries `mode` runs in right now: the forced one inside forced_precision, else its own
    (use_precision's rule; no Python-side choice of buffers or entries depends on the mode, the library reads its own)"""
    return mode if _precision_forced is None else _precision_forced


class forced_precision:
    """Context manager: while active, use_precision(m) sets `mode` whatever m is, so every model of the process runs in
    `mode` whatever it was built in (the weights' fp16 splits stay registered and are simply not read in 'f32').  On exit the
    library is back in the mode it was in on entry, so a bare ops.* call behind the context runs as one in front of it did; the
    next model re-asserts its own as always.  Not re-entrant across threads: the library keeps ONE current mode."""

    def __init__(self, mode):
        if mode not in PRECISIONS:
            raise ValueError(f"precision {mode!r}: expected one of {sorted(PRECISIONS)}")
        self.mode = mode

    def __enter__(self):
        global _precision_forced
        self._outer, self._was = _precision_forced, _precision_now
        _precision_forced = self.mode
        use_precision(self.mode)
        return self

    def __exit__(self, *exc):
        global _precision_forced
        _precision_forced = self._outer
        back = self._outer if self._outer is not None else self._was
        if back is not None:
            use_precision(back)
        return False


def set_precision(mode):
    """'f32' (exact fp32 MFMA), 'f16x3' (split-fp16 MFMA, fp32-class accuracy) or 'f16' (fp16 operands, one MFMA per
    product, fp32 accumulation: opt-in, not fp32-class).  The library keeps ONE current mode;
    every model carries its own and re-asserts it on entry (use_precision), so models of different precision can live
    in one process."""
    global _precision_now
    if mode not in PRECISIONS:
        raise ValueError(f"precision {mode!r}: expected one of {sorted(PRECISIONS)}")
    check(_lib.load().hgl_set_precision(PRECISIONS[mode]), "hgl_set_precision")
    _precision_now = mode


def use_precision(mode):
    """make `mode` the library's current precision if it is not already (called on entry by every model method); inside
    forced_precision the forced mode takes its place"""
    mode = effective_precision(mode)
    if mode != _precision_now:
        set_precision(mode)


def split_overflow_count(reset=True, sync=True):
    """Number of GPU threads of the f16x3 path that met an activation beyond the fp16 range since the last reset
    (hgl_split_overflow_count).  Synchronises the device first unless sync=False."""
    if sync:
        torch.cuda.synchronize()
    n = C.c_ulonglong(0)
    check(_lib.load().hgl_split_overflow_count(1 if reset else 0, C.byref(n)), "hgl_split_overflow_count")
    return int(n.value)


def split_overflow_peek(buf):
    """Enqueue, on the current stream, a copy of the two overflow counters into `buf` (pinned int32 [2] host tensor): no
    wait, no reset.  Read buf after an event recorded behind this call has completed."""
    assert buf.is_pinned() and buf.dtype == torch.int32 and buf.numel() >= 2
    check(_lib.load().hgl_split_overflow_peek_async(buf.data_ptr(), _stream()), "hgl_split_overflow_peek_async")


def split_overflow_snapshot(buf):
    """Enqueue, on the current stream, a copy of ALL THREE overflow counters (GEMM, attention, SAM decoder) into `buf` (pinned
    int32 [3] host tensor): no wait, no reset (hgl_split_overflow_snapshot_async).  Their sum is split_overflow_count(reset=
    False) as of this point of the stream.  Read buf after an event recorded behind this call has completed."""
    assert buf.is_pinned() and buf.dtype == torch.int32 and buf.numel() >= 3
    check(_lib.load().hgl_split_overflow_snapshot_async(buf.data_ptr(), _stream()), "hgl_split_overflow_snapshot_async")


class SplitOverflow(_lib.HybridGLError):
    """an activation left the fp16 range in f16x3 or f16 mode: the results since the last clean check contain inf / NaN"""


def check_split_overflow():
    """raise if the f16x3 / f16 path met a value it cannot represent (the results since the last check then contain inf /
    NaN); the cure is HYBRIDGL_PRECISION=f32"""
    n = split_overflow_count(reset=True)
    if n:
        raise SplitOverflow(f"activations exceeded the fp16 range (|x| > 65504) in f16x3 / f16 mode ({n} GPU threads saw one): "
                            "the results contain inf / NaN; rerun with HYBRIDGL_PRECISION=f32 (or precision='f32')")


X3_KERNELS = {"auto": -1, "v1": 0, "P": 1}


def select_x3_kernel(kind="auto"):
    """Pins the tiling of the f16x3 GEMM ('auto' = cost model; all tilings are bit-identical)."""
    check(_lib.load().hgl_gemm_f16x3_select(X3_KERNELS[kind]), "hgl_gemm_f16x3_select")


def gemm_f16x3(a, w, bias=None, residual=None, act="none", out=None, balanced=False):
    """gemm() through the split-fp16 matrix-core path (registers w on first use).  balanced=True: the row-balanced launch of
    the model code's residual GEMMs (whole rounds of the persistent tiling + a split-K tail; hgl_gemm_f16x3 with scratch for
    the tail's partial sums)."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    register_split_weight(w)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    # the tail is at most half a round of 256 x 256 tiles in k K slices with k x tiles <= CUs: <= 256 slice-tiles of 256 KiB
    extra = (2 * 256 * 256 * 256 * 4 + 4096) if balanced else 0
    need = (M * K * 4 + 255) // 256 * 256 + extra      # the SIZE handed over selects the launch, not the (grow-only) buffer's
    ws = workspace(need, a.device, "gemm_f16x3")
    check(lib.hgl_gemm_f16x3(_dev(a, torch.float32, "a"), _dev(w, torch.float32, "w"),
                             _dev(bias, torch.float32, "bias") if bias is not None else None,
                             _dev(residual, torch.float32, "residual") if residual is not None else None,
                             _dev(out, torch.float32, "out"), M, N, K, ACT[act], ws.data_ptr(), need,
                             _stream()), "hgl_gemm_f16x3")
    return out


def layernorm(x, w, b, eps=1e-5):
    lib = _lib.load()
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    check(lib.hgl_layernorm_f32(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"),
                                _dev(b, torch.float32, "b"), _dev(y, torch.float32, "y"), rows, D,
                                float(eps), _stream()), "hgl_layernorm_f32")
    return y


def attention(q, k, v, heads, scale=None, mask="none", keep=None, keep_b0=0, keep_n=0,
              rel_h=None, rel_w=None):
    """q: [B,Sq,H*hd], k,v: [B,Sk,H*hd] contiguous -> [B,Sq,H*hd]."""
    lib = _lib.load()
    B, Sq, Dm = q.shape
    Sk = k.shape[1]
    hd = Dm // heads
    if scale is None:
        scale = hd ** -0.5
    out = torch.empty_like(q)
    kp = None
    if keep is not None:
        kp, keep = _u8(keep, "keep")
    kh = kw = 0
    if rel_h is not None:
        kh, kw = rel_h.shape[-1], rel_w.shape[-1]
    check(lib.hgl_attention_f32(_dev(q, torch.float32, "q"), _dev(k, torch.float32, "k"),
                                _dev(v, torch.float32, "v"), _dev(out, torch.float32, "out"),
                                B, heads, Sq, Sk, hd, Dm, Dm, Dm, Dm,
                                Sq * Dm, Sk * Dm, Sk * Dm, Sq * Dm, float(scale), MASK[mask], kp,
                                keep_b0, keep_n,
                                _dev(rel_h, torch.float32, "rel_h") if rel_h is not None else None,
                                _dev(rel_w, torch.float32, "rel_w") if rel_w is not None else None,
                                kh, kw, _stream()), "hgl_attention_f32")
    return out


def attention_presplit(qkv, heads, scale=None, mask="none", keep=None, keep_b0=0, keep_n=0):
    """qkv: [B,S,3*H*hd] fp32 contiguous (the in-projection output, q | k | v) -> [B,S,H*hd] through the kernels that take
    the fp16 hi / lo planes (csrc/attention_ps.hip); split-fp16 mode, hd in {64, 80}."""
    lib = _lib.load()
    B, S, D3 = qkv.shape
    Dm = D3 // 3
    hd = Dm // heads
    if scale is None:
        scale = hd ** -0.5
    out = torch.empty((B, S, Dm), dtype=torch.float32, device=qkv.device)
    scratch = torch.empty(B * S * D3, dtype=torch.float32, device=qkv.device)
    kp = None
    if keep is not None:
        kp, keep = _u8(keep, "keep")
    check(lib.hgl_attention_presplit_f32(_dev(qkv, torch.float32, "qkv"), D3, B, heads, S, hd, _dev(out, torch.float32, "out"), Dm,
                                         float(scale), MASK[mask], kp, keep_b0, keep_n, scratch.data_ptr(), scratch.numel() * 4,
                                         _stream()), "hgl_attention_presplit_f32")
    return out


def sam_relpos_tables(q, rel_pos_h, rel_pos_w, B, heads, size, rel_h=None, rel_w=None):
    """The rel-pos producer of the SAM encoder's attention (hgl_sam_relpos_tables): rel_h, rel_w [B*heads, size*size, size]
    from the UNSCALED q of B windows of size x size tokens.  q: fp32 [B*size*size, ldq], or the pair (q_hi, q_lo) of fp16 planes
    of that shape (f16x3 mode); the heads' q are the first heads*hd columns of a row.  rel_pos_h / rel_pos_w: [2*size-1, hd].
    The library picks the kernels as the encoder does."""
    lib = _lib.load()
    S = size * size
    hd = rel_pos_h.shape[1]
    planes = isinstance(q, (tuple, list))
    q0 = q[0] if planes else q
    assert q0.shape[0] == B * S and tuple(rel_pos_h.shape) == tuple(rel_pos_w.shape) == (2 * size - 1, hd)
    if rel_h is None:
        rel_h = torch.empty((B * heads, S, size), dtype=torch.float32, device=q0.device)
    if rel_w is None:
        rel_w = torch.empty((B * heads, S, size), dtype=torch.float32, device=q0.device)
    assert tuple(rel_h.shape) == tuple(rel_w.shape) == (B * heads, S, size)
    need = lib.hgl_sam_relpos_tables_workspace_bytes(B, heads, S, size)
    ws = workspace(need, q0.device, "sam_relpos")
    check(lib.hgl_sam_relpos_tables(None if planes else _dev(q, torch.float32, "q"),
                                    _dev(q[0], torch.float16, "q_hi") if planes else None,
                                    _dev(q[1], torch.float16, "q_lo") if planes else None, q0.shape[1], B, heads, S, size, hd,
                                    _dev(rel_pos_h, torch.float32, "rel_pos_h"), _dev(rel_pos_w, torch.float32, "rel_pos_w"),
                                    _dev(rel_h, torch.float32, "rel_h"), _dev(rel_w, torch.float32, "rel_w"), ws.data_ptr(), need,
                                    _stream()), "hgl_sam_relpos_tables")
    return rel_h, rel_w


def mask_resize(masks, g):
    """TF.resize(masks.float(), (g,g)) of model/backbone.py:160 -> [N, g*g] fp32."""
    lib = _lib.load()
    N, H, W = masks.shape
    mp, masks = _u8(masks, "masks")
    pm = torch.empty((N, g * g), dtype=torch.float32, device=masks.device)
    check(lib.hgl_mask_resize(mp, N, H, W, g, _dev(pm, torch.float32, "pm"), _stream()), "hgl_mask_resize")
    return pm


def calculate_score(img, txt, logit_scale):
    lib = _lib.load()
    N, E = img.shape
    T = txt.shape[0]
    out = torch.empty((N, T), dtype=torch.float32, device=img.device)
    check(lib.hgl_calculate_score(_dev(img, torch.float32, "img"), _dev(txt, torch.float32, "txt"), N, T, E,
                                  float(logit_scale), _dev(out, torch.float32, "out"), _stream()),
          "hgl_calculate_score")
    return out


_ws_cache = {}


def workspace(nbytes, device, tag="default"):
    """Grow-only device workspace (allocated outside the timed/hot path, reused).  One buffer per (tag, stream): the
    stages of the evaluation loop run on their own streams, and a buffer that grows (a larger image, more proposals)
    is replaced while kernels of ANOTHER stream could still be using the old one -- the caching allocator only orders
    reuse within the allocating stream."""
    key = (str(device), tag, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def coherence_scores(imgattn, masks, dirflag="none", black=1.8):
    """Hybridgl_main.py:201-223 for all masks at once -> [N] fp32."""
    lib = _lib.load()
    N, H, W = masks.shape
    assert imgattn.shape == (H, W)
    mp, masks = _u8(masks, "masks")
    need = lib.hgl_coherence_workspace_bytes(N, H, W)
    ws = workspace(need, masks.device, "coherence")
    out = torch.empty((N,), dtype=torch.float32, device=masks.device)
    check(lib.hgl_coherence_scores(_dev(imgattn, torch.float32, "imgattn"), mp, N, H, W,
                                   DIRFLAG.get(dirflag, 0), float(black), _dev(out, torch.float32, "out"),
                                   ws.data_ptr(), ws.numel(), _stream()), "hgl_coherence_scores")
    return out


def iou_counts(pred, gt):
    """Compute_IoU (utils.py:365-384) counts: tensor([I, U]) int64 on device."""
    lib = _lib.load()
    pp, pred = _u8(pred, "pred")
    gp, gt = _u8(gt, "gt")
    assert pred.numel() == gt.numel()
    out = torch.empty((2,), dtype=torch.int64, device=pred.device)
    check(lib.hgl_iou(pp, gp, pred.numel(), out.data_ptr(), _stream()), "hgl_iou")
    return out


def iou_select(masks, idx, which, gt):
    """Compute_IoU(masks[idx[which]], gt) with the index resolved on the device -> tensor([I,U])."""
    lib = _lib.load()
    mp, masks = _u8(masks, "masks")
    gp, gt = _u8(gt, "gt")
    HW = gt.numel()
    assert masks.numel() % HW == 0
    out = torch.empty((2,), dtype=torch.int64, device=masks.device)
    check(lib.hgl_iou_select(mp, _dev(idx, torch.int32, "idx"), int(which), gp, HW, out.data_ptr(), _stream()),
          "hgl_iou_select")
    return out


def rle_slot_words(H, W):
    """the slot size at which hgl_rle_encode_device never loses a mask: the words of its bit plane, ceil(H*W/32)"""
    return (int(H) * int(W) + 31) // 32


# The int32 blocks the RLE entries hand out as views of ONE flat buffer: name -> the shapes of its parts, in memory order and
# without a gap, from (S, slot_words, G, C, Sb).  The only statement of these layouts: rle_block and rle_block_words read it.
RLE_BLOCKS = {
    "set": lambda S, sw, G, C, Sb: ((S, 4), (S, sw)),                       # table | slots: rle_encode, rle_pack, rle_from_strings
    "status": lambda S, sw, G, C, Sb: ((S, 4), (S, sw), (S, 4)),            # table | slots | status: rle_from_polygons, rle_merge
    "clean": lambda S, sw, G, C, Sb: ((S, 4), (S, sw), (S, 4), (S, 4)),     # table | slots | boxes | result: rle_remove_small_regions
    "select": lambda S, sw, G, C, Sb: ((S, 4), (S, sw), (C, S)),            # table | slots | cols: rle_select's `out`
    "group": lambda S, sw, G, C, Sb: ((S, 4), (S, sw), (2, S), (C * S,)),   # table | slots | iou, stability bits | area bits, C = 0 / 1: a staged group of proposals.py
    "back": lambda S, sw, G, C, Sb: ((S,), (G,)),                           # out_src | out_n: rle_select's `back`
    "nms": lambda S, sw, G, C, Sb: ((S,), (S, 4), (G,)),                    # out_idx | result | out_n: rle_nms
    "aux": lambda S, sw, G, C, Sb: ((S, 4), (S, 4)),                        # boxes | status: rle_decode_group
    "match": lambda S, sw, G, C, Sb: ((S, 4), (Sb, 4)),                     # match_a | match_b: rle_match
}


def rle_block_ends(name, S, slot_words=0, G=0, C=0, Sb=0):
    """where every part of block `name` (RLE_BLOCKS) ends, in int32 elements from the start of the block"""
    return list(accumulate(map(prod, RLE_BLOCKS[name](S, slot_words, G, C, Sb))))


def rle_block(name, flat, S, slot_words=0, G=0, C=0, Sb=0):
    """the parts of block `name` as views of the flat int32 buffer that begins with it: device tensor, host tensor or numpy
    array alike"""
    parts, a = [], 0
    for shape in RLE_BLOCKS[name](S, slot_words, G, C, Sb):
        b = a + prod(shape)
        parts.append(flat[a:b].reshape(shape))
        a = b
    return parts


def rle_block_words(name, S, slot_words=0, G=0, C=0, Sb=0):
    """the int32 elements of block `name`: what its flat buffer holds"""
    return rle_block_ends(name, S, slot_words, G, C, Sb)[-1]


def rle_split(flat, S, slot_words):
    """(slots [S, slot_words], table [S, 4]) as views of the flat int32 buffer rle_encode fills (device tensor, host tensor
    or numpy array alike): the table first, then the slots"""
    table, slots = rle_block("set", flat, S, slot_words)
    return slots, table


def _out(buf, numel, dtype, device, name):
    """The one check of a buffer a caller lends (`out`, `aux`, `back`, `status`): a fresh one when buf is None, else buf itself,
    both flat.  ValueError unless buf is a contiguous `dtype` tensor of exactly `numel` elements on `device`: its pointer goes
    to a kernel as it is."""
    if buf is None:
        return torch.empty(numel, dtype=dtype, device=device)
    if buf.numel() != numel or buf.dtype != dtype or not buf.is_contiguous() or buf.device != device:
        raise ValueError(f"{name}: expected {numel} {str(dtype)[6:]} elements, contiguous, on {device}; got {tuple(buf.shape)} "
                         f"{str(buf.dtype)[6:]} on {buf.device}" + ("" if buf.is_contiguous() else ", strided"))
    return buf.view(-1)


def _ptr(t):
    """where a view begins in its buffer -- data_ptr(), except that torch gives 0 for a view without an element and the library
    wants the slots named also where slot_words is 0"""
    return t.data_ptr() or t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def _rle_ws(device, size_fn, *args):
    """(pointer, bytes) of the RLE workspace at the size the library's size_fn(*args) asks for"""
    ws = workspace(size_fn(*args), device, "rle")
    return ws.data_ptr(), ws.numel()


def rle_encode(masks, sel=None, slot_words=None, out=None):
    """Column-major run lengths (utils/amg.py:107-136) of masks[sel] on the device: hgl_rle_encode_device on the current
    stream, no synchronisation.  masks [N,H,W] bool / uint8; sel: integer device tensor [S] (converted on the device) or
    None for every mask; slot_words: int32 words per entry (default ceil(H*W/32): nothing is ever lost).
    Returns (slots [S, slot_words] int32, table [S,4] int32 = n_counts, form, area, 0), two views of one flat buffer
    (`out`: a contiguous int32 device tensor of S * (4 + slot_words) elements to use for it); form 0: the slot holds the
    counts, 1: the column-major bit plane, 2: neither fits, 3: index out of range (include/hybridgl.h).  The words are
    unsigned: view them as uint32 on the host."""
    lib = _lib.load()
    N, H, W = masks.shape
    mp, masks = _u8(masks, "masks")
    sp = None
    S = N
    if sel is not None:
        if not sel.is_cuda or sel.is_floating_point() or sel.dtype == torch.bool:
            raise TypeError("sel: expected an integer device tensor")
        sel = sel.reshape(-1).to(torch.int64).contiguous()
        sp, S = sel.data_ptr(), int(sel.numel())
    slot_words = rle_slot_words(H, W) if slot_words is None else int(slot_words)
    out = _out(out, rle_block_words("set", S, slot_words), torch.int32, masks.device, "out")
    slots, table = rle_split(out, S, slot_words)
    if S == 0:
        return slots, table
    check(lib.hgl_rle_encode_device(mp, N, H, W, sp, S, _ptr(slots), slot_words, table.data_ptr(),
                                    *_rle_ws(masks.device, lib.hgl_rle_encode_workspace_bytes, S, H, W), _stream()),
          "hgl_rle_encode_device")
    return slots, table


def rle_pack(counts_list, H, W, slot_words=None, device=None):
    """Host run lengths -> what ops.rle_encode would hand out for them: (slots [S, slot_words] int32, table [S,4] int32) on
    the device, every row in form 0.  counts_list: ragged lists / arrays of uint32 counts (column-major runs of H x W masks,
    zeros first); slot_words: default the longest list (at least 1), so runs cross the bus and not ceil(H*W/32) words per
    mask; a list longer than an explicit slot_words raises ValueError.  One pinned staging buffer, one host -> device copy
    on the current stream; table columns 2 and 3 are 0 (the decoder does not read them)."""
    import numpy as np
    if int(H) <= 0 or int(W) <= 0:
        raise ValueError(f"rle_pack: bad size {H} x {W}")
    rows = [np.asarray(c, dtype=np.uint32).reshape(-1) for c in counts_list]
    S = len(rows)
    longest = max([len(r) for r in rows], default=0)
    if slot_words is None:
        slot_words = max(longest, 1)
    slot_words = int(slot_words)
    if longest > slot_words:
        k = next(i for i, r in enumerate(rows) if len(r) > slot_words)
        raise ValueError(f"rle_pack: entry {k} has {len(rows[k])} counts, slot_words is {slot_words}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    stage = torch.zeros(rle_block_words("set", S, slot_words), dtype=torch.int32, pin_memory=True)
    slots, table = rle_split(stage.numpy(), S, slot_words)
    for i, r in enumerate(rows):
        table[i, 0] = len(r)
        slots[i, :len(r)] = r.view(np.int32)
    flat = stage.to(device, non_blocking=True)
    return rle_split(flat, S, slot_words)


RLE_STRING_CAP_PER_ENTRY = 4096      # the default room of rle_to_strings per entry, in bytes: a guess until tools/rle_bench.py --strings says otherwise


def rle_strings_split(flat, S, cap):
    """(bytes uint8 [cap], offsets int64 [S+1], status int32 [S]) as views of the flat uint8 buffer rle_to_strings fills (device
    tensor, host tensor or numpy array alike): the offsets first, then the status, then the bytes -- what a caller wants on the
    host is one stretch from the front"""
    S, cap = int(S), int(cap)
    a, b = 8 * (S + 1), 8 * (S + 1) + 4 * S
    if isinstance(flat, torch.Tensor):
        return flat[b:b + cap], flat[:a].view(torch.int64), flat[a:b].view(torch.int32)
    return flat[b:b + cap], flat[:a].view("int64"), flat[a:b].view("int32")


def rle_strings_bytes(S, cap):
    """the uint8 elements of the flat buffer of rle_to_strings for S entries and cap string bytes"""
    return 8 * (int(S) + 1) + 4 * int(S) + int(cap)


def rle_to_strings(slots, table, cap=None, out=None):
    """COCO's compressed strings (maskApi.c:203-216 rleToString) of an encoded set on the device: hgl_rle_to_strings_device on
    the current stream, no synchronisation.  slots / table: what rle_encode or rle_pack returns.  cap: the room for all strings
    together, default RLE_STRING_CAP_PER_ENTRY * S.  Returns (bytes uint8 [cap], offsets int64 [S+1], status int32 [S]), three
    views of one flat uint8 buffer (`out`: a contiguous uint8 device tensor of rle_strings_bytes(S, cap) elements to use for
    it; rle_strings_split takes it apart).  The strings lie back to back in entry order, entry s at offsets[s] .. offsets[s+1];
    the offsets are true also when cap is too small.  status 0: written; 1: the entry is a bit plane (form 1), finish it on the
    host; 2: no mask; 3: the string does not lie wholly inside cap and no byte of it was written (include/hybridgl.h)."""
    lib = _lib.load()
    sp, sw, tp, S = _rle_set(slots, table, "rle_to_strings")
    cap = RLE_STRING_CAP_PER_ENTRY * S if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"rle_to_strings: cap {cap}")
    out = _out(out, rle_strings_bytes(S, cap), torch.uint8, slots.device, "out")
    if out.data_ptr() % 8:
        raise ValueError("out: the buffer must be 8-byte aligned (it begins with the int64 offsets)")
    data, offsets, status = rle_strings_split(out, S, cap)
    check(lib.hgl_rle_to_strings_device(sp, sw, tp, S, data.data_ptr(), cap, offsets.data_ptr(), status.data_ptr(), _stream()),
          "hgl_rle_to_strings_device")
    return data, offsets, status


def rle_strings_pack(strings):
    """Compressed strings -> what one host -> device copy needs, on the host, vectorised over the concatenated bytes: returns
    (buf: a pinned uint8 tensor holding the int64 offsets [S+1] and then the bytes back to back; offsets: the int64 numpy view
    of its front; n_counts int64 [S]: the counts every string holds = its bytes that end a group).  strings: bytes or ASCII str.
    Raises ValueError naming the entry for a NUL byte (the host parser stops there, the device would not) or a non-ASCII str."""
    import numpy as np
    raw = []
    for k, s in enumerate(strings):
        if isinstance(s, str):
            try:
                s = s.encode("ascii")
            except UnicodeEncodeError:
                raise ValueError(f"rle_strings_pack: entry {k} is not ASCII") from None
        raw.append(bytes(s))
    S = len(raw)
    joined = b"".join(raw)
    buf = torch.empty(8 * (S + 1) + len(joined), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    host = buf.numpy()
    offsets = host[:8 * (S + 1)].view(np.int64)
    offsets[0] = 0
    np.cumsum(np.fromiter(map(len, raw), dtype=np.int64, count=S), out=offsets[1:])
    data = host[8 * (S + 1):]
    data[:] = np.frombuffer(joined, dtype=np.uint8)
    nul = np.flatnonzero(data == 0)
    if nul.size:
        raise ValueError(f"rle_strings_pack: entry {int(np.searchsorted(offsets, nul[0], side='right')) - 1} holds a NUL byte")
    ends = np.zeros(len(joined) + 1, dtype=np.int64)      # ends[p] = the bytes before p that end a group (csrc/rle_string.h: c & 32 == 0)
    np.cumsum(((data - np.uint8(48)) & np.uint8(32)) == 0, out=ends[1:])
    return buf, offsets, ends[offsets[1:]] - ends[offsets[:-1]]      # a difference of running sums: empty strings need no care


def rle_from_strings(data, offsets, S, slot_words, out=None, status=None):
    """The inverse of rle_to_strings on the device (maskApi.c:217-230 rleFrString without the decode):
    hgl_rle_from_strings_device on the current stream, no synchronisation.  data: uint8 device tensor of the strings back to
    back; offsets: int64 device tensor [S+1] (the two parts of rle_strings_pack's buffer once it is on the device).  Returns
    (slots [S, slot_words] int32, table [S,4] int32, status [S,4] int32 = code, n_counts, 0, 0): slots and table are the views
    of one flat buffer as rle_encode lays it out (`out`: S * (4 + slot_words) int32 elements), every accepted row in form 0.
    code 0: read; 1: n_counts > slot_words (the true n_counts is in the status); 2: truncated; 3: a group of more than 7
    characters; 4: broken offsets -- the rows of codes 1 to 4 say "no mask" to every decoder (include/hybridgl.h).  `status`: a
    contiguous int32 device tensor [S,4] to use for it (a stretch of a buffer that leaves in one read-back)."""
    lib = _lib.load()
    S, slot_words = int(S), int(slot_words)
    if offsets.numel() != S + 1:
        raise ValueError(f"rle_from_strings: {S} entries need {S + 1} offsets, got {offsets.numel()}")
    slots, table = rle_split(_out(out, rle_block_words("set", S, slot_words), torch.int32, data.device, "out"), S, slot_words)
    status = _out(status, 4 * S, torch.int32, data.device, "status").view(S, 4)
    if S == 0:
        return slots, table, status
    check(lib.hgl_rle_from_strings_device(_dev(data, torch.uint8, "data") if data.numel() else None, int(data.numel()),
                                          _dev(offsets, torch.int64, "offsets"), S, _ptr(slots), slot_words, table.data_ptr(),
                                          status.data_ptr(), _stream()), "hgl_rle_from_strings_device")
    return slots, table, status


def _rle_set(slots, table, name):
    """(slots pointer, slot_words, table pointer, S) of one encoded set: int32 device tensors [S, slot_words] and [S, 4]"""
    if slots.dim() != 2 or table.dim() != 2 or table.shape[1] != 4 or table.shape[0] != slots.shape[0]:
        raise ValueError(f"{name}: expected slots [S, slot_words] and table [S, 4], got {tuple(slots.shape)} and {tuple(table.shape)}")
    return _dev(slots, torch.int32, name + " slots"), int(slots.shape[1]), _dev(table, torch.int32, name + " table"), int(slots.shape[0])


def rle_decode(slots, table, H, W, out=None):
    """The inverse of rle_encode on the device: hgl_rle_decode_device on the current stream, no synchronisation.  slots /
    table: what rle_encode or rle_pack returns (form 0: counts, form 1: the bit plane).  Returns (masks [S,H,W] uint8 0 / 1,
    status [S,4] int32 = code, area, 0, 0): code 0 = decoded, 1 = decoded but the counts do not sum to H*W (clipped as the
    host codec clips), 2 = the slot holds no mask (zeros) (include/hybridgl.h).  `out`: a contiguous uint8 device tensor of
    exactly S*H*W elements to decode into; every byte of it is written."""
    lib = _lib.load()
    H, W = int(H), int(W)
    sp, sw, tp, S = _rle_set(slots, table, "rle_decode")
    masks = _out(out, S * H * W, torch.uint8, slots.device, "out").view(S, H, W)
    status = torch.empty((S, 4), dtype=torch.int32, device=slots.device)
    if S == 0:
        return masks, status
    check(lib.hgl_rle_decode_device(sp, sw, tp, S, H, W, masks.data_ptr(), status.data_ptr(),
                                    *_rle_ws(slots.device, lib.hgl_rle_decode_workspace_bytes, S, H, W, sw), _stream()),
          "hgl_rle_decode_device")
    return masks, status


def _rle_rows(name, sizes, counts_a, counts_b=None, tail=None, running=False):
    """The [G, k] int64 image rows of the RLE group calls, for the rle_*_layout functions: H, W, the image's first entry in one
    or two sets (the running sums of counts_a and counts_b) and -- with `tail` -- one more column: tail(g, H, W, na, nb) is its
    value or, when `running`, what image g adds to a running offset, and the column is the offset before the image.  Returns
    (rows, the offset behind the last image).  One flat list and one array: a row costs what it cost in the five loops before."""
    import numpy as np
    G, two = len(sizes), counts_b is not None
    if len(counts_a) != G or (two and len(counts_b) != G):
        raise ValueError(f"{name}: {G} sizes, {len(counts_a)} and {len(counts_b)} counts" if two else
                         f"{name}: {G} sizes and {len(counts_a)} counts")
    flat, ea, eb, off = [], 0, 0, 0
    for g, ((H, W), na, nb) in enumerate(zip(sizes, counts_a, counts_b if two else repeat(0))):
        if int(na) < 0 or int(nb) < 0:
            raise ValueError(f"{name}: image {g} has {na} and {nb} entries" if two else f"{name}: image {g} has {na} entries")
        H, W, na, nb = int(H), int(W), int(na), int(nb)
        flat += (H, W, ea, eb) if two else (H, W, ea)
        if tail is not None:
            t = tail(g, H, W, na, nb)
            flat.append(off if running else t)
            off += t if running else 0
        ea += na
        eb += nb
    return np.array(flat, dtype=np.int64).reshape(G, 3 + two + (tail is not None)), off


def _rle_group(name, sets, layout, sizes, *counts, **limits):
    """The one check of the RLE group calls.  sets: per list of counts its (slots, table), or a number of entries where there
    is no set (yet); layout: the call's rle_*_layout function, whose _rle_rows refuses lengths that differ and a negative
    count.  Returns (per set: slots pointer, slot_words, table pointer, S), the image rows, the total behind them (0 where
    the layout has none), G.  ValueError for counts that do not sum to their set's entries."""
    two = sum(isinstance(s, tuple) for s in sets) == 2
    sets = [_rle_set(*s, name + " " + "ab"[k] if two else name) if isinstance(s, tuple) else (None, 0, None, int(s))
            for k, s in enumerate(sets)]
    rows = layout(sizes, *counts, **limits)
    images, total = rows if isinstance(rows, tuple) else (rows, 0)
    for (_, _, _, S), c in zip(sets, counts):
        if int(sum(int(n) for n in c)) != S:
            raise ValueError(f"{name}: counts sum to {sum(c)}, the set has {S} entries")
    return sets, images, total, len(images)


def rle_group_layout(sizes, counts):
    """(images [G,4] int64 = H, W, first entry, byte offset; total bytes) of a group decoded back to back: image g's
    counts[g] masks of sizes[g] = (H, W) follow those of image g-1 with no padding"""
    return _rle_rows("rle_group_layout", sizes, counts, None, lambda g, H, W, n, _: n * H * W, running=True)


def rle_decode_group(slots, table, sizes, counts, out=None, aux=None):
    """A whole group's proposals in one call (hgl_rle_decode_group_device on the current stream, no synchronisation): the
    S = sum(counts) entries of slots / table (what rle_encode or rle_pack returns) belong to G = len(sizes) <= 64 images,
    counts[g] consecutive entries of sizes[g] = (H, W) each; an image may own none.  Returns (masks: a list of G uint8 views
    [counts[g], H, W], values 0 / 1, packed back to back in one buffer; boxes [S,4] int32: inclusive XYXY of every mask as
    sam.mask_boxes gives it, derived from the runs; status [S,4] int32 as rle_decode).  `out`: a contiguous uint8 device
    tensor of exactly the packed size to decode into; every byte of it is written.  boxes and status are the two halves of
    ONE int32 buffer [2,S,4] (`aux`: such a contiguous device tensor to use for it), so a caller that wants both on the host
    copies one tensor.  The number of launches depends neither on G nor on the sizes."""
    lib = _lib.load()
    ((sp, sw, tp, S),), images, total, G = _rle_group("rle_decode_group", [(slots, table)], rle_group_layout, sizes, counts)
    flat = _out(out, total, torch.uint8, slots.device, "out")
    boxes, status = rle_block("aux", _out(aux, rle_block_words("aux", S), torch.int32, slots.device, "aux"), S)
    masks = [flat[int(o):int(o) + int(n) * int(H) * int(W)].view(int(n), int(H), int(W))
             for (H, W, _, o), n in zip(images, counts)]
    if S == 0:
        return masks, boxes, status
    check(lib.hgl_rle_decode_group_device(sp, sw, tp, S, images.ctypes.data, G, flat.data_ptr(), total, boxes.data_ptr(), status.data_ptr(),
                                          *_rle_ws(slots.device, lib.hgl_rle_decode_group_workspace_bytes, S, sw), _stream()),
          "hgl_rle_decode_group_device")
    return masks, boxes, status


def rle_iou(slots_a, table_a, slots_b, table_b, H, W):
    """(|A & B|, |A | B|) of entry s of one encoded set against entry s of another, int64 [S,2] on the device, computed on
    bit planes (hgl_rle_iou_device; no mask is expanded to bytes).  (-1, -1) where either slot holds no mask."""
    lib = _lib.load()
    H, W = int(H), int(W)
    ap, asw, atp, S = _rle_set(slots_a, table_a, "rle_iou a")
    bp, bsw, btp, Sb = _rle_set(slots_b, table_b, "rle_iou b")
    if S != Sb:
        raise ValueError(f"rle_iou: the sets have {S} and {Sb} entries")
    iu = torch.empty((S, 2), dtype=torch.int64, device=slots_a.device)
    if S == 0:
        return iu
    check(lib.hgl_rle_iou_device(ap, asw, atp, bp, bsw, btp, S, H, W, iu.data_ptr(),
                                 *_rle_ws(slots_a.device, lib.hgl_rle_iou_workspace_bytes, S, H, W, asw, bsw), _stream()),
          "hgl_rle_iou_device")
    return iu


def rle_match_layout(sizes, counts_a, counts_b):
    """(images [G,5] int64 = H, W, first A entry, first B entry, element offset; total elements) of a group's [na, nb] matrices
    packed back to back"""
    return _rle_rows("rle_match_layout", sizes, counts_a, counts_b, lambda g, H, W, na, nb: na * nb, running=True)


def rle_match(slots_a, table_a, slots_b, table_b, sizes, counts_a, counts_b, crowd_b=None, matrix=True):
    """Every mask of set A against every mask of set B, image by image (hgl_rle_match_device on the current stream, no
    synchronisation): the entries of either set (what rle_encode or rle_pack returns) belong to G = len(sizes) <= 64 images,
    counts_a[g] / counts_b[g] consecutive entries of sizes[g] = (H, W); an image may own none on either side.  Returns
    (inter: a list of G int32 views [na_g, nb_g] of one buffer, |a & b| of every pair, -1 in the row / column of an entry that
    holds no mask -- or None with matrix=False; match_a [Sa,4] int32 = (code, area, best, I_best); match_b [Sb,4] likewise).
    best: the index within the image's other set of the partner with the largest I / D, D = area(a) where crowd_b[b] is set
    and the union elsewhere, compared exactly, the lowest index on a tie, -1 when nothing intersects (include/hybridgl.h).
    crowd_b: bool / uint8 device tensor [Sb] or None.  No mask becomes pixels."""
    lib = _lib.load()
    ((ap, asw, atp, Sa), (bp, bsw, btp, Sb)), images, total, G = _rle_group(
        "rle_match", [(slots_a, table_a), (slots_b, table_b)], rle_match_layout, sizes, counts_a, counts_b)
    if slots_a.device != slots_b.device:
        raise ValueError("rle_match: the two sets live on different devices")
    dev = slots_a.device
    cp = None
    if crowd_b is not None:
        if crowd_b.numel() != Sb:
            raise ValueError(f"crowd_b: expected {Sb} flags, got {crowd_b.numel()}")
        cp, crowd_b = _u8(crowd_b, "crowd_b")
    match_a, match_b = rle_block("match", torch.empty(rle_block_words("match", Sa, Sb=Sb), dtype=torch.int32, device=dev), Sa, Sb=Sb)
    flat = torch.empty(total, dtype=torch.int32, device=dev) if matrix else None
    inter = [flat[int(o):int(o) + int(na) * int(nb)].view(int(na), int(nb))
             for (_, _, _, _, o), na, nb in zip(images, counts_a, counts_b)] if matrix else None
    if Sa + Sb == 0:
        return inter, match_a, match_b
    check(lib.hgl_rle_match_device(ap, asw, atp, Sa, bp, bsw, btp, Sb, images.ctypes.data, G, cp,
                                   flat.data_ptr() if matrix else None, total, match_a.data_ptr(), match_b.data_ptr(),
                                   *_rle_ws(dev, lib.hgl_rle_match_workspace_bytes, images.ctypes.data, G, Sa, asw, Sb, bsw, int(matrix)),
                                   _stream()), "hgl_rle_match_device")
    return inter, match_a, match_b


NMS_METRIC = {"iou": 0, "containment": 1}


def rle_nms_layout(sizes, counts):
    """images [G,3] int64 = (H, W, first entry) of a mask NMS, a clean-up or a rasterisation over G images: image g owns
    counts[g] consecutive entries of sizes[g] = (H, W)"""
    return _rle_rows("rle_nms_layout", sizes, counts)[0]


rle_clean_layout = rle_nms_layout


def rle_nms(slots, table, sizes, counts, scores=None, thr=0.7, metric="iou", out=None):
    """Greedy suppression by mask overlap inside one encoded set, image by image (hgl_rle_nms_device on the current stream, no
    synchronisation): the S entries of slots / table (what rle_encode or rle_pack returns) belong to G = len(sizes) <= 64
    images, counts[g] <= 4096 consecutive entries of sizes[g] = (H, W); an image may own none.  scores: float device tensor [S]
    (the walk takes the box NMS's order: descending score, the index breaks ties, a NaN first) or None for the given order,
    which is rleNms's.  An entry is kept iff no kept entry before it has ratio > thr with it; metric "iou": I / union,
    "containment": I / the smaller area; an empty mask never suppresses and is never suppressed.
    Returns (out_idx [S] int32: from image g's first entry on, its kept entries in walk order as indices into its list; out_n
    [G] int32: how many; result [S,4] int32 = code, area, rank, by: the entry's position in the walk and the index of the kept
    entry of lowest rank that suppressed it, -1 for a kept one and for code 2).  No mask becomes pixels.  The three are views of
    ONE int32 buffer, out_idx | result | out_n (`out`: a contiguous int32 device tensor of 5 S + G elements to use for it)."""
    lib = _lib.load()
    if metric not in NMS_METRIC:
        raise ValueError(f"rle_nms: metric {metric!r} (one of {sorted(NMS_METRIC)})")
    thr = float(thr)
    if thr != thr:
        raise ValueError("rle_nms: the threshold is NaN")
    ((sp, sw, tp, S),), images, _, G = _rle_group("rle_nms", [(slots, table)], rle_nms_layout, sizes, counts)
    dev = slots.device
    cp = None
    if scores is not None:
        if scores.numel() != S:
            raise ValueError(f"scores: expected {S} values, got {scores.numel()}")
        scores = scores.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        cp = _dev(scores, torch.float32, "scores")
    # one buffer: a caller that wants all three copies one tensor
    out_idx, result, out_n = rle_block("nms", _out(out, rle_block_words("nms", S, G=G), torch.int32, dev, "out"), S, G=G)
    if S == 0:
        out_n.zero_()
        return out_idx, out_n, result
    check(lib.hgl_rle_nms_device(sp, sw, tp, S, images.ctypes.data, G, cp, thr, NMS_METRIC[metric], out_idx.data_ptr(),
                                 out_n.data_ptr(), result.data_ptr(),
                                 *_rle_ws(dev, lib.hgl_rle_nms_workspace_bytes, images.ctypes.data, G, S, sw), _stream()), "hgl_rle_nms_device")
    return out_idx, out_n, result


def rle_select_layout(sizes, counts, max_keep=None):
    """images [G,4] int64 = (H, W, first entry, max_keep) of a compaction over G images: image g owns counts[g] consecutive
    entries of sizes[g] = (H, W).  max_keep: None (no limit: -1 in every row), one number for every image, or one per image (None
    or a negative number: no limit for that image)"""
    if max_keep is None or not hasattr(max_keep, "__len__"):
        max_keep = [max_keep] * len(sizes)
    if len(max_keep) != len(sizes) == len(counts):      # the counts' length is refused first
        raise ValueError(f"rle_select_layout: {len(sizes)} sizes and {len(max_keep)} limits")
    return _rle_rows("rle_select_layout", sizes, counts, None,
                     lambda g, H, W, n, _: -1 if (mk := max_keep[g]) is None or (mk := int(mk)) < 0 else mk)[0]


def rle_select(slots, table, sizes, counts, keep=None, nms_result=None, cols=None, max_keep=None, out=None, back=None):
    """The kept entries of an encoded set, compacted image by image into a second, dense set (hgl_rle_select_device on the
    current stream, no synchronisation): the S entries of slots / table belong to G = len(sizes) <= 64 images, counts[g] <= 4096
    consecutive entries of sizes[g] = (H, W).  Exactly one of keep (bool / uint8 device tensor [S], nonzero = kept) and
    nms_result (the result [S,4] of rle_nms: kept iff the code is 0 or 1 and by == -1) says who survives; max_keep (see
    rle_select_layout) lets only the first max_keep kept entries of an image survive.  cols: a contiguous device tensor [C,S] of
    a 4-byte dtype, C <= 8, or None: side columns that travel with the entries.
    Returns (out_slots [S, slot_words], out_table [S,4], out_cols [C,S] in cols' dtype, out_src [S] int32, out_n [G] int32): from
    image g's first entry on, its out_n[g] survivors in stored order -- row, the words the row defines, columns, and out_src =
    the survivor's index within the image's list -- and behind them placeholders: an empty code-0 mask (row (1, 0, 0, 0), one
    count H*W), out_src -1, columns 0.  So rle_decode_group(out_slots, out_table, sizes, counts) needs no count from the device.
    Slot words beyond what an entry's form defines are not written.  The first three are views of ONE int32 buffer, table | slots
    | cols (`out`: a contiguous int32 device tensor of S * (4 + slot_words + C) elements to use for it), the last two of another,
    out_src | out_n (`back`: S + G elements)."""
    lib = _lib.load()
    ((sp, sw, tp, S),), images, _, G = _rle_group("rle_select", [(slots, table)], rle_select_layout, sizes, counts, max_keep=max_keep)
    if (keep is None) == (nms_result is None):
        raise ValueError("rle_select: exactly one of keep and nms_result selects the entries")
    dev = slots.device
    kp = rp = cp = None
    if keep is not None:
        if keep.numel() != S:
            raise ValueError(f"keep: expected {S} flags, got {keep.numel()}")
        kp, keep = _u8(keep.reshape(-1), "keep")
    else:
        if tuple(nms_result.shape) != (S, 4):
            raise ValueError(f"nms_result: expected [{S}, 4], got {tuple(nms_result.shape)}")
        rp = _dev(nms_result, torch.int32, "nms_result")
    C, cdtype = 0, torch.int32
    if cols is not None:
        if cols.dim() != 2 or cols.shape[1] != S or cols.element_size() != 4:
            raise ValueError(f"cols: expected a [C, {S}] tensor of a 4-byte dtype, got {tuple(cols.shape)} {cols.dtype}")
        C, cdtype = int(cols.shape[0]), cols.dtype
        if C:
            cp = _dev(cols, cdtype, "cols")
    out_table, out_slots, out_cols = rle_block("select", _out(out, rle_block_words("select", S, sw, C=C), torch.int32, dev, "out"), S, sw, C=C)
    out_src, out_n = rle_block("back", _out(back, rle_block_words("back", S, G=G), torch.int32, dev, "back"), S, G=G)
    out_cols = out_cols.view(cdtype)
    if S == 0:      # the entry launches nothing and leaves out_n alone
        out_n.zero_()
        return out_slots, out_table, out_cols, out_src, out_n
    check(lib.hgl_rle_select_device(sp, sw, tp, S, images.ctypes.data, G, kp, rp, cp, C, _ptr(out_slots), out_table.data_ptr(),
                                    out_cols.data_ptr() if C else None, out_src.data_ptr(), out_n.data_ptr(), _stream()),
          "hgl_rle_select_device")
    return out_slots, out_table, out_cols, out_src, out_n


CLEAN_MODES = {"holes": 1, "islands": 2, "both": 3}


def rle_remove_small_regions(slots, table, sizes, counts, area_thresh, mode="both", seg_cap=None, slot_words=None, out=None):
    """remove_small_regions (utils/amg.py:267-291) on an encoded set, image by image (hgl_rle_clean_device on the current stream,
    no synchronisation): the S entries of slots / table (what rle_encode or rle_pack returns) belong to G = len(sizes) <= 64
    images, counts[g] <= 4096 consecutive entries of sizes[g] = (H, W); an image may own none.  mode "holes": 8-connected
    components of the complement smaller than area_thresh are filled; "islands": components of the foreground smaller than it are
    dropped (the first largest in raster order stays when all are small); "both": holes, then islands on the result -- SAM's order.
    No mask becomes pixels and no pixel gets a label: the components are found on column segments.  seg_cap: the segments per
    entry and colour the workspace is sized for (an entry with more gets code 3); default the bound that never refuses, the
    set's largest W*ceil(H/2) + W; a caller who packed form-0 rows from strings passes slot_words // 2 + max W + 1.  slot_words:
    int32 words per output entry (default the input's).
    Returns (out_slots [S, slot_words], out_table [S,4]: the cleaned set as rle_encode would write it -- the canonical
    re-encoding where nothing was removed; boxes [S,4] int32: inclusive XYXY as sam.mask_boxes gives it; result [S,4] int32 =
    code, area after, changed (bit 0: the holes pass found a small component, bit 1: the islands pass did), area before).  Code 2
    (no mask in the slot) and 3 (over seg_cap): table row (0, 3, 0, 0), slot untouched, box zeros.  The four are views of ONE
    int32 buffer, table | slots | boxes | result (`out`: a contiguous int32 device tensor of S * (12 + slot_words) elements)."""
    lib = _lib.load()
    if mode not in CLEAN_MODES:
        raise ValueError(f"rle_remove_small_regions: mode {mode!r} (one of {sorted(CLEAN_MODES)})")
    ((sp, sw, tp, S),), images, _, G = _rle_group("rle_remove_small_regions", [(slots, table)], rle_clean_layout, sizes, counts)
    osw = sw if slot_words is None else int(slot_words)
    if seg_cap is None:
        seg_cap = max([int(W) * ((int(H) + 1) // 2) + int(W) for H, W in sizes], default=1)
    dev = slots.device
    out_table, out_slots, boxes, result = rle_block("clean", _out(out, rle_block_words("clean", S, osw), torch.int32, dev, "out"), S, osw)
    if S == 0:
        return out_slots, out_table, boxes, result
    check(lib.hgl_rle_clean_device(sp, sw, tp, S, images.ctypes.data, G, int(area_thresh), CLEAN_MODES[mode], int(seg_cap),
                                   _ptr(out_slots), osw, out_table.data_ptr(), boxes.data_ptr(), result.data_ptr(),
                                   *_rle_ws(dev, lib.hgl_rle_clean_workspace_bytes, images.ctypes.data, G, S, sw, int(seg_cap)), _stream()),
          "hgl_rle_clean_device")
    return out_slots, out_table, boxes, result


PAINT_FILL, PAINT_OUTLINE = 1 << 24, 1 << 25
_paint_pool = None      # the pinned staging of host paint lists: a buffer returns with the event behind its upload


def rle_paint_style(fill=None, a=1.0, b=0.0, outline=None):
    """One style row of rle_paint, uint32 [4]: fill / outline are (R, G, B) or None (the flag is then clear); a pixel of the mask
    becomes sat_u8(rint(pixel * a + fill * b)) per channel, a pixel of the mask's edge the outline colour."""
    import numpy as np
    rgb = lambda c: 0 if c is None else (int(c[0]) & 255) << 16 | (int(c[1]) & 255) << 8 | (int(c[2]) & 255)
    bits = np.array([a, b], dtype=np.float32).view(np.uint32)
    return np.array([rgb(fill) | (PAINT_FILL if fill is not None else 0) | (PAINT_OUTLINE if outline is not None else 0),
                     bits[0], bits[1], rgb(outline)], dtype=np.uint32)


def rle_paint_layout(sizes, counts, order_counts):
    """(images [G,5] int64 = H, W, first entry, first list position, pixel offset; total pixels) of a group's canvases packed
    back to back: image g owns counts[g] entries and order_counts[g] list positions"""
    return _rle_rows("rle_paint_layout", sizes, counts, order_counts, lambda g, H, W, n, m: H * W, running=True)


def rle_paint(slots, table, sizes, counts, order, order_counts, style, base=None, out=None, labels=False):
    """Entries of an encoded set painted over their images (hgl_rle_paint_device on the current stream, no synchronisation): the
    S entries of slots / table belong to G = len(sizes) <= 64 images, counts[g] consecutive entries of sizes[g] = (H, W), and
    the K list positions likewise, order_counts[g] each.  order [K]: position t of image g paints the image's entry order[t];
    style [K,4]: one rle_paint_style row per position (one row alone serves every position).  Either is a host sequence / array --
    both then travel in ONE pinned staging buffer and one copy -- or an int32 device tensor, taken as it is: the kept indices of
    rle_nms or the tail's winner index can be the list with no read-back.  base: None (black canvases), a contiguous uint8 device
    tensor of the packed canvases (3 * sum(H*W) bytes, RGB, row-major), or a list of G [H,W,3] uint8 device tensors.
    Returns (images: G uint8 views [H,W,3] of one buffer (`out`: a contiguous uint8 device tensor of exactly 3 * sum(H*W)
    elements, every byte of which is written); labels: G int32 views [H,W] -- the image-local list position that last changed
    the pixel, -1 for none -- or None; status [K,4] int32 = code, area, edge pixels, 0 (include/hybridgl.h)).  No mask becomes
    bytes.  ValueError, before anything is uploaded, for what the plan refuses."""
    import numpy as np
    global _paint_pool
    lib = _lib.load()
    on_dev = [torch.is_tensor(v) and v.is_cuda for v in (order, style)]
    K = int(order.numel()) if on_dev[0] else len(order)
    ((sp, sw, tp, S), _), images, total, G = _rle_group("rle_paint", [(slots, table), K], rle_paint_layout, sizes, counts, order_counts)
    dev = slots.device
    if not 1 <= G <= 64 or any(int(H) <= 0 or int(W) <= 0 or int(H) * int(W) >= 1 << 31 for H, W in sizes):
        raise ValueError(f"rle_paint: {G} images of sizes {list(sizes)} (1 .. 64 images, 0 < H*W < 2^31)")
    need = lib.hgl_rle_paint_workspace_bytes(images.ctypes.data, G, S, sw, K, total)
    if K and not need:
        raise ValueError("rle_paint: the library refuses this geometry (too many plane words or tiles for one call)")
    if isinstance(base, (list, tuple)):
        if len(base) != G or any(tuple(b.shape) != (int(H), int(W), 3) for b, (H, W) in zip(base, sizes)):
            raise ValueError("base: expected one [H, W, 3] tensor per image")
        base = torch.cat([b.reshape(-1) for b in base])
    if base is not None:
        base = _out(base, 3 * total, torch.uint8, dev, "base")
    flat = _out(out, 3 * total, torch.uint8, dev, "out")
    if base is not None and base.data_ptr() < flat.data_ptr() + flat.numel() and flat.data_ptr() < base.data_ptr() + base.numel():
        raise ValueError("out overlaps base")
    # the host halves of the list: one pinned buffer, one copy
    host = []
    if not on_dev[0]:
        host.append(np.asarray(order, dtype=np.int32).reshape(-1))
    if not on_dev[1]:
        rows = np.asarray(style, dtype=np.uint32)
        rows = np.broadcast_to(rows, (K, 4)) if rows.ndim == 1 else rows
        if rows.shape != (K, 4):
            raise ValueError(f"style: expected [{K}, 4] words, got {rows.shape}")
        host.append(rows.reshape(-1).view(np.int32) if rows.flags.c_contiguous else np.ascontiguousarray(rows).reshape(-1).view(np.int32))
    parts = []
    if host and K:
        if _paint_pool is None:
            from .staging import PinnedPool
            _paint_pool = PinnedPool(floor=1024)
        n = sum(h.size for h in host)
        pin = _paint_pool.take(n, torch.int32)
        pin.numpy()[:n] = np.concatenate(host)
        up = torch.empty(n, dtype=torch.int32, device=dev)
        up.copy_(pin[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _paint_pool.give(pin, ev)
        a = 0
        for h in host:
            parts.append(up[a:a + h.size])
            a += h.size
    order_d = order if on_dev[0] else (parts.pop(0) if K else None)
    style_d = style if on_dev[1] else (parts.pop(0) if K else None)
    op = sp_ = None
    if K:
        if order_d.numel() != K or style_d.numel() != 4 * K:
            raise ValueError(f"rle_paint: {K} list positions, {order_d.numel()} indices and {style_d.numel()} style words")
        op, sp_ = _dev(order_d, torch.int32, "order"), _dev(style_d, torch.int32, "style")
    status = torch.empty((K, 4), dtype=torch.int32, device=dev)      # one tensor of its own: no flat buffer to share, no block
    lab = torch.empty(total, dtype=torch.int32, device=dev) if labels else None
    ws = workspace(need, dev, "rle")
    check(lib.hgl_rle_paint_device(sp if S else None, sw, tp if S else None, S, op, sp_, K, images.ctypes.data, G,
                                   None if base is None else base.data_ptr(), flat.data_ptr(), total,
                                   None if lab is None else lab.data_ptr(), status.data_ptr() if K else None,
                                   ws.data_ptr(), ws.numel(), _stream()), "hgl_rle_paint_device")
    views = lambda buf, c: [buf[int(o) * c:(int(o) + int(H) * int(W)) * c].view(*((int(H), int(W), 3) if c == 3 else (int(H), int(W))))
                            for H, W, _, _, o in images]
    return views(flat, 3), (views(lab, 1) if labels else None), status


def heat_ramp(colours, a, b):
    """A ramp of heat_paint, uint32 [256,3]: row L = (colour 0x00RRGGBB, the fp32 bits of a_L, of b_L).  colours: [256,3] (R, G,
    B); a, b: 256 weights each, or one number for every level.  Level L paints sat_u8(rint(pixel * a_L + colour_L * b_L))."""
    import numpy as np
    c = np.asarray(colours, dtype=np.int64)
    if c.shape != (256, 3) or c.min() < 0 or c.max() > 255:
        raise ValueError(f"heat_ramp: expected [256, 3] colours in 0 .. 255, got {c.shape}")
    rows = np.empty((256, 3), dtype=np.uint32)
    rows[:, 0] = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    for col, w in ((1, a), (2, b)):
        w = np.asarray(w, dtype=np.float32)
        if w.shape not in ((), (256,)):
            raise ValueError(f"heat_ramp: expected one weight or 256, got {w.shape}")
        rows[:, col] = np.broadcast_to(w, (256,)).view(np.uint32) if w.shape else np.full(256, w, np.float32).view(np.uint32)
    return rows


def heat_paint_layout(sizes, dirflags=None, shared_heat=None, shared_base=None):
    """(maps [M,6] int64 = H, W, dirflag, heat element, base pixel, canvas pixel; heat elements; base pixels; canvas pixels) of
    M maps of sizes[m] = (H, W): the canvases packed back to back, and so the heat-maps and the base images -- except that maps
    with the same number in shared_heat [M] read ONE heat extent (one map under several directions) and maps with the same
    number in shared_base [M] ONE base image (several sentences over one image); both must then agree in size.  dirflags:
    "none" / "left" / "right" / "middle" or 0 .. 3 per map (default none)."""
    import numpy as np
    M = len(sizes)
    dirflags = [0] * M if dirflags is None else list(dirflags)
    if len(dirflags) != M or any(s is not None and len(s) != M for s in (shared_heat, shared_base)):
        raise ValueError(f"heat_paint_layout: {M} sizes, {len(dirflags)} dirflags and shared lists of other lengths")
    rows = np.zeros((M, 6), dtype=np.int64)
    ends = [0, 0, 0]      # heat, base, canvas
    seen = [{}, {}]
    for m, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        d = dirflags[m]
        d = DIRFLAG[d] if isinstance(d, str) else int(d)
        if H <= 0 or W <= 0 or H * W >= 1 << 31 or not 0 <= d <= 3:
            raise ValueError(f"heat_paint_layout: map {m}: size {H} x {W} (0 < H*W < 2^31), dirflag {dirflags[m]!r}")
        rows[m, :3] = (H, W, d)
        for k, shared in enumerate((shared_heat, shared_base)):
            key = None if shared is None else shared[m]
            if key is not None and key in seen[k]:
                at, size = seen[k][key]
                if size != (H, W):
                    raise ValueError(f"heat_paint_layout: map {m} shares an extent of size {size} but is {(H, W)}")
            else:
                at = ends[k]
                ends[k] += H * W
                if key is not None:
                    seen[k][key] = (at, (H, W))
            rows[m, 3 + k] = at
        rows[m, 5] = ends[2]
        ends[2] += H * W
    return rows, ends[0], ends[1], ends[2]


def heat_paint(heat, maps, ramp, base=None, out=None, levels=False):
    """Heat-maps turned into colours over their images (hgl_heat_paint_device on the current stream, no synchronisation; the
    contract is include/hybridgl.h's).  heat: contiguous float32 device tensor, read flat; maps: HOST [M,6] int64 rows (H, W,
    dirflag, heat element, base pixel, canvas pixel), what heat_paint_layout builds; ramp: [256,3] uint32 rows of heat_ramp, a
    host array (uploaded) or a device tensor; base: None (black) or a contiguous uint8 device tensor that holds every base extent
    (3 bytes per pixel); out: a contiguous uint8 device tensor of 3 * canvas pixels, every byte of a canvas written and none
    between canvases (default: a fresh one that ends with the last canvas).
    Returns (pictures: M uint8 views [H,W,3] of out; levels: M uint8 views [H,W] or None; status [M,4] int32 = code, bits of mn,
    of mx, of peak).  levels: False, True, or a uint8 device tensor of canvas pixels to write them to.  ValueError for a geometry
    the plan refuses; out over base is the library's HGL_EINVAL."""
    import numpy as np
    lib = _lib.load()
    maps = np.ascontiguousarray(np.asarray(maps, dtype=np.int64))
    if maps.ndim != 2 or maps.shape[1] != 6 or not 1 <= maps.shape[0] <= 64:
        raise ValueError(f"heat_paint: maps {maps.shape} (expected [M, 6], 1 <= M <= 64)")
    M = int(maps.shape[0])
    dev = heat.device
    hp = _dev(heat, torch.float32, "heat")
    px = maps[:, 0] * maps[:, 1]
    total = int((maps[:, 5] + px).max()) if out is None else out.numel() // 3
    if out is not None and out.numel() % 3:
        raise ValueError(f"out: {out.numel()} bytes are no whole number of pixels")
    need = lib.hgl_heat_paint_workspace_bytes(maps.ctypes.data, M, heat.numel(), total)
    if not need:
        raise ValueError(f"heat_paint: the library refuses this geometry ({M} maps, {heat.numel()} heat elements, {total} canvas pixels)")
    if base is not None:
        _dev(base, torch.uint8, "base")
        if int(maps[:, 4].min()) < 0 or 3 * int((maps[:, 4] + px).max()) > base.numel():
            raise ValueError(f"base: {base.numel()} bytes do not hold every base extent")
    flat = _out(out, 3 * total, torch.uint8, dev, "out")
    if isinstance(ramp, np.ndarray):
        if ramp.shape != (256, 3) or ramp.dtype != np.uint32:
            raise ValueError(f"ramp: expected [256, 3] uint32, got {ramp.shape} {ramp.dtype}")
        ramp = torch.from_numpy(ramp.view(np.int32).copy()).to(dev, non_blocking=True)
    if ramp.numel() != 768 or ramp.element_size() != 4:
        raise ValueError(f"ramp: expected [256, 3] words, got {tuple(ramp.shape)} {ramp.dtype}")
    rp = _dev(ramp, ramp.dtype, "ramp")
    status = torch.empty((M, 4), dtype=torch.int32, device=dev)
    lev = None if levels is False else _out(None if levels is True else levels, total, torch.uint8, dev, "levels")
    levels = lev is not None
    ws = workspace(need, dev, "rle")
    check(lib.hgl_heat_paint_device(hp, heat.numel(), maps.ctypes.data, M, rp, None if base is None else base.data_ptr(),
                                    flat.data_ptr(), total, None if lev is None else lev.data_ptr(), status.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()), "hgl_heat_paint_device")
    views = lambda buf, c: [buf[int(p) * c:(int(p) + int(H) * int(W)) * c].view(*((int(H), int(W), 3) if c == 3 else (int(H), int(W))))
                            for H, W, _, _, _, p in maps]
    return views(flat, 3), (views(lev, 1) if levels else None), status


POLY_RULE = {"once": 0, "any": 1}


def rle_from_polygons(entries, sizes, counts, rule="once", slot_words=None, device=None, out=None):
    """Polygons rasterised on the device, straight into RLE (hgl_rle_from_polygons_device on the current stream, no
    synchronisation): what rle_encode would return for the masks refer_io.gt_mask_from_polygons gives, without the pixels.
    entries: per entry a list of flat polygons [x0, y0, x1, y1, ...] (an entry may own none: the empty mask); the S entries
    belong to G = len(sizes) <= 64 images, counts[g] consecutive entries of sizes[g] = (H, W), as in rle_decode_group.
    rule: "once" = the pixels covered by exactly one polygon (the REFER target), "any" = by at least one.  slot_words: int32
    words per entry (default the largest ceil(H*W/32) of the call: nothing is ever lost).  One pinned staging buffer holds the
    coordinates and both offset arrays; one host -> device copy.  Returns (slots [S, slot_words] int32, table [S,4] int32 =
    n_counts, form, area, 0 as rle_encode writes them, status [S,4] int32 = code, sum of the polygons' own areas, 0, 0; code 0
    = rasterised, 2 = refused): three views of one flat buffer, table, slots, status in this order (`out`: a contiguous int32
    device tensor of S * (8 + slot_words) elements to use for it).  Raises ValueError before the upload for what the host codec refuses: a coordinate that is NaN
    or outside (-1e5, 1e5), a polygon without a vertex."""
    import numpy as np
    lib = _lib.load()
    if rule not in POLY_RULE:
        raise ValueError(f"rle_from_polygons: rule {rule!r} (one of {sorted(POLY_RULE)})")
    ((_, _, _, S),), images, _, G = _rle_group("rle_from_polygons", [len(entries)], rle_nms_layout, sizes, counts)
    polys, entry_polys = [], [0]
    for e, entry in enumerate(entries):
        for k, poly in enumerate(entry):
            xy = np.asarray(poly, dtype=np.float64).reshape(-1)
            if len(xy) < 2 or len(xy) % 2:
                raise ValueError(f"rle_from_polygons: entry {e} polygon {k} has {len(xy)} coordinates (x, y pairs, at least one)")
            if not bool(np.all((xy > -1.0e5) & (xy < 1.0e5))):      # false for a NaN
                raise ValueError(f"rle_from_polygons: entry {e} polygon {k}: a coordinate is NaN or outside (-1e5, 1e5)")
            polys.append(xy)
        entry_polys.append(len(polys))
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise _lib.HybridGLError(f"rle_from_polygons: device {device} (no CPU path exists)")
    if device.index is None:      # "cuda" is the current device: a lent `out` states the one it is on
        device = torch.device("cuda", torch.cuda.current_device())
    if slot_words is None:
        slot_words = max([rle_slot_words(H, W) for H, W in sizes], default=1)
    slot_words = int(slot_words)
    table, slots, status = rle_block("status", _out(out, rle_block_words("status", S, slot_words), torch.int32, device, "out"), S, slot_words)
    if S == 0:
        return slots, table, status
    P, n_xy = len(polys), int(sum(len(p) for p in polys))
    stage = torch.empty(8 * n_xy + 4 * (P + 1) + 4 * (S + 1), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    if P:
        host[:8 * n_xy].view(np.float64)[:] = np.concatenate(polys)
    off = host[8 * n_xy:].view(np.int32)
    off[0] = 0
    off[1:P + 1] = np.cumsum([len(p) // 2 for p in polys], dtype=np.int64)
    off[P + 1:] = entry_polys
    buf = stage.to(device, non_blocking=True)
    xy_p = buf.data_ptr()
    check(lib.hgl_rle_from_polygons_device(xy_p, xy_p + 8 * n_xy, P, xy_p + 8 * n_xy + 4 * (P + 1), S, images.ctypes.data, G,
                                           POLY_RULE[rule], _ptr(slots), slot_words, table.data_ptr(), status.data_ptr(),
                                           *_rle_ws(device, lib.hgl_rle_from_polygons_workspace_bytes, images.ctypes.data, G, S, P),
                                           _stream()), "hgl_rle_from_polygons_device")
    return slots, table, status


def rle_merge_rule(name, k):
    """(lo, hi) of a named vote over k members: a pixel is set iff lo <= (members that cover it) <= hi.  "union" (1, k),
    "intersect" (k, k), "majority" (k // 2 + 1, k), "at_least:T" (T, max(T, k)), "exactly:T" (T, T) with T >= 0.  ValueError on
    anything else.  Pure Python."""
    k = int(k)
    if k < 0:
        raise ValueError(f"rle_merge_rule: {k} members")
    if name == "union":
        return 1, max(k, 1)
    if name == "intersect":
        return k, k
    if name == "majority":
        return k // 2 + 1, max(k, k // 2 + 1)
    if isinstance(name, str) and ":" in name:
        kind, _, arg = name.partition(":")
        if kind in ("at_least", "exactly") and arg.isdigit():
            t = int(arg)
            return (t, max(t, k)) if kind == "at_least" else (t, t)
    raise ValueError(f"rle_merge_rule: rule {name!r} (union, intersect, majority, at_least:T, exactly:T)")


def rle_merge_layout(sizes, counts_src, counts_out):
    """images [G,4] int64 = (H, W, first source entry, first output entry) of a merge over G images: image g owns
    counts_src[g] consecutive source entries and counts_out[g] consecutive output entries of sizes[g] = (H, W)"""
    return _rle_rows("rle_merge_layout", sizes, counts_src, counts_out)[0]


def rle_merge(slots, table, sizes, counts_src, members, member_offsets, bounds, counts_out, slot_words=None, out=None):
    """New masks out of encoded masks, by vote (hgl_rle_merge_device on the current stream, no synchronisation): the source
    entries (slots / table: what rle_encode or rle_pack returns) belong to G = len(sizes) <= 64 images, counts_src[g]
    consecutive entries of sizes[g] = (H, W); image g owns counts_out[g] consecutive output entries.  Output entry s merges the
    source entries members[member_offsets[s] : member_offsets[s+1]] (absolute indices, all of its own image; one listed twice
    counts twice) and a pixel of it is set iff bounds[s] = (lo, hi) holds for the number of members that cover it
    (rle_merge_rule names the usual ones).  members: a list of per-entry lists (member_offsets is then None) or a flat int32
    sequence / device tensor with member_offsets [S+1]; bounds: [S,2].  slot_words: int32 words per output entry (default the
    largest ceil(H*W/32) of the call: nothing is ever lost).  Returns (slots [S, slot_words] int32, table [S,4] int32 as
    rle_encode writes them, status [S,4] int32 = code, k, 0, 0; code 0 = merged, 1 = merged with a clipped member, 2 = refused):
    three views of one flat buffer, table, slots, status in this order (`out`: a contiguous int32 device tensor of
    S * (8 + slot_words) elements to use for it).  No mask becomes pixels."""
    import numpy as np
    lib = _lib.load()
    ((sp, sw, tp, Ssrc), (_, _, _, S)), images, _, G = _rle_group(
        "rle_merge", [(slots, table), sum(int(n) for n in counts_out)], rle_merge_layout, sizes, counts_src, counts_out)
    dev = slots.device
    if member_offsets is None:
        lists = [np.asarray(m, dtype=np.int64).reshape(-1) for m in members]
        member_offsets = np.concatenate([[0], np.cumsum([len(m) for m in lists], dtype=np.int64)])
        members = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)

    def i32(x, shape, name):
        if not torch.is_tensor(x):
            a = np.asarray(x, dtype=np.int64).reshape(shape)
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError(f"rle_merge: {name} does not fit int32")
            x = torch.from_numpy(a.astype(np.int32))
        x = x.to(device=dev, dtype=torch.int32).reshape(shape).contiguous()
        return x

    members = i32(members, (-1,), "members")
    member_offsets = i32(member_offsets, (-1,), "member_offsets")
    bounds = i32(bounds, (-1, 2), "bounds")
    M = int(members.numel())
    if member_offsets.numel() != S + 1 or bounds.shape[0] != S:
        raise ValueError(f"rle_merge: {S} output entries need {S + 1} member offsets and {S} bounds, got {member_offsets.numel()} "
                         f"and {bounds.shape[0]}")
    if slot_words is None:
        slot_words = max([rle_slot_words(H, W) for H, W in sizes], default=1)
    slot_words = int(slot_words)
    otable, oslots, status = rle_block("status", _out(out, rle_block_words("status", S, slot_words), torch.int32, dev, "out"), S, slot_words)
    if S == 0:
        return oslots, otable, status
    check(lib.hgl_rle_merge_device(sp if Ssrc else None, sw, tp if Ssrc else None, Ssrc, images.ctypes.data, G,
                                   members.data_ptr() if M else None, M, member_offsets.data_ptr(), bounds.data_ptr(),
                                   _ptr(oslots), slot_words, otable.data_ptr(), S, status.data_ptr(),
                                   *_rle_ws(dev, lib.hgl_rle_merge_workspace_bytes, images.ctypes.data, G, Ssrc, sw, S, M), _stream()),
          "hgl_rle_merge_device")
    return oslots, otable, status


def score_sentence(hybrid, sentence_feat, noun_phrase_feat, other_noun_feats, boxes, gem_score,
                   logit_scale=100.0, r=0.5, k1=3, k2=6, alpha=0.6, relaword="none", has_other_nouns=False):
    """Per-sentence tail (Hybridgl_main.py:153-196,225-228).

    other_noun_feats: [K,E] tensor or None.  Returns (idx[2] int32: pure argmax, final index;
    score_clip [N]; score_neg [N])."""
    lib = _lib.load()
    N, E = hybrid.shape
    dev = hybrid.device
    idx = torch.empty((2,), dtype=torch.int32, device=dev)
    sc = torch.empty((N,), dtype=torch.float32, device=dev)
    sn = torch.empty((N,), dtype=torch.float32, device=dev)
    need = lib.hgl_score_sentence_workspace_bytes(N, E)
    ws = workspace(need, dev, "score_sentence")
    n_other = 0 if other_noun_feats is None else int(other_noun_feats.shape[0])
    sent = sentence_feat.reshape(-1)
    nphr = noun_phrase_feat.reshape(-1)
    check(lib.hgl_score_sentence(_dev(hybrid, torch.float32, "hybrid"),
                                 _dev(sent, torch.float32, "sentence_feat"),
                                 _dev(nphr, torch.float32, "noun_phrase_feat"),
                                 _dev(other_noun_feats, torch.float32, "other_noun_feats") if n_other else None,
                                 n_other, float(r),
                                 _dev(boxes, torch.int64, "boxes"), _dev(gem_score, torch.float32, "gem_score"),
                                 N, E, float(logit_scale), int(k1), int(k2), float(alpha),
                                 RELAWORD.get(relaword, 0), int(bool(has_other_nouns)),
                                 idx.data_ptr(), sc.data_ptr(), sn.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream()), "hgl_score_sentence")
    return idx, sc, sn


def _pack_sentences(sentences, H, W, keep, what="sentence"):
    """list of sentence dicts (score_ref's docstring) -> HglSentence array; the tensors behind its pointers go to `keep`"""
    recs = (_lib.HglSentence * len(sentences))()
    for j, q in enumerate(sentences):
        a = q["imgattn"]
        if tuple(a.shape) != (H, W):
            raise ValueError(f"{what} {j}: imgattn {tuple(a.shape)} != masks {(H, W)}")
        tp, tt = _u8(q["target"], "target")
        if tuple(tt.shape) != (H, W):
            raise ValueError(f"{what} {j}: target {tuple(tt.shape)} != masks {(H, W)}")
        keep += [a, tt]
        recs[j] = _lib.HglSentence(int(q["sentence_row"]), int(q["noun_phrase_row"]), int(q.get("other_row0", 0)), int(q.get("n_other", 0)),
                                   DIRFLAG.get(q.get("dirflag", "none"), 0), RELAWORD.get(q.get("relaword", "none"), 0),
                                   int(bool(q.get("has_other_nouns", False))), float(q.get("black", 1.8)),
                                   _dev(a, torch.float32, "imgattn"), tp)
    return recs


def _tail_outputs(S, N, dev, want_scores):
    """(idx [S,2] int32, iu [S,4] int64, score_clip, score_neg, gem [S,N] or None) and the pointers of the last three"""
    idx = torch.empty((S, 2), dtype=torch.int32, device=dev)
    iu = torch.empty((S, 4), dtype=torch.int64, device=dev)
    scores = tuple(torch.empty((S, N), dtype=torch.float32, device=dev) if want_scores else None for _ in range(3))
    return (idx, iu) + scores, [t.data_ptr() if t is not None else None for t in scores]


def score_ref(hybrid, text, boxes, masks, sentences, logit_scale=100.0, r=0.5, k1=3, k2=6, alpha=0.6, cum=None, want_scores=False):
    """The whole tail of one dataset item (Hybridgl_main.py:153-230) in four launches: hgl_score_ref.

    hybrid [N,E], text [T,E] (every string of the ref), boxes [N,4] int64 XYWH, masks [N,H,W] bool / uint8;
    sentences: list of dicts {sentence_row, noun_phrase_row, other_row0, n_other, dirflag, relaword (strings as in the
    reference), has_other_nouns, black, imgattn [H,W] fp32 tensor, target [H,W] bool / uint8 tensor}.
    cum: int64 [4] device tensor incremented in place by (I, U, I_final, U_final) summed over the sentences.
    Returns (idx [S,2] int32, iu [S,4] int64) and, with want_scores, (score_clip, score_neg, gem) [S,N] each."""
    lib = _lib.load()
    N, E = hybrid.shape
    T = text.shape[0]
    S = len(sentences)
    mp, masks = _u8(masks, "masks")
    _, H, W = masks.shape
    dev = hybrid.device
    keep = []
    recs = _pack_sentences(sentences, H, W, keep)
    out, (scp, snp, gmp) = _tail_outputs(S, N, dev, want_scores)
    need = lib.hgl_score_ref_workspace_bytes(S, N, E, H, W)
    ws = workspace(need, dev, "score_ref")
    check(lib.hgl_score_ref(_dev(hybrid, torch.float32, "hybrid"), _dev(text, torch.float32, "text"), T,
                            _dev(boxes, torch.int64, "boxes"), mp, N, E, H, W, recs, S, float(logit_scale), float(r), int(k1), int(k2),
                            float(alpha), out[0].data_ptr(), out[1].data_ptr(), _dev(cum, torch.int64, "cum") if cum is not None else None,
                            scp, snp, gmp, ws.data_ptr(), ws.numel(), _stream()), "hgl_score_ref")
    return out if want_scores else out[:2]


def _group_ref(i, q, keep, k1, k2, idx, iu, scores=(None, None, None)):
    """one ref dict of score_group -> its HglGroupRef record with the given k1 / k2 and output pointers; what the record points
    to goes to `keep`"""
    hybrid, text = q["hybrid"], q["text"]
    mp, masks = _u8(q["masks"], "masks")
    _, H, W = masks.shape
    sent = _pack_sentences(q["sentences"], H, W, keep, f"ref {i} sentence")
    keep += [sent, masks]
    return _lib.HglGroupRef(_dev(hybrid, torch.float32, "hybrid"), _dev(text, torch.float32, "text"), text.shape[0],
                            _dev(q["boxes"], torch.int64, "boxes"), mp, hybrid.shape[0], H, W, sent, len(q["sentences"]), int(k1), int(k2),
                            idx, iu, *scores)


def score_group(refs, logit_scale=100.0, r=0.5, alpha=0.6, cum=None, want_scores=False):
    """The tails of the R refs of a group (Hybridgl_main.py:153-230 each) in ONE set of four launches: hgl_score_group.
    refs: list of dicts {hybrid [N,E], text [T,E], boxes [N,4] int64, masks [N,H,W], sentences (as for score_ref), k1, k2};
    shapes may differ from ref to ref.  cum as for score_ref.  Returns one tuple per ref, as score_ref would (rows identical
    to its rows)."""
    lib = _lib.load()
    R = len(refs)
    recs = (_lib.HglGroupRef * R)()
    keep, outs = [], []
    E = refs[0]["hybrid"].shape[1]
    dev = refs[0]["hybrid"].device
    for i, q in enumerate(refs):
        out, scores = _tail_outputs(len(q["sentences"]), q["hybrid"].shape[0], dev, want_scores)
        recs[i] = _group_ref(i, q, keep, q["k1"], q["k2"], out[0].data_ptr(), out[1].data_ptr(), scores)
        outs.append(out if want_scores else out[:2])
    need = lib.hgl_score_group_workspace_bytes(recs, R, E)
    ws = workspace(need, dev, "score_group")
    check(lib.hgl_score_group(recs, R, E, float(logit_scale), float(r), float(alpha),
                              _dev(cum, torch.int64, "cum") if cum is not None else None, ws.data_ptr(), ws.numel(), _stream()),
          "hgl_score_group")
    return outs


def _sweep_k(q, configs, name):
    """the C values of k1 / k2 (`name`) of one ref: the ref's own sequence of C (a caller that carries a clamp per
    configuration), else the configuration's (r, alpha, k1, k2), else the ref's int"""
    own = q.get(name)
    if own is not None and not isinstance(own, int):
        own = [int(v) for v in own]
        if len(own) != len(configs):
            raise ValueError(f"{name}: {len(own)} values for {len(configs)} configurations")
        return own
    at = 2 if name == "k1" else 3
    if any(len(t) < 4 for t in configs) and own is None:
        raise ValueError(f"a configuration without k1 / k2 needs the ref's own {name}")
    return [int(t[at]) if len(t) >= 4 else int(own) for t in configs]


def score_group_sweep(refs, configs, logit_scale=100.0, cum=None, cum_ceiling=None):
    """score_group under C configurations of (r, alpha, k1, k2) in one pass: hgl_score_group_sweep (min / max and pooling once,
    one pass over the mask planes for the IoU of every proposal with every target, one scoring workgroup per sentence and
    distinct r).  refs as for score_group; configs: list of (r, alpha) or (r, alpha, k1, k2), at most 256 with at most 32
    distinct r.  A ref's k1 / k2 per configuration: the ref's own k1 / k2 when that is a sequence of C, else the
    configuration's, else the ref's int.  cum: int64 [C,4] device tensor, incremented by every configuration's column sums;
    cum_ceiling: int64 [2], incremented by the (I, U) of every sentence's best proposal.
    Returns per ref (idx [C,S,2] int32, iu [C,S,4] int64, ceiling [S,3] int64 = best proposal, its I, its U); row c equals
    score_group's rows under configuration c bit for bit."""
    import ctypes as C_
    lib = _lib.load()
    R, C = len(refs), len(configs)
    cfg = (_lib.HglSweepConfig * max(C, 1))()
    for c, t in enumerate(configs):
        cfg[c] = _lib.HglSweepConfig(float(t[0]), float(t[1]))
    recs = (_lib.HglGroupRef * R)()
    swp = (_lib.HglSweepRef * R)()
    keep, outs = [], []
    E = refs[0]["hybrid"].shape[1]
    dev = refs[0]["hybrid"].device
    for i, q in enumerate(refs):
        S = len(q["sentences"])
        k1, k2 = _sweep_k(q, configs, "k1"), _sweep_k(q, configs, "k2")
        ks = (C_.c_int32 * max(2 * C, 1))(*[v for pair in zip(k1, k2) for v in pair])
        out = (torch.empty((C, S, 2), dtype=torch.int32, device=dev), torch.empty((C, S, 4), dtype=torch.int64, device=dev),
               torch.empty((S, 3), dtype=torch.int64, device=dev))
        recs[i] = _group_ref(i, q, keep, 1, 1, None, None)
        swp[i] = _lib.HglSweepRef(ks, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        keep.append(ks)
        outs.append(out)
    need = lib.hgl_score_group_sweep_workspace_bytes(recs, R, E, cfg, C)
    ws = workspace(need, dev, "score_group_sweep")
    check(lib.hgl_score_group_sweep(recs, swp, R, E, float(logit_scale), cfg, C,
                                    _dev(cum, torch.int64, "cum") if cum is not None else None,
                                    _dev(cum_ceiling, torch.int64, "cum_ceiling") if cum_ceiling is not None else None,
                                    ws.data_ptr(), ws.numel(), _stream()), "hgl_score_group_sweep")
    return outs


def synthesize_views(sam_img, blurred, image_norm, masks, res=224, out=None):
    """Hybridgl_main.py:93-125 -> (local_imgs, global_imgs) [N,3,res,res] fp32 (written into `out` when given)."""
    lib = _lib.load()
    N, H, W = masks.shape
    mp, masks = _u8(masks, "masks")
    dev = masks.device
    if out is not None:
        loc, glo = out
        assert tuple(loc.shape) == (N, 3, res, res) == tuple(glo.shape) and loc.is_contiguous() and glo.is_contiguous()
    else:
        loc = torch.empty((N, 3, res, res), dtype=torch.float32, device=dev)
        glo = torch.empty((N, 3, res, res), dtype=torch.float32, device=dev)
    check(lib.hgl_synthesize_views(_dev(sam_img, torch.uint8, "sam_img"), _dev(blurred, torch.uint8, "blurred"),
                                   _dev(image_norm, torch.float32, "image_norm"), mp, N, H, W, res,
                                   loc.data_ptr(), glo.data_ptr(), _stream()), "hgl_synthesize_views")
    return loc, glo


# ---- visual prompts (include/hybridgl.h HglViewPrompt; the rules are csrc/view_prompt.h) ----
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # Hybridgl_main.py:93
_VP_ENUMS = {"window": {"frame": 0, "box": 1}, "local_bg": {"fill": 0, "keep": 1},
             "global_bg": {"blur": 0, "keep": 1, "gray": 2, "fill": 3}, "marker": {"none": 0, "ellipse": 1, "box": 2},
             "square": {"off": 0, "on": 1, "false": 0, "true": 1}}
_VP_RANGES = {"window": (0, 1), "pad_permille": (0, 4000), "square": (0, 1), "local_bg": (0, 1), "global_bg": (0, 3),
              "marker": (0, 2), "thickness": (1, 64), "grow": (0, 4096)}
_VP_COLOURS = ("local_fill", "global_fill", "marker_rgb")
VIEW_PROMPT_PRESETS = {
    "hybridgl": {},                                                           # Hybridgl_main.py:93-125
    "black": {"global_bg": "fill", "global_fill": (0, 0, 0)},                 # utils.py:336 'black'
    "gray": {"global_bg": "gray"},
    "keep": {"global_bg": "keep"},
    "red_circle": {"global_bg": "keep", "marker": "ellipse", "marker_rgb": (255, 0, 0), "thickness": 2},   # utils.py:322 'circle'
    "masked_crop": {"window": "box", "square": 1},
    "crop": {"window": "box", "square": 1, "local_bg": "keep"},
}


def view_prompt(preset="hybridgl", **fields):
    """-> _lib.HglViewPrompt: the preset (VIEW_PROMPT_PRESETS), then `fields` over it.  Enumerated fields take their number or
    their name (window="box", global_bg="gray", marker="ellipse"); colours take three numbers.  ValueError names the field."""
    if preset not in VIEW_PROMPT_PRESETS:
        raise ValueError(f"view_prompt: unknown preset {preset!r} (one of {', '.join(VIEW_PROMPT_PRESETS)})")
    vals = {"window": 0, "pad_permille": 0, "square": 0, "local_bg": 0, "local_fill": CLIP_MEAN, "global_bg": 0,
            "global_fill": (0, 0, 0), "marker_rgb": (255, 0, 0), "marker": 0, "thickness": 1, "grow": 0}
    p = _lib.HglViewPrompt()
    for key, v in {**vals, **VIEW_PROMPT_PRESETS[preset], **fields}.items():
        if key not in vals:
            raise ValueError(f"view_prompt: unknown field {key!r}")
        if key in _VP_COLOURS:
            try:
                v = [float(c) if key == "local_fill" else int(c) for c in v]
            except (TypeError, ValueError):
                v = []
            ok = (lambda c: abs(c) < float("inf")) if key == "local_fill" else (lambda c: 0 <= c <= 255)
            if len(v) != 3 or not all(ok(c) for c in v):
                raise ValueError(f"view_prompt: {key} takes three " + ("finite numbers" if key == "local_fill" else "numbers 0..255"))
            getattr(p, key)[:] = v
            continue
        if isinstance(v, str) and v in _VP_ENUMS.get(key, {}):
            v = _VP_ENUMS[key][v]
        try:
            v = int(v) if not isinstance(v, float) or v == int(v) else None
        except (TypeError, ValueError):
            v = None
        lo, hi = _VP_RANGES[key]
        if v is None or not lo <= v <= hi:
            names = f" or one of {', '.join(_VP_ENUMS[key])}" if key in _VP_ENUMS else ""
            raise ValueError(f"view_prompt: {key} takes {lo}..{hi}{names}")
        setattr(p, key, v)
    return p


def parse_view_prompt(spec):
    """The command line's --view_prompt: a preset name, `key=value,key=value`, or a preset followed by such pairs
    ("red_circle,thickness=3,marker_rgb=0:255:0"; the three numbers of a colour are joined by ':').  None / "" -> None."""
    if spec is None or isinstance(spec, _lib.HglViewPrompt):
        return spec
    parts = [s.strip() for s in str(spec).split(",") if s.strip()]
    if not parts:
        return None
    preset = parts.pop(0) if "=" not in parts[0] else "hybridgl"
    fields = {}
    for part in parts:
        key, eq, val = (s.strip() for s in part.partition("="))
        if not eq or not key or not val:
            raise ValueError(f"view_prompt: {part!r} is not key=value")
        if key in fields:
            raise ValueError(f"view_prompt: {key} given twice")
        fields[key] = val.split(":") if key in _VP_COLOURS else val
    return view_prompt(preset, **fields)


def view_prompt_fields(p):
    """the struct as a plain dict (colours as tuples)"""
    return {k: (tuple(getattr(p, k)) if k in _VP_COLOURS else getattr(p, k)) for k, _ in p._fields_}


def view_prompt_is_default(p):
    return p is None or view_prompt_fields(p) == view_prompt_fields(view_prompt())


def view_prompt_name(p):
    """the preset's name when the prompt is one, else its non-default fields as a spec (the result log's header)"""
    f = view_prompt_fields(p if p is not None else view_prompt())
    for name in VIEW_PROMPT_PRESETS:
        if f == view_prompt_fields(view_prompt(name)):
            return name
    d = view_prompt_fields(view_prompt())
    return ",".join(f"{k}={':'.join(str(c) for c in v) if isinstance(v, tuple) else v}" for k, v in f.items() if v != d[k])


def view_prompt_needs_boxes(p):
    return p.window == 1 or p.marker != 0


def xywh_to_view_boxes(boxes):
    """a record's XYWH boxes -> the inclusive int32 XYXY of hgl_mask_boxes: (x, y, x + w, y + h), as box_xyxy_to_xywh only
    subtracts"""
    b = boxes.to(torch.int32)
    return torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], dim=1).contiguous()


def synthesize_views_prompt(sam_img, blurred, image_norm, masks, prompt, boxes=None, res=224, out=None):
    """synthesize_views under a visual prompt (view_prompt / parse_view_prompt).  boxes: [N,4] int32 inclusive XYXY; None with
    a prompt that needs boxes computes them with sam.mask_boxes.  blurred may be None unless the prompt's global background
    is the blur."""
    import ctypes as C
    lib = _lib.load()
    N, H, W = masks.shape
    mp, masks = _u8(masks, "masks")
    dev = masks.device
    if out is not None:
        loc, glo = out
        assert tuple(loc.shape) == (N, 3, res, res) == tuple(glo.shape) and loc.is_contiguous() and glo.is_contiguous()
    else:
        loc = torch.empty((N, 3, res, res), dtype=torch.float32, device=dev)
        glo = torch.empty((N, 3, res, res), dtype=torch.float32, device=dev)
    if boxes is None and view_prompt_needs_boxes(prompt) and N > 0:
        from . import sam
        boxes = sam.mask_boxes(masks)
    if boxes is not None and tuple(boxes.shape) != (N, 4):
        raise ValueError(f"boxes: expected [{N}, 4], got {tuple(boxes.shape)}")
    check(lib.hgl_synthesize_views_prompt(_dev(sam_img, torch.uint8, "sam_img"),
                                          _dev(blurred, torch.uint8, "blurred") if blurred is not None else None,
                                          _dev(image_norm, torch.float32, "image_norm"), mp,
                                          _dev(boxes, torch.int32, "boxes") if boxes is not None else None, N, H, W, res,
                                          C.byref(prompt), loc.data_ptr(), glo.data_ptr(), _stream()),
          "hgl_synthesize_views_prompt")
    return loc, glo


def cv_gaussian_kernel_q8(k=15, sigma=0.0):
    """the k 8.8 fixed-point taps of cv2.GaussianBlur on uint8 (sum 256) -> ctypes uint16 array (host)"""
    import ctypes as C
    taps = (C.c_uint16 * k)()
    check(_lib.load().hgl_cv_gaussian_kernel_q8(k, float(sigma), taps), "hgl_cv_gaussian_kernel_q8")
    return taps


def gaussian_blur_u8(img, k=15, sigma=0.0, mode="cv2"):
    """cv2.GaussianBlur(img, (k, k), sigma) on a [H,W,C] uint8 device tensor (Hybridgl_main.py:99).
    mode="cv2": OpenCV's 8-bit fixed-point path restated (integer arithmetic; parity with the package unpinned);
    mode="float": the double-precision separable Gaussian of synth.box_blur_u8, bit-identical to it."""
    import ctypes as C
    import numpy as np
    lib = _lib.load()
    H, W, Cc = img.shape
    out = torch.empty_like(img)
    ws = workspace(lib.hgl_gaussian_blur_u8_workspace_bytes(H, W, Cc), img.device, "blur")
    if mode == "cv2":
        taps = cv_gaussian_kernel_q8(k, sigma)
        check(lib.hgl_gaussian_blur_u8_q8(_dev(img, torch.uint8, "img"), H, W, Cc, taps, taps, k, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "hgl_gaussian_blur_u8_q8")
        return out
    assert mode == "float"
    sigma = sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    r = k // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2 * sigma * sigma))
    g /= g.sum()
    taps = (C.c_double * k)(*[float(v) for v in g])
    check(lib.hgl_gaussian_blur_u8(_dev(img, torch.uint8, "img"), H, W, Cc, taps, k, out.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _stream()), "hgl_gaussian_blur_u8")
    return out
