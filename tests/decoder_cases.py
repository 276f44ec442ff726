"""Cases, float64 reference and route restatement for the SAM mask decoder (csrc/sam_api.hip: dec_route / decode_impl behind
hgl_sam_decode_points(_gated / _multi) and hgl_sam_decode_prompts; csrc/sam_decoder_fused.hip: dec_tail_kernel, dec_i2t_kernel;
csrc/sam_decoder_t2i.hip: t2i_fold_q_kernel, t2i_raw_attn_kernel, t2i_unfold_v_kernel, i2t_prep_kernel, dec_i2t_fold_kernel),
plain numpy, no GPU code.

THE REFERENCE is a second implementation, in float64 and straight from the formulae, of PromptEncoder (points, labelled points and
box corners, mask inputs; modeling/prompt_encoder.py) and of MaskDecoder.predict_masks with its TwoWayTransformer
(modeling/mask_decoder.py, modeling/transformer.py), with the call surface of oracle/sam_oracle.py: embed_points, embed_prompts,
embed_masks, dense_pe, mask_decoder.  It shares no code with the oracle (tests/test_decoder_cases_host.py holds the two against
each other).  What the device is handed in fp32 -- normalised coordinates, the embedding, the weights -- is read as those fp32
values; everything after that is float64.  mask_decoder takes a list of prompt indices and computes only those (prompts do
not interact), and can return the tensors a bisection needs (`inter`: tokens and image tokens after each layer, the tokens after
the final attention, the upscaled rows, the hyper-network rows, the widest token -> image score range and the peak probability).

THE STRESS KNOB.  stress_decoder(sd, temp) multiplies q_proj of the three token -> image attentions by temp (1, 4 or 16): with the
seeded weights the widest score range of a token -> image row is about 16 in base e, at temp 16 about 250 with a peak
probability of 1.0 -- exponentials underflow, whole key ranges carry no weight, the running maximum stops moving early.

THE ROUTE.  dec_route(...) below restates the conditions of DecRoute dec_route() in csrc/sam_api.hip for the decoder every case
uses (C = 256, 8 heads, internal width 128, every weight registered in the split modes), capacities included;
route_kernels(...) says which decoder-specific kernels such a route launches.  The table names both per case BY HAND; the host
test holds the hand-written fields and kernel sets against these two functions.

Two facts the capacity conditions decide, which reading the shape conditions alone misses (HW image tokens, per prompt):
  the image -> token buffer (DecPlan::atti) holds 512 HW bytes; the raw token -> image attention needs 114 688 bytes for the
  folded queries plus 57 792 per key range (RawT2iScratch::bytes).
  * grid 16 (HW 256, 131 072 bytes): too small for one key range (172 480) -- raw_t2i is OFF at grid 16 for every prompt
    count, ns is computed (8 at P = 5, 1 at P = 129) but unused.  Fusion masks 23 and 55 take the same route there.
  * grid 32 (HW 1024, 524 288 bytes): holds one key range (172 480) but not eight (577 024) -- raw_t2i is on from 129
    prompts per image (ns = 1) and off below.
  * grid 48 (HW 2304 = 9 x 256) is the smallest square grid that takes raw_t2i with eight key ranges (nine chunks of 32 keys
    a range); grids 64 and 128 take it as well.
The grid-16 and grid-32 cases with few prompts stay in the table with the route they really take; raw32_p129, raw48,
raw48_multi3x5, raw32_multi2x129 and the grid-64 / grid-128 cases are the ones that reach the raw kernels, and the stress knob
runs on both kinds.
"""
import math
from collections import namedtuple

import numpy as np
from scipy.special import erf

F32, F64 = np.float32, np.float64
HEADS, C, INTERNAL = 8, 256, 128
ALL_FUSED = 0x7fffffff


def encoder_cfg(grid):
    """the cheapest encoder that constructs around a decoder of this grid (the encoder is never run)"""
    return dict(embed_dim=64, depth=1, num_heads=2, global_attn_indexes=(0,), img_size=16 * grid, patch_size=16, window_size=0,
                out_chans=C)


# ============================================================================================================ the reference
def _w(sd, key):
    return np.asarray(sd[key], dtype=F64)


def _linear(sd, key, x):
    return x @ _w(sd, key + ".weight").T + _w(sd, key + ".bias")


def _layer_norm(sd, key, x, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * _w(sd, key + ".weight") + _w(sd, key + ".bias")


def _gelu(x):
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def _pe(sd, c01):
    """PositionEmbeddingRandom._pe_encoding: sin | cos of 2 pi (2 c - 1) G"""
    ang = 2.0 * math.pi * ((2.0 * np.asarray(c01, dtype=F64) - 1.0) @ _w(sd, "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"))
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=-1)


def coords01(xy, input_size):
    """(pixel + 0.5) / size as the fp32 values the device is handed"""
    xy = np.asarray(xy)
    xy = xy if xy.dtype in (np.float32, np.float64) else xy.astype(F64)
    return ((xy + xy.dtype.type(0.5)) / xy.dtype.type(input_size)).astype(F32)


def dense_pe(sd, h, w):
    """get_dense_pe -> [h*w, C]; the cell centres (i + 0.5) / n as the fp32 values the device is handed"""
    y = ((np.arange(h, dtype=F32) + F32(1)) - F32(0.5)) / F32(h)
    x = ((np.arange(w, dtype=F32) + F32(1)) - F32(0.5)) / F32(w)
    grid = np.stack([np.broadcast_to(x[None, :], (h, w)), np.broadcast_to(y[:, None], (h, w))], axis=-1)
    return _pe(sd, grid).reshape(h * w, -1)


def embed_points(sd, points_xy, input_size=1024):
    """one foreground point + the padding point per prompt: [P,2] pixels -> [P,2,C]"""
    P = len(points_xy)
    out = np.empty((P, 2, C), dtype=F64)
    out[:, 0] = _pe(sd, coords01(np.asarray(points_xy, dtype=F64), input_size)) + _w(sd, "prompt_encoder.point_embeddings.1.weight")[0]
    out[:, 1] = _w(sd, "prompt_encoder.not_a_point_embed.weight")[0]
    return out


def embed_prompts(sd, coords_xy, labels, input_size=1024):
    """[P,n,2] pixels, labels [P,n] (-1 padding, 0 / 1 points, 2 / 3 box corners) -> [P,n,C]"""
    labels = np.asarray(labels)
    out = _pe(sd, coords01(coords_xy, input_size))
    out[labels == -1] = _w(sd, "prompt_encoder.not_a_point_embed.weight")[0]
    for lab in range(4):
        out[labels == lab] += _w(sd, f"prompt_encoder.point_embeddings.{lab}.weight")[0]
    return out


def embed_masks(sd, mask_input):
    """mask_downscaling: [B,1,4h,4w] -> [B, h*w, C]: conv 2x2 stride 2 (1 -> 4), LayerNorm2d, GELU, conv 2x2 stride 2 (4 -> 16),
    LayerNorm2d, GELU, conv 1x1 (16 -> C)"""
    p = "prompt_encoder.mask_downscaling"

    def conv2(x, key):      # x [B,H,W,ci], weight [co,ci,2,2]
        w = _w(sd, f"{p}.{key}.weight")
        out = np.zeros(x.shape[:1] + (x.shape[1] // 2, x.shape[2] // 2, w.shape[0]), dtype=F64)
        for ky in range(2):
            for kx in range(2):
                out += x[:, ky::2, kx::2, :] @ w[:, :, ky, kx].T
        return out + _w(sd, f"{p}.{key}.bias")

    x = np.asarray(mask_input, dtype=F64)[:, 0, :, :, None]
    x = _gelu(_layer_norm(sd, f"{p}.1", conv2(x, "0"), 1e-6))
    x = _gelu(_layer_norm(sd, f"{p}.4", conv2(x, "3"), 1e-6))
    w3 = _w(sd, f"{p}.6.weight")
    x = x @ w3.reshape(w3.shape[0], -1).T + _w(sd, f"{p}.6.bias")
    return x.reshape(x.shape[0], -1, x.shape[-1])


def _attention(sd, p, q, k, v, stats=None):
    """Attention.forward: projections, 8 heads, soft-max(q k^T / sqrt(d)) v, out-projection.  stats: [range, peak] updated with
    the widest score range of a row and the largest probability"""
    q, k, v = _linear(sd, f"{p}.q_proj", q), _linear(sd, f"{p}.k_proj", k), _linear(sd, f"{p}.v_proj", v)
    B, Nq, I = q.shape
    d = I // HEADS
    qh, kh, vh = (t.reshape(t.shape[0], t.shape[1], HEADS, d).transpose(0, 2, 1, 3) for t in (q, k, v))     # [B, heads, N, d]
    s = (qh @ kh.transpose(0, 1, 3, 2)) / math.sqrt(d)
    if stats is not None:
        stats[0] = max(stats[0], float((s.max(-1) - s.min(-1)).max()))
    e = np.exp(s - s.max(-1, keepdims=True))
    a = e / e.sum(-1, keepdims=True)
    if stats is not None:
        stats[1] = max(stats[1], float(a.max()))
    o = (a @ vh).transpose(0, 2, 1, 3).reshape(B, Nq, I)
    return _linear(sd, f"{p}.out_proj", o)


def mask_decoder(sd, image_emb_nhwc, sparse, multimask=True, dense=None, prompts=None, inter=None):
    """MaskDecoder.predict_masks on the prompts listed (None: all): image_emb_nhwc [h,w,C], sparse [P,n,C] (embed_points /
    embed_prompts), dense None (no_mask_embed) or [P,h*w,C] (embed_masks) -> (low-res logits [len(prompts), 3 or 1, 4h, 4w],
    iou [len(prompts), 3 or 1]) in float64.  inter: a dict that receives the intermediate tensors."""
    h, w, _ = image_emb_nhwc.shape
    sel = np.arange(len(sparse)) if prompts is None else np.asarray(prompts, dtype=np.int64)
    B = len(sel)
    out_tok = np.concatenate([_w(sd, "mask_decoder.iou_token.weight"), _w(sd, "mask_decoder.mask_tokens.weight")], 0)
    tokens = np.concatenate([np.broadcast_to(out_tok, (B,) + out_tok.shape), np.asarray(sparse, dtype=F64)[sel]], axis=1)
    emb = np.asarray(image_emb_nhwc, dtype=F64).reshape(1, h * w, C)
    if dense is None:
        keys = np.repeat(emb + _w(sd, "prompt_encoder.no_mask_embed.weight").reshape(1, 1, C), B, axis=0)
    else:
        keys = emb + np.asarray(dense, dtype=F64)[sel]
    pos = dense_pe(sd, h, w)[None]
    t = "mask_decoder.transformer"
    stats = [0.0, 0.0]
    queries = tokens
    for i in range(2):
        l = f"{t}.layers.{i}"
        if i == 0:
            queries = _attention(sd, f"{l}.self_attn", queries, queries, queries)
        else:
            qp = queries + tokens
            queries = queries + _attention(sd, f"{l}.self_attn", qp, qp, queries)
        queries = _layer_norm(sd, f"{l}.norm1", queries, 1e-5)
        queries = _layer_norm(sd, f"{l}.norm2", queries + _attention(sd, f"{l}.cross_attn_token_to_image", queries + tokens,
                                                                     keys + pos, keys, stats), 1e-5)
        hid = np.maximum(_linear(sd, f"{l}.mlp.lin1", queries), 0.0)
        queries = _layer_norm(sd, f"{l}.norm3", queries + _linear(sd, f"{l}.mlp.lin2", hid), 1e-5)
        keys = _layer_norm(sd, f"{l}.norm4", keys + _attention(sd, f"{l}.cross_attn_image_to_token", keys + pos, queries + tokens,
                                                               queries), 1e-5)
        if inter is not None:
            inter[f"queries_l{i}"], inter[f"keys_l{i}"] = queries, keys
    queries = queries + _attention(sd, f"{t}.final_attn_token_to_image", queries + tokens, keys + pos, keys, stats)
    queries = _layer_norm(sd, f"{t}.norm_final_attn", queries, 1e-5)

    def conv_t(x, key):     # ConvTranspose2d(k 2, s 2) on [B,H,W,ci], weight [ci,co,2,2] -> [B,2H,2W,co]
        wt = _w(sd, f"mask_decoder.output_upscaling.{key}.weight")
        out = np.empty((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], wt.shape[1]), dtype=F64)
        for ky in range(2):
            for kx in range(2):
                out[:, ky::2, kx::2, :] = x @ wt[:, :, ky, kx]
        return out + _w(sd, f"mask_decoder.output_upscaling.{key}.bias")

    up = _gelu(_layer_norm(sd, "mask_decoder.output_upscaling.1", conv_t(keys.reshape(B, h, w, C), "0"), 1e-6))
    up = _gelu(conv_t(up, "3"))
    hyper = []
    for i in range(4):
        x = queries[:, 1 + i]
        for j in range(3):
            x = _linear(sd, f"mask_decoder.output_hypernetworks_mlps.{i}.layers.{j}", x)
            x = np.maximum(x, 0.0) if j < 2 else x
        hyper.append(x)
    hyper = np.stack(hyper, 1)
    masks = (hyper @ up.reshape(B, 16 * h * w, -1).transpose(0, 2, 1)).reshape(B, 4, 4 * h, 4 * w)      # hyper . upscaled per pixel
    iou = queries[:, 0]
    for j in range(3):
        iou = _linear(sd, f"mask_decoder.iou_prediction_head.layers.{j}", iou)
        iou = np.maximum(iou, 0.0) if j < 2 else iou
    if inter is not None:
        inter.update(queries_final=queries, upscaled=up, hyper=hyper, score_range=stats[0], peak_probability=stats[1])
    return (masks[:, 1:], iou[:, 1:]) if multimask else (masks[:, :1], iou[:, :1])


T2I_ATTENTIONS = ("mask_decoder.transformer.layers.0.cross_attn_token_to_image",
                  "mask_decoder.transformer.layers.1.cross_attn_token_to_image",
                  "mask_decoder.transformer.final_attn_token_to_image")


def stress_decoder(sd, temp):
    """a copy of the state dict with q_proj (weight and bias) of the three token -> image attentions multiplied by temp"""
    assert temp in (1, 4, 16), temp
    out = type(sd)(sd)
    for a in T2I_ATTENTIONS:
        for leaf in ("weight", "bias"):
            out[f"{a}.q_proj.{leaf}"] = (np.asarray(sd[f"{a}.q_proj.{leaf}"]) * F32(temp)).astype(F32)
    return out


# ================================================================================================================ the route
Route = namedtuple("Route", "x3 merged raw_t2i shared plain fuse_i2t chunked fused_tail ns multi")

ATTI_BYTES = 512             # per prompt and image token: DecPlan::atti, [P*HW, C/2] floats
KP_BYTES = 1536              # DecPlan::kp, three such buffers
T2I_FOLDED_BYTES = 56 * C * 8         # Q' as fp16 hi | lo and as floats
T2I_PART_BYTES = (56 * C + 56 * 2) * 4   # one key range's partial rows
I2T_FOLD_BYTES = 56 * C * 4 + 16384 * 4 + 256
FEWQ_PART_BYTES = 16 * 7 * 10 * 4     # per chunk of 256 keys


def key_ranges(ppi, HW):
    return 8 if ppi <= 128 and HW % 256 == 0 else 1


def dec_route(grid, P, n_img=1, n_sparse=2, dense=False, fusion=ALL_FUSED, precision="f16x3"):
    """DecRoute dec_route() of csrc/sam_api.hip for ONE launch sequence of P prompts over n_img images"""
    HW, T, ppi = grid * grid, 5 + n_sparse, P // n_img
    atti = P * HW * ATTI_BYTES
    x3 = precision != "f32"
    merged = x3 and bool(fusion & 2)
    ns = key_ranges(ppi, HW)
    raw = (merged and bool(fusion & 32) and bool(fusion & 4) and T == 7 and HW % 128 == 0 and P <= 65535 and not dense and
           P * T2I_FOLDED_BYTES + n_img * ppi * ns * T2I_PART_BYTES <= atti and P * I2T_FOLD_BYTES <= atti and
           P * 56 * HW * 4 <= P * HW * KP_BYTES)
    shared = (not dense, False)
    plain = (dense, False)
    fuse_i2t = tuple(merged and bool(fusion & 4) and HW % 64 == 0 and P <= 65535 and T == 7 and not plain[li] for li in range(2))
    ch = bool(fusion & 16) and HW >= 256 and P <= 65535 and atti >= P * ((HW + 255) // 256) * FEWQ_PART_BYTES
    fused_tail = x3 and bool(fusion & 1) and HW % 64 == 0 and (grid % 64 == 0 or 64 % grid == 0) and P <= 65535
    return Route(x3, merged, raw, shared, plain, fuse_i2t, (ch, ch, ch), fused_tail, ns, shared[0] and fuse_i2t[0] and ch)


KERNELS = ("dec_tail_kernel", "dec_i2t_kernel", "dec_i2t_fold_kernel", "t2i_fold_q_kernel", "t2i_raw_attn_kernel",
           "t2i_unfold_v_kernel", "i2t_prep_kernel", "hyper_logits_kernel", "ln_gelu64_kernel", "ln256_pe_split_kernel",
           "mask_downscaling_kernel", "attn_fewq_chunk_kernel")


def kernel_id(name):
    """the decoder-specific kernel a launched kernel's name (demangled or Itanium-mangled) stands for, or None.
    abi_ref.launched_kernels reports every '..attn_..kernel' by the part its attention pattern finds: the raw token -> image
    attention arrives as plain 'attn_kernel' (no kernel of csrc/attention*.hip has that name: theirs carry a suffix)"""
    if name == "attn_kernel":
        return "t2i_raw_attn_kernel"
    for k in ("dec_i2t_fold_kernel", "dec_i2t_kernel") + tuple(x for x in KERNELS if not x.startswith("dec_i2t")):
        if k in name:
            return k
    return None


def route_kernels(r, dense):
    """the decoder-specific kernels a launch sequence of route r enqueues (decode_impl, dec_t2i, dec_i2t of csrc/sam_api.hip);
    mask_downscaling_kernel belongs to embed_masks, which the dense cases call inside the watched region"""
    k = set()
    k |= {"dec_tail_kernel"} if r.fused_tail else {"hyper_logits_kernel", "ln_gelu64_kernel"}
    for li in range(2):
        if r.fuse_i2t[li] and r.raw_t2i and not r.shared[li]:
            k |= {"i2t_prep_kernel", "dec_i2t_fold_kernel"}
        elif r.fuse_i2t[li]:
            k.add("dec_i2t_kernel")
        elif r.x3:
            k.add("ln256_pe_split_kernel")
    if r.raw_t2i:
        k |= {"t2i_fold_q_kernel", "t2i_raw_attn_kernel", "t2i_unfold_v_kernel"}
    # the chunked few-query attention: layer 0 always goes through it where it serves; layer 1 and the final one unless raw
    if r.chunked[0] or (r.chunked[1] and not r.raw_t2i):
        k.add("attn_fewq_chunk_kernel")
    if dense:
        k.add("mask_downscaling_kernel")
    return frozenset(k)


# ================================================================================================================ the cases
# kind: "points" (hgl_sam_decode_points: a foreground point + padding), "multi" (hgl_sam_decode_points_multi), "gated"
# (hgl_sam_decode_points_gated), "lab3" / "lab9" (hgl_sam_decode_prompts with three / nine sparse tokens: T = 8 / 14), "dense"
# (box corners + the dense rows of embed_masks).  P: prompts per image.  fusion: the mask handed to hgl_sam_decoder_fusion.
# route: the DecRoute fields (of each launch sequence the call makes) the case is there for; kernels: the decoder-specific
# kernels the call must launch -- every other name of KERNELS must NOT be launched.
Case = namedtuple("Case", "name grid P kind fusion precision n_img first_mask temp route kernels note")

TAIL, I2T, FOLD, PREP = "dec_tail_kernel", "dec_i2t_kernel", "dec_i2t_fold_kernel", "i2t_prep_kernel"
RAW3 = ("t2i_fold_q_kernel", "t2i_raw_attn_kernel", "t2i_unfold_v_kernel")
UNFUSED_TAIL = ("hyper_logits_kernel", "ln_gelu64_kernel")
LN_SPLIT, MASK_DS, CHUNK = "ln256_pe_split_kernel", "mask_downscaling_kernel", "attn_fewq_chunk_kernel"

K_CHUNKED = frozenset({TAIL, I2T, CHUNK})                  # grid 16 / 32 by default: everything fused but the raw attention
K_RAW = frozenset({TAIL, I2T, FOLD, PREP, CHUNK, *RAW3})   # layer 0 chunked + dec_i2t, layer 1 and the final attention raw
K_F32 = frozenset({*UNFUSED_TAIL, CHUNK})                  # fp32 launches; the chunked attention is precision-independent
K_DENSE = frozenset({MASK_DS, LN_SPLIT, I2T, CHUNK, TAIL})
NOT_RAW = dict(raw_t2i=False, merged=True, fuse_i2t=(True, True), chunked=(True, True, True), fused_tail=True)
RAW = dict(raw_t2i=True, merged=True, fuse_i2t=(True, True), chunked=(True, True, True), fused_tail=True)


def _case(name, grid, P, kernels, route, note, kind="points", fusion=ALL_FUSED, precision="f16x3", n_img=1, first_mask=1, temp=1):
    return Case(name, grid, P, kind, fusion, precision, n_img, first_mask, temp, route, frozenset(kernels), note)


def _cases():
    c = [
        _case("g8", 8, 5, {TAIL, I2T}, dict(chunked=(False,) * 3, raw_t2i=False, fuse_i2t=(True, True), fused_tail=True, multi=False),
              "HW 64: general attention for the tokens, one dec_i2t tile = the image, a tail tile spans 8 grid rows"),
        _case("g12", 12, 5, {*UNFUSED_TAIL, LN_SPLIT},
              dict(chunked=(False,) * 3, raw_t2i=False, merged=True, fuse_i2t=(False, False), fused_tail=False, multi=False),
              "HW 144, no multiple of 64: merged projection with q from kvq, general attention writes the split planes"),
        _case("g16_p5", 16, 5, K_CHUNKED, dict(NOT_RAW, ns=8, multi=True),
              "ns = 8 computed, raw_t2i off by the capacity of atti (module docstring)"),
        _case("g16_p129", 16, 129, K_CHUNKED, dict(NOT_RAW, ns=1, multi=True), "first prompt count with one key range; raw_t2i off by capacity"),
        _case("g16_multi3x5", 16, 5, K_CHUNKED, dict(NOT_RAW, multi=True, ns=8), "three images in one launch sequence", kind="multi", n_img=3),
        _case("g16_multi2x129", 16, 129, K_CHUNKED, dict(NOT_RAW, multi=True, ns=1), "two images of 129 prompts", kind="multi", n_img=2),
    ]
    fus = {0: ({*UNFUSED_TAIL, LN_SPLIT}, dict(merged=False, fuse_i2t=(False, False), chunked=(False,) * 3, fused_tail=False)),
           1: ({TAIL, LN_SPLIT}, dict(merged=False, fuse_i2t=(False, False), chunked=(False,) * 3, fused_tail=True)),
           3: ({TAIL, LN_SPLIT}, dict(merged=True, fuse_i2t=(False, False), chunked=(False,) * 3, fused_tail=True)),
           7: ({TAIL, I2T}, dict(merged=True, fuse_i2t=(True, True), chunked=(False,) * 3, fused_tail=True)),
           23: (K_CHUNKED, dict(NOT_RAW)),
           55: (K_CHUNKED, dict(NOT_RAW))}
    for f, (k, r) in fus.items():
        c.append(_case(f"g16_fusion{f}", 16, 6, k, dict(r, raw_t2i=False, x3=True), "fusion mask against the reference directly", fusion=f))
    c += [
        _case("g64_fusion23", 64, 4, K_CHUNKED, dict(NOT_RAW), "the merged + chunked route at a grid where 55 differs from it", fusion=23),
        _case("g16_f32", 16, 5, K_F32, dict(x3=False, merged=False, raw_t2i=False, fuse_i2t=(False, False), fused_tail=False, multi=False),
              "f32 mode: the plain launches throughout", precision="f32"),
        _case("g12_f32", 12, 5, UNFUSED_TAIL, dict(x3=False, chunked=(False,) * 3), "f32 mode below one chunk of keys", precision="f32"),
        _case("g16_first0", 16, 5, K_CHUNKED, dict(fused_tail=True), "first_mask = 0 through the fused tail", kind="lab2", first_mask=0),
        _case("g24_first0", 24, 4, {I2T, CHUNK, *UNFUSED_TAIL}, dict(fused_tail=False), "first_mask = 0 through hyper_logits", kind="lab2",
              first_mask=0),
        _case("g16_gated", 16, 8, K_CHUNKED, dict(fused_tail=True), "the IoU gate skips some prompts in the fused tail", kind="gated"),
        _case("g24_gated", 24, 8, {I2T, CHUNK, *UNFUSED_TAIL}, dict(fused_tail=False), "the IoU gate with the unfused tail (no skip there)",
              kind="gated"),
        _case("g16_dense", 16, 4, K_DENSE, dict(plain=(True, False), shared=(False, False), fuse_i2t=(False, True), raw_t2i=False, multi=False),
              "per-prompt image tokens from layer 0: plain[0], then merged + dec_i2t + chunks", kind="dense"),
        _case("g32_dense", 32, 3, K_DENSE, dict(plain=(True, False), shared=(False, False), fuse_i2t=(False, True), raw_t2i=False, multi=False),
              "the same at HW 1024", kind="dense"),
        _case("g16_lab3", 16, 4, {TAIL, LN_SPLIT, CHUNK}, dict(fuse_i2t=(False, False), raw_t2i=False, merged=True, multi=False),
              "T = 8, multimask", kind="lab3"),
        _case("g16_lab3_single", 16, 4, {TAIL, LN_SPLIT, CHUNK}, dict(fuse_i2t=(False, False)), "T = 8, single mask", kind="lab3", first_mask=0),
        _case("g24_lab3_single", 24, 4, {*UNFUSED_TAIL, LN_SPLIT, CHUNK}, dict(fuse_i2t=(False, False), fused_tail=False),
              "T = 8 over a ragged chunk, single mask", kind="lab3", first_mask=0),
        _case("g24_lab9", 24, 3, {*UNFUSED_TAIL, LN_SPLIT, CHUNK}, dict(fuse_i2t=(False, False), raw_t2i=False, fused_tail=False),
              "T = 14: queries 7 at a time, multimask", kind="lab9"),
        _case("g16_lab9_single", 16, 3, {TAIL, LN_SPLIT, CHUNK}, dict(fuse_i2t=(False, False)), "T = 14, single mask", kind="lab9", first_mask=0),
        _case("g24", 24, 9, {I2T, CHUNK, *UNFUSED_TAIL},
              dict(raw_t2i=False, fuse_i2t=(True, True), chunked=(True,) * 3, fused_tail=False, multi=True),
              "HW 576: ragged last chunk of 64 keys, a dec_i2t tile spans 2 2/3 grid rows, no fused tail"),
        _case("g32", 32, 5, K_CHUNKED, dict(NOT_RAW, ns=8, multi=True),
              "HW 1024: a tail tile covers two grid rows; raw_t2i off (eight key ranges do not fit atti)"),
        _case("raw32_p129", 32, 129, K_RAW, dict(RAW, ns=1, multi=True),
              "raw_t2i with ONE key range of 32 chunks; dec_i2t_fold with 8 tiles a prompt"),
        _case("raw48", 48, 5, {*(K_RAW - {TAIL}), *UNFUSED_TAIL}, dict(RAW, fused_tail=False, ns=8, multi=True),
              "smallest grid with eight key ranges (9 chunks each); 18 fold tiles; 64 % 48 != 0: the unfused tail"),
        _case("raw48_multi3x5", 48, 5, {*(K_RAW - {TAIL}), *UNFUSED_TAIL}, dict(RAW, fused_tail=False, ns=8, multi=True),
              "the raw route over three images: per-set partials", kind="multi", n_img=3),
        _case("raw32_multi2x129", 32, 129, K_RAW, dict(RAW, ns=1, multi=True), "the raw route with one key range over two images", kind="multi",
              n_img=2),
        _case("g64_p7", 64, 7, K_RAW, dict(RAW, ns=8, multi=True), "the production grid, 16 chunks per key range"),
        _case("g64_p64", 64, 64, K_RAW, dict(RAW, ns=8, multi=True), "the production grid and batch"),
        _case("g128_p2", 128, 2, K_RAW, dict(RAW, ns=8, multi=True),
              "HW 16384: a tail tile is half a grid row, 64 chunks per key range; the capacities hold (atti 8 MB a prompt against "
              "577 024 bytes; were they not to, the route would be g32's: K_CHUNKED)"),
        _case("g8_multi2", 8, 5, {TAIL, I2T}, dict(multi=False, chunked=(False,) * 3), "not multi: image by image", kind="multi", n_img=2),
        _case("g12_multi2", 12, 5, {*UNFUSED_TAIL, LN_SPLIT}, dict(multi=False, fuse_i2t=(False, False)), "not multi: image by image",
              kind="multi", n_img=2),
    ]
    for temp in (4, 16):
        c += [
            _case(f"g16_p5_t{temp}", 16, 5, K_CHUNKED, dict(NOT_RAW, ns=8), "stress: chunked route", temp=temp),
            _case(f"g16_p129_t{temp}", 16, 129, K_CHUNKED, dict(NOT_RAW, ns=1), "stress: chunked route", temp=temp),
            _case(f"g32_t{temp}", 32, 5, K_CHUNKED, dict(NOT_RAW, ns=8), "stress: four chunks of 256 keys", temp=temp),
            _case(f"g24_t{temp}", 24, 9, {I2T, CHUNK, *UNFUSED_TAIL}, dict(raw_t2i=False, chunked=(True,) * 3), "stress: ragged chunk", temp=temp),
            _case(f"raw32_p129_t{temp}", 32, 129, K_RAW, dict(RAW, ns=1), "stress: raw attention, one key range", temp=temp),
            _case(f"raw48_t{temp}", 48, 5, {*(K_RAW - {TAIL}), *UNFUSED_TAIL}, dict(RAW, fused_tail=False, ns=8),
                  "stress: raw attention, eight key ranges joined by t2i_unfold_v", temp=temp),
        ]
    return c


CASES = _cases()
N_SPARSE = {"points": 2, "multi": 2, "gated": 2, "lab2": 2, "lab3": 3, "lab9": 9, "dense": 2}


def launch_shape(c):
    """(P, n_img) of each launch sequence the call of case c makes: the multi route serves all images at once, otherwise the
    call goes image by image (dec_multi_images / decode_multi of csrc/sam_api.hip)"""
    if c.n_img > 1 and dec_route(c.grid, c.n_img * c.P, c.n_img, 2, False, c.fusion, c.precision).multi:
        return c.n_img * c.P, c.n_img
    return c.P, 1


def case_route(c):
    P, n_img = launch_shape(c)
    return dec_route(c.grid, P, n_img, N_SPARSE[c.kind], c.kind == "dense", c.fusion, c.precision)


def checked_prompts(P):
    """first, last and two in between (all of them up to four)"""
    return sorted({0, P // 3, (2 * P) // 3, P - 1})


# =============================================================================================================== the inputs
def case_inputs(c):
    """seeded inputs of case c: emb [n_img, g, g, C] standard normal fp32; per kind the prompt arrays in PIXELS of an image of
    16 * grid (pts [n_img * P, 2], or co [P, n, 2] + lab [P, n]); mask_in [P, 1, 4g, 4g] for the dense kind.  The first point of
    an image's first prompt is the corner (0, 0), of its last prompt the corner (size - 1, size - 1)."""
    g, size = c.grid, 16 * c.grid
    rng = np.random.default_rng([c.grid, c.P, c.n_img, N_SPARSE[c.kind]])
    out = dict(size=size, emb=rng.standard_normal((c.n_img, g, g, C)).astype(F32))
    n_pts = c.n_img * c.P
    pts = np.floor(rng.random((n_pts, 2)) * size).astype(F64)
    for img in range(c.n_img):      # the first and the last prompt of every image are checked: the two corners go there
        pts[img * c.P], pts[(img + 1) * c.P - 1] = (0.0, 0.0), (size - 1.0, size - 1.0)
    if c.kind in ("points", "multi", "gated"):
        out["pts"] = pts
        return out
    n = N_SPARSE[c.kind]
    co = np.floor(rng.random((c.P, n, 2)) * size).astype(F64)
    co[:, 0] = pts
    if c.kind == "dense":      # box corners: top-left, bottom-right
        co = np.sort(co, axis=1)
        lab = np.tile(np.array([2, 3]), (c.P, 1))
        out["mask_in"] = (4.0 * rng.standard_normal((c.P, 1, 4 * g, 4 * g))).astype(F32)
    elif c.kind == "lab2":     # a labelled point + padding
        lab = np.stack([rng.integers(0, 2, c.P), np.full(c.P, -1)], 1)
        co[:, 1] = 0.0
    else:                      # labelled points, the last token padding; prompt 0 ends in a box instead
        lab = np.concatenate([rng.integers(0, 2, (c.P, n - 1)), np.full((c.P, 1), -1)], 1)
        co[:, -1] = 0.0
        lab[0, -2:] = (2, 3)
        co[0, -2:] = np.sort(np.floor(rng.random((2, 2)) * size), axis=0)
    out["co"], out["lab"] = co, lab.astype(np.int64)
    return out
