"""GPU: the SAM mask decoder on every route of dec_route() (csrc/sam_api.hip) against the float64 reference of
tests/decoder_cases.py -- one test per row of decoder_cases.CASES, which names the shape, the DecRoute fields the row is there
for and the decoder-specific kernels its route must launch (every other one of decoder_cases.KERNELS must not run).

Each case:
  * low-res logits and IoU predictions of the first, the last and two prompts in between (of every image, for the multi-image
    calls) against the float64 reference.  The bar is 16 * e32, where e32 is the largest difference between the fp32 oracle
    (oracle/sam_oracle.py) and the float64 reference on the same prompts, computed in the test for the logits and for the IoU
    rows separately (the IoU head's own e32 is a tenth of the logits': one e32 for both would leave its bar ten times too wide).
    Why 16: a split-fp16 product carries about 2^-22, four times fp32's 2^-24, and exponentials in base 2 and re-associated LayerNorm
    sums get another factor of four.  The bar never exceeds the one tests/test_gpu_sam.py has for the same quantity
    (2e-4 * max(1, |ref|) on the logits, 1e-4 on the IoU rows).  Worst error, e32 and their ratio are printed first.
  * the decoder-specific kernels launched are exactly the set the table lists: a silent change of route fails.
  * a second call gives the same bits; ops.split_overflow_count() is 0 afterwards (the stress cases included).
  * multi-image calls: every row equals the row of its image's own call bit for bit, on the multi route and on the
    image-by-image fall-back alike.
  * gated calls: the gate sits in the widest gap of the reference's best IoU per prompt; the IoU rows of all prompts and the
    logits of the kept ones are checked.

Route fields per case: decoder_cases.CASES (`route`, `kernels`, `note`), held against the restated dec_route by
tests/test_decoder_cases_host.py.  DecRoute values the table cannot reach: fuse_i2t = (True, False) (layer 1 is never plain);
chunked with different values per attention (one condition serves all three with this decoder's widths); x3 with C != 256 or an
unregistered weight, merged off by weight geometry (sam.py registers all of them); any P > 65535 condition (a test of that
size is no few-seconds test).

MEASURED on an MI355X (multi-image cases: the image with the largest ratio).  Every ratio is at most 1.79: on every route
the decoder is as close to float64 as the fp32 oracle is, the stress cases included; no case needed a multiple of its own.

  case               logits: err  e32  ratio   IoU: err  e32  ratio
  g8                 3.7e-06 4.1e-06  0.89   4.6e-07 5.3e-07  0.88
  g12                5.1e-06 6.0e-06  0.84   4.7e-07 5.3e-07  0.89
  g16_p5             3.4e-06 4.4e-06  0.76   2.4e-07 5.9e-07  0.41
  g16_p129           4.0e-06 5.7e-06  0.71   2.4e-07 2.7e-07  0.90
  g16_multi3x5       3.3e-06 4.6e-06  0.71   3.0e-07 3.2e-07  0.95
  g16_multi2x129     3.2e-06 4.4e-06  0.73   3.4e-07 4.1e-07  0.82
  g16_fusion0        5.1e-06 5.0e-06  1.03   4.2e-07 2.6e-07  1.58
  g16_fusion1        5.4e-06 5.0e-06  1.08   4.2e-07 2.6e-07  1.58
  g16_fusion3        4.6e-06 5.0e-06  0.93   3.8e-07 2.6e-07  1.45
  g16_fusion7        4.2e-06 5.0e-06  0.84   4.7e-07 2.6e-07  1.79
  g16_fusion23       3.9e-06 5.0e-06  0.79   2.9e-07 2.6e-07  1.09
  g16_fusion55       3.9e-06 5.0e-06  0.79   2.9e-07 2.6e-07  1.09
  g64_fusion23       4.9e-06 9.4e-06  0.52   3.5e-07 9.0e-07  0.39
  g16_f32            5.2e-06 4.4e-06  1.18   4.5e-07 5.9e-07  0.76
  g12_f32            5.9e-06 6.0e-06  0.97   6.6e-07 5.3e-07  1.25
  g16_first0         3.0e-06 4.5e-06  0.65   2.2e-07 3.9e-07  0.56
  g24_first0         2.7e-06 4.0e-06  0.68   3.5e-07 4.5e-07  0.78
  g16_gated          3.0e-06 6.4e-06  0.47   3.7e-07 8.5e-07  0.44
  g24_gated          3.6e-06 5.8e-06  0.62   5.5e-07 9.4e-07  0.59
  g16_dense          3.5e-06 6.1e-06  0.58   6.9e-07 6.4e-07  1.08
  g32_dense          4.3e-06 5.0e-06  0.87   4.8e-07 4.9e-07  0.98
  g16_lab3           4.8e-06 5.1e-06  0.93   4.0e-07 5.1e-07  0.78
  g16_lab3_single    2.6e-06 3.8e-06  0.69   2.1e-07 7.6e-07  0.27
  g24_lab3_single    3.1e-06 4.5e-06  0.69   1.1e-07 6.1e-07  0.18
  g24_lab9           4.3e-06 5.2e-06  0.83   4.9e-07 6.4e-07  0.77
  g16_lab9_single    2.9e-06 3.4e-06  0.84   2.6e-07 5.2e-07  0.50
  g24                3.6e-06 5.7e-06  0.63   3.5e-07 2.9e-07  1.19
  g32                3.9e-06 5.8e-06  0.67   4.2e-07 4.5e-07  0.95
  raw32_p129         4.4e-06 5.7e-06  0.77   5.2e-07 5.4e-07  0.97
  raw48              4.3e-06 7.6e-06  0.56   3.4e-07 5.0e-07  0.68
  raw48_multi3x5     4.5e-06 7.0e-06  0.64   7.0e-07 9.8e-07  0.71
  raw32_multi2x129   4.9e-06 6.3e-06  0.77   5.3e-07 6.0e-07  0.89
  g64_p7             4.4e-06 8.2e-06  0.53   4.7e-07 1.0e-06  0.45
  g64_p64            4.2e-06 9.6e-06  0.44   4.2e-07 1.2e-06  0.35
  g128_p2            4.8e-06 5.0e-06  0.96   2.7e-07 3.0e-07  0.92
  g8_multi2          2.8e-06 3.9e-06  0.71   2.9e-07 3.0e-07  0.95
  g12_multi2         3.7e-06 4.7e-06  0.79   5.4e-07 6.3e-07  0.86
  g16_p5_t4          6.0e-06 8.5e-06  0.71   6.4e-07 8.4e-07  0.76
  g16_p129_t4        5.1e-06 7.0e-06  0.73   7.9e-07 6.6e-07  1.20
  g32_t4             8.1e-06 1.3e-05  0.62   7.2e-07 7.8e-07  0.92
  g24_t4             5.8e-06 9.7e-06  0.59   5.7e-07 1.2e-06  0.47
  raw32_p129_t4      5.4e-06 1.2e-05  0.44   8.5e-07 1.1e-06  0.77
  raw48_t4           6.6e-06 1.4e-05  0.48   9.3e-07 1.9e-06  0.49
  g16_p5_t16         2.2e-05 5.3e-05  0.42   2.1e-06 2.4e-06  0.89
  g16_p129_t16       1.3e-05 2.7e-05  0.48   2.5e-06 2.6e-06  0.97
  g32_t16            2.0e-05 5.0e-05  0.41   5.1e-06 5.6e-06  0.92
  g24_t16            2.3e-05 4.9e-05  0.47   2.4e-06 2.7e-06  0.88
  raw32_p129_t16     1.6e-05 3.7e-05  0.43   2.4e-06 5.3e-06  0.46
  raw48_t16          2.5e-05 4.8e-05  0.52   5.1e-06 4.8e-06  1.06
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_ref
import decoder_cases as D
from hybridgl_amd import _lib, ops
from hybridgl_amd import sam as hsam
from hybridgl_amd import weights
from oracle import sam_oracle as S

pytestmark = pytest.mark.gpu

MULTIPLE = 16
HGL_EINVAL, HGL_EWORKSPACE = -1, -3


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fusion(mask):
    return _lib.load().hgl_sam_decoder_fusion(mask)


def _model(c, dev):
    cfg = D.encoder_cfg(c.grid)
    sd = D.stress_decoder(weights.sam_state_dict(cfg, 0), c.temp)
    return sd, hsam.Sam(sd, cfg, dev, precision=c.precision)


def _device_inputs(c, inp, dev):
    g, size = c.grid, inp["size"]
    d = dict(emb=T(inp["emb"].reshape(c.n_img, g * g, D.C), dev))
    if "pts" in inp:
        d["p01"] = T(D.coords01(inp["pts"], size), dev)
    else:
        d["c01"], d["lab"] = T(D.coords01(inp["co"], size), dev), T(inp["lab"].astype(np.int32), dev)
    if "mask_in" in inp:
        d["mask_in"] = T(inp["mask_in"], dev)
    return d


def _call(m, c, d, gate=None):
    """the entry point of the case's kind -> (low_res, iou) device tensors"""
    if c.kind == "multi":
        return m.decode_points_multi(d["emb"], d["p01"], c.n_img)
    if c.kind in ("points", "gated"):
        return m.decode_points(d["emb"][0], d["p01"], iou_gate=gate)
    dense = m.embed_masks(d["mask_in"]) if c.kind == "dense" else None
    return m.decode_prompts(d["emb"][0], d["c01"], d["lab"], first_mask=c.first_mask, dense=dense)


def _references(c, sd, inp, img, sel):
    """float64 reference and fp32 oracle of image img on the prompts sel (indices within the image) -> (low, iou) twice"""
    size, mm = inp["size"], c.first_mask == 1
    if "pts" in inp:
        pts = inp["pts"][img * c.P:(img + 1) * c.P]
        s64, s32 = D.embed_points(sd, pts, size), S.embed_points(sd, pts, size)
    else:
        s64, s32 = D.embed_prompts(sd, inp["co"], inp["lab"], size), S.embed_prompts(sd, inp["co"], inp["lab"], size)
    d64 = d32 = None
    if "mask_in" in inp:      # the rows of the checked prompts only, in their order
        d64, d32 = D.embed_masks(sd, inp["mask_in"][sel]), S.embed_masks(sd, inp["mask_in"][sel])
        full = np.zeros((c.P,) + d64.shape[1:])
        full[sel] = d64
        d64 = full
    ref = D.mask_decoder(sd, inp["emb"][img], s64, multimask=mm, dense=d64, prompts=sel)
    orc = S.mask_decoder(sd, inp["emb"][img], s32[sel], multimask=mm, dense=d32)
    return ref, orc


def _judge(name, got_low, got_iou, ref, orc, rows=None):
    """prints worst error, e32 and the ratio of either output; returns (within the bars, the figures).  rows: the prompts whose
    logits count (None: all)"""
    (rlow, riou), (olow, oiou) = ref, orc
    rows = np.arange(len(rlow)) if rows is None else rows
    e32_low, e32_iou = float(np.abs(olow - rlow).max()), float(np.abs(oiou - riou).max())
    elow = float(np.abs(got_low[rows] - rlow[rows]).max())
    eiou = float(np.abs(got_iou - riou).max())
    scale = float(np.abs(rlow).max())
    bar_low, bar_iou = min(MULTIPLE * e32_low, 2e-4 * max(1.0, scale)), min(MULTIPLE * e32_iou, 1e-4)
    print(f"decoder route {name}: logits err {elow:.3e} e32 {e32_low:.3e} ratio {elow / e32_low:.2f} | iou err {eiou:.3e} "
          f"e32 {e32_iou:.3e} ratio {eiou / e32_iou:.2f} (max |logit| {scale:.2f}, bars {bar_low:.3e} / {bar_iou:.3e})")
    assert np.isfinite(got_low[rows]).all() and np.isfinite(got_iou).all()
    return elow <= bar_low and eiou <= bar_iou, (name, elow, bar_low, eiou, bar_iou)


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_decoder_route_vs_float64_reference(cuda, c):
    old = _fusion(-1)
    m = None
    try:
        _fusion(c.fusion)
        sd, m = _model(c, cuda)
        inp = D.case_inputs(c)
        d = _device_inputs(c, inp, cuda)
        ops.split_overflow_count()
        k = 1 if c.first_mask == 1 else 0          # first_mask 0: column 0 is the single-mask output
        cols = slice(0, 3) if k else slice(0, 1)
        gate, kept = None, None
        if c.kind == "gated":
            # the reference's best prediction per prompt, ALL prompts; the gate in the middle of the widest gap between them
            sel = list(range(c.P))
            ref, orc = _references(c, sd, inp, 0, sel)
            best = np.sort(ref[1].max(1))
            i = int(np.argmax(np.diff(best)))
            gate = float(0.5 * (best[i] + best[i + 1]))
            kept = ref[1].max(1) > gate
            assert best[i + 1] - best[i] > 1e-3 and 0 < kept.sum() < c.P, (best, gate)
        out = {}
        names = abi_ref.launched_kernels(lambda: out.setdefault("r", _call(m, c, d, gate)))
        low, iou = (t.cpu().numpy() for t in out["r"])
        ran = {D.kernel_id(n) for n in names} - {None}
        print(f"decoder route {c.name}: kernels {sorted(ran)}")
        assert ran == set(c.kernels), (sorted(ran), sorted(c.kernels))
        assert low.shape == (c.n_img * c.P, 3, 4 * c.grid, 4 * c.grid) and iou.shape == (c.n_img * c.P, 3)

        verdicts = []
        if c.kind == "gated":
            assert np.array_equal((iou > gate).any(1), kept)
            verdicts.append(_judge(c.name, low[:, cols], iou[:, cols], ref, orc, rows=np.flatnonzero(kept)))
        else:
            sel = D.checked_prompts(c.P)
            for img in range(c.n_img):
                ref, orc = _references(c, sd, inp, img, sel)
                rows = [img * c.P + s for s in sel]
                verdicts.append(_judge(f"{c.name}[image {img}]" if c.n_img > 1 else c.name, low[rows][:, cols], iou[rows][:, cols], ref, orc))

        low2, iou2 = (t.cpu().numpy() for t in _call(m, c, d, gate))          # run to run: the same bits
        live = slice(None) if kept is None else kept
        assert np.array_equal(iou2, iou) and np.array_equal(low2[live], low[live])
        if c.kind == "multi":          # every image's rows == its own call's, whichever way the launch went
            for img in range(c.n_img):
                l1, i1 = m.decode_points(d["emb"][img], d["p01"][img * c.P:(img + 1) * c.P].contiguous())
                assert torch.equal(i1, out["r"][1][img * c.P:(img + 1) * c.P]), img
                assert torch.equal(l1, out["r"][0][img * c.P:(img + 1) * c.P]), img
        assert ops.split_overflow_count() == 0
        for ok, what in verdicts:
            assert ok, what
    finally:
        _fusion(old)
        ops.set_precision(ops.default_precision())
        del m
        torch.cuda.empty_cache()


def test_decoder_error_returns_leave_the_outputs_alone(cuda):
    """hgl_sam_decode_prompts through ctypes: 1 and 12 sparse tokens -> HGL_EINVAL, a workspace one byte short -> HGL_EWORKSPACE;
    the pre-filled outputs keep their bits; the full workspace then decodes"""
    c = next(x for x in D.CASES if x.name == "g16_p5")
    m = None
    try:
        sd, m = _model(c, cuda)
        lib = _lib.load()
        g, P = c.grid, 3
        emb = T(np.random.default_rng(0).standard_normal((g * g, D.C)).astype(np.float32), cuda)
        low = torch.full((P, 3, 4 * g, 4 * g), -7777.25, dtype=torch.float32, device=cuda)
        iou = torch.full((P, 3), -7777.25, dtype=torch.float32, device=cuda)
        need = lib.hgl_sam_decode_workspace_bytes(C.byref(m.dec_w), P)
        ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
        ops.use_precision(m.precision)

        def call(n, ws_bytes):
            co = torch.full((P, n, 2), 0.5, dtype=torch.float32, device=cuda)
            lab = torch.ones((P, n), dtype=torch.int32, device=cuda)
            rc = lib.hgl_sam_decode_prompts(C.byref(m.dec_w), emb.data_ptr(), co.data_ptr(), lab.data_ptr(), n, None, 1, P,
                                            low.data_ptr(), iou.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
            torch.cuda.synchronize()
            return rc

        for n, ws_bytes, want in ((1, need, HGL_EINVAL), (12, need, HGL_EINVAL), (2, need - 1, HGL_EWORKSPACE)):
            assert call(n, ws_bytes) == want, (n, ws_bytes)
            assert bool((low == -7777.25).all()) and bool((iou == -7777.25).all()), (n, ws_bytes)
        assert call(2, need) == 0
        assert bool(torch.isfinite(low).all()) and not bool((iou == -7777.25).any())
    finally:
        ops.set_precision(ops.default_precision())
        del m
        torch.cuda.empty_cache()
