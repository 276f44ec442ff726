"""The fused mask post-processing (csrc/sam_glue.hip: hgl_sam_postprocess) on every kernel path and tile route, against the
float64-blend reference of tests/post_cases.py (cases, reference and checker are checked on the CPU by
tests/test_post_cases_host.py, which also proves which route each geometry takes).

Routes: the shared-table kernel and the per-pixel kernel (every shared-table geometry runs once more with HGL_SAM_POST_SEP=0,
which puts the per-pixel kernel on the downscaling ratios), each with the XCD tile remap on (K = 16, K = 8 where a launch has
one tile per candidate) and off (K = 15); per-pixel tiles staged in LDS, read from global memory, and both in one launch; the
16-byte store and the bytewise stores; the IoU filter on and off; stability offsets 1.0 and 0.1; with and without the logits.

Every call is judged twice over: the production configuration (no logits) by the checker, which needs none; the call with
logits by the logits themselves (within tol = 2^-20 max|low_res| of the reference) with masks, boxes, stability and keep as
exact functions of them, and its four production outputs bit-equal to the call without.  Every call is made twice and must
repeat itself bit for bit (the counters are atomics), and the K = 15 / K = 8 results must equal the K = 16 ones on their common
candidates bit for bit: remap off against remap on.
"""
import functools
import os

import numpy as np
import pytest
import torch

import post_cases as P
from hybridgl_amd import _lib, ops
from hybridgl_amd import sam as hsam
from hybridgl_amd import weights

pytestmark = pytest.mark.gpu
HGL_EWORKSPACE = -3
ENV = "HGL_SAM_POST_SEP"

# (geometry, per-pixel kernel forced): a shared-table geometry and its forced twin are neighbours, so they share one reference
ROUTES = [(g, forced) for g in P.GEOMS for forced in ((False, True) if g.kernel == "sep" else (False,))]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def sam(cuda):
    """one model for the module: post-processing does not depend on the precision mode"""
    return hsam.Sam(weights.sam_state_dict("tiny", 0), weights.SAM_CONFIGS["tiny"], cuda)


@functools.lru_cache(maxsize=1)
def world(gid):
    """the K = 16 batch of a geometry, its reference and the bounds per stability offset: computed once, never changed"""
    g = next(g for g in P.GEOMS if P.geom_id(g) == gid)
    names, low = P.planes(g)
    ref = P.reference(low, g.inp, g.orig, g.S)
    tol = P.tolerance(low)
    return names, low, ref, tol, {off: P.Bounds(ref, tol, off) for off in sorted({p.off for p in P.PARAMS})}


def same(x, y):
    """bit for bit (a NaN equals a NaN)"""
    if x.is_floating_point():
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    return torch.equal(x, y)


def twice(m, what, *args):
    """every call is made twice: the results must be bit-identical -> the four production outputs"""
    a, b = m.postprocess(*args), m.postprocess(*args)
    assert a[4] is None and b[4] is None
    for name, x, y in zip(("masks", "boxes", "stability", "keep"), a, b):
        assert same(x, y), (what, name, "is not reproducible")
    return a[:4]


def run_geometry(m, cuda, g, forced):
    """every batch size x parameter set of one geometry on one kernel -> list of (geometry, kernel, K, parameters, pattern,
    quantity, detail ...) that are wrong"""
    gid = P.geom_id(g)
    _, _, ref16, tol, bounds = world(gid)
    kern = "per-pixel (forced)" if forced else {"sep": "shared-table", "pix": "per-pixel"}[g.kernel]
    bad = []
    got16 = {}
    for K in P.batch_sizes(g):
        names, low, idx = P.batch(g, K)
        idx = list(idx)
        iou = P.IOU16[idx]
        low_t, iou_t = T(low, cuda), T(iou, cuda)
        for p in P.PARAMS:
            tag = (gid, kern, K, p.name)
            alive = P.passes_iou(iou, p.iou_thr)
            live_t = T(alive, cuda)
            args = (low_t, iou_t, g.inp, g.orig, p.iou_thr, p.stab_thr, p.off)
            # the production configuration: no logits; judged by the checker alone
            prod = twice(m, tag, *args)
            masks, boxes, stab, keep = (t.cpu().numpy() for t in prod)
            bad += [tag + t for t in P.check_outputs(bounds[p.off].take(idx), names, masks, boxes, stab, keep, iou, p)]
            # with logits: they are within tol of the reference, everything else is an exact function of them, and the four
            # production outputs do not change
            out = m.postprocess(*args, return_logits=True)
            again = m.postprocess(*args, return_logits=True)
            for name, x, y, z in zip(("masks", "boxes", "stability", "keep"), out, again, prod):
                if not same(x, y):
                    bad.append(tag + ("*", name, "with logits: not reproducible"))
                if not same(x, z):
                    bad.append(tag + ("*", name, "differs between the calls with and without logits"))
            if not same(out[4][live_t], again[4][live_t]):
                bad.append(tag + ("*", "logits", "not reproducible"))
            full = out[4].cpu().numpy()
            full[~alive] = 0                                       # never written for a filtered candidate
            want = P.outputs_from_logits(full, iou, p)
            for k, n in enumerate(names):
                if alive[k]:
                    err = float(np.abs(full[k] - ref16[idx[k]]).max())
                    if not err <= tol:
                        bad.append(tag + (n, "logits", err, tol))
                for name, x, y in zip(("mask of its logits", "box of its logits", "stability of its logits", "keep of its logits"),
                                      (masks, boxes, stab, keep), want):
                    if not np.array_equal(x[k], y[k], equal_nan=name.startswith("stab")):
                        bad.append(tag + (n, name, np.asarray(x[k]).ravel()[:4].tolist(), np.asarray(y[k]).ravel()[:4].tolist()))
            # remap off (K = 15) and the one-tile launches (K = 8) against remap on (K = 16), on the common candidates
            if K == 16:
                got16[p.name] = prod + (out[4],)
            else:
                sel = torch.tensor(idx, device=cuda)
                for name, x, y in zip(("masks", "boxes", "stability", "keep"), prod, got16[p.name]):
                    if not same(x, y[sel]):
                        bad.append(tag + ("*", name, "differs from the K = 16 launch"))
                if not same(out[4][live_t], got16[p.name][4][sel][live_t]):
                    bad.append(tag + ("*", "logits", "differ from the K = 16 launch"))
    return bad


@pytest.mark.parametrize("g,forced", ROUTES, ids=[P.geom_id(g) + ("-perpixel" if f else "") for g, f in ROUTES])
def test_postprocess_route_against_the_reference(cuda, sam, g, forced):
    assert float(sam.mask_threshold) == P.MASK_THRESHOLD            # the threshold the reference and the checker assume
    old_img, old_env = sam.img_size, os.environ.get(ENV)
    try:
        sam.img_size = g.S
        if forced:
            os.environ[ENV] = "0"
        else:
            os.environ.pop(ENV, None)
        bad = run_geometry(sam, cuda, g, forced)
    finally:
        sam.img_size = old_img
        if old_env is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old_env
    assert not bad, f"{len(bad)} wrong (geometry, kernel, K, parameters, pattern, quantity): {bad[:12]}"


def test_bad_arguments_are_refused_loudly(cuda, sam):
    """K = 65536 (gridDim.z holds 65535), an input size beyond the S x S plane, a workspace one byte short: each is an error
    before the first launch, and the outputs keep what they held"""
    one = torch.zeros((65536, 1, 1), dtype=torch.float32, device=cuda)
    with pytest.raises(_lib.HybridGLError, match="bad shape"):
        sam.postprocess(one, torch.ones(65536, device=cuda), (1, 1), (1, 1))
    g = P.GEOMS[2]
    names, low, _ = P.batch(g, 8)
    low_t, iou_t = T(low, cuda), T(P.IOU16[list(P.PICK8)], cuda)
    assert sam.img_size == g.S
    for inp in ((g.S + 1, g.S), (g.S, g.S + 1)):
        with pytest.raises(_lib.HybridGLError, match="bad shape"):
            sam.postprocess(low_t, iou_t, inp, g.orig)
    sam.postprocess(low_t, iou_t, (g.S, g.S), g.orig)                 # exactly the plane is fine
    lib = _lib.load()
    K, (H, W) = 8, g.orig
    masks = torch.full((K, H, W), 7, dtype=torch.uint8, device=cuda)
    boxes = torch.full((K, 4), -7, dtype=torch.int32, device=cuda)
    stab = torch.full((K,), -7.0, dtype=torch.float32, device=cuda)
    keep = torch.full((K,), 7, dtype=torch.uint8, device=cuda)
    need = lib.hgl_sam_postprocess_workspace_bytes(K)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)

    def call(nbytes):
        return lib.hgl_sam_postprocess(low_t.data_ptr(), iou_t.data_ptr(), K, g.low, g.low, g.S, g.inp[0], g.inp[1], H, W, 0.0, 1.0,
                                       -1e30, 0.0, masks.data_ptr(), boxes.data_ptr(), stab.data_ptr(), keep.data_ptr(), None,
                                       ws.data_ptr(), nbytes, ops._stream())

    for nbytes in (need - 1, 0):
        assert call(nbytes) == HGL_EWORKSPACE
        assert b"workspace too small" in lib.hgl_last_error()
        torch.cuda.synchronize()
        assert bool((masks == 7).all()) and bool((boxes == -7).all()) and bool((stab == -7).all()) and bool((keep == 7).all())
    assert call(need) == 0                                            # the same call with the workspace it asked for
    ref = sam.postprocess(low_t, iou_t, g.inp, g.orig)
    for x, y in zip((masks, boxes, stab, keep), ref):
        assert same(x, y)
