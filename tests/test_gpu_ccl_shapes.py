"""The connected-component clean-up (csrc/sam_ccl.hip: remove_small_regions, remove_small_regions_boxes, mask_boxes) against
the oracle at every width and height at which its host code or its kernels take another route, on patterns that each aim at
one mechanism (tests/ccl_cases.py; the generator and the oracle are checked on the CPU by tests/test_ccl_cases_host.py).

Widths: below 16 (a 16-byte chunk of box_kernel spans several rows), around 64 (one step of a row scan), 128, around 768 (the
last width with 16-row LDS strips), around 1024 (a second group of RowScan steps; 12- and 11-row strips), 2049, 4096 / 4097 /
6144 (3- and 2-row strips), 6145 (no strips: the global pass over all row pairs).  Heights, with s rows per strip:
1 (no merge launch), 2, s-1, s, s+1 (a one-row last strip), 2s, 2s+1.  Thresholds 1 (nothing is small: the unchanged path of
the apply pass), 2, 20 and H*W+1 (everything is small: islands keeps the first largest).  Everything is binary, every
comparison exact, every call is made twice and must repeat itself bit for bit.
"""
import numpy as np
import pytest
import torch

import ccl_cases as C
from hybridgl_amd import ops
from hybridgl_amd import sam as hsam
from oracle import sam_oracle as S

pytestmark = pytest.mark.gpu
MODES = ("holes", "islands")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def twice(fn, *args):
    """every call is made twice: the results must be bit-identical"""
    a, b = fn(*args), fn(*args)
    if isinstance(a, torch.Tensor):
        a, b = (a,), (b,)
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"{fn.__name__} is not reproducible"
    return a if len(a) > 1 else a[0]


def oracle(b, thr, mode):
    """-> (uint8 [N,H,W] of 0/1, bool [N])"""
    res = [S.remove_small_regions(m != 0, thr, mode) for m in b]
    return np.stack([r[0] for r in res]).astype(np.uint8), np.array([bool(r[1]) for r in res])


def check_batch(cuda, names, b, thrs, modes=MODES):
    """all three entry points on one batch against the oracle -> nothing; raises with the list of (pattern, mode, threshold)
    that differ"""
    H, W = b.shape[1:]
    mt = T(b, cuda)
    bad = []
    bx_in = twice(hsam.mask_boxes, mt).cpu().numpy().astype(np.int64)
    ref_in = S.mask_to_box(b != 0)
    bad += [(n, "mask_boxes") for i, n in enumerate(names) if not np.array_equal(bx_in[i], ref_in[i])]
    for mode in modes:
        for thr in thrs:
            out, ch = twice(hsam.remove_small_regions, mt, thr, mode)
            outb, chb, bx = twice(hsam.remove_small_regions_boxes, mt, thr, mode)
            assert torch.equal(outb, out) and torch.equal(chb, ch), (H, W, mode, thr, "the two entry points differ")
            out, ch, bx = out.cpu().numpy(), ch.cpu().numpy(), bx.cpu().numpy().astype(np.int64)
            ref, rch = oracle(b, thr, mode)
            rbx = S.mask_to_box(ref)
            for i, n in enumerate(names):
                if not np.array_equal(out[i], ref[i]):
                    bad.append((n, mode, thr, "mask", int((out[i] != ref[i]).sum())))
                if ch[i] not in (0, 1) or bool(ch[i]) != rch[i]:
                    bad.append((n, mode, thr, "changed", int(ch[i])))
                if not np.array_equal(bx[i], rbx[i]):
                    bad.append((n, mode, thr, "box", bx[i].tolist(), rbx[i].tolist()))
    assert not bad, f"{H}x{W}, {len(names)} masks: {len(bad)} differ from the oracle: {bad[:12]}"


@pytest.mark.parametrize("shape", C.shapes(), ids=lambda s: f"W{s[1]}-H{s[0]}")
def test_clean_up_equals_oracle_on_the_grid(cuda, shape):
    """every pattern that exists at the shape in ONE batch (so N varies and N*H is often no multiple of 4: the four row-waves
    of a workgroup straddle two masks or run off the end), both modes, four thresholds"""
    H, W = shape
    names, b = C.batch(H, W)
    check_batch(cuda, names, b, C.thresholds(H, W))


@pytest.mark.parametrize("H,W,n", [(17, 129, 1), (17, 129, 5), (25, 1024, 1), (3, 4097, 3), (33, 6145, 1), (1, 65, 1), (2, 2, 1)])
def test_batches_of_one_and_row_counts_one_over_a_multiple_of_four(cuda, H, W, n):
    """N = 1 (each pattern on its own: its mask is the whole batch, whatever its neighbours in the grid test were) and
    N*H % 4 == 1 (the last workgroup holds ONE row)"""
    names, b = C.batch(H, W)
    assert n == 1 or n * H % 4 == 1
    if n == 1:
        pick = [i for i, nm in enumerate(names)
                if nm in ("serpentine", "speckle50", "seam_links_se_k10_0", "seam_links_sw_k1_0", "tie_a", "comb_down2", "nonbinary",
                          "corners_cols", "thresh_exact_rows_inv")]
        assert pick
        for i in pick:
            check_batch(cuda, names[i:i + 1], b[i:i + 1], C.thresholds(H, W))
    else:
        for o in (0, len(names) - n):
            check_batch(cuda, names[o:o + n], b[o:o + n], C.thresholds(H, W))


@pytest.mark.parametrize("H,W", [(17, 129), (23, 1025), (5, 4097), (3, 7)])
def test_chained_clean_up_into_slices_at_odd_offsets(cuda, H, W):
    """holes, then islands with boxes, the way Sam._cleanup chains them: inputs and outputs are slices of larger tensors that
    begin at an ODD byte offset (H*W odd, an odd number of masks before the slice).  Equal to the calls on fresh tensors and
    to the oracle's two-step sequence (sam_oracle.amg_filter); nothing outside the slices is written."""
    assert H * W % 2 == 1
    names, b = C.batch(H, W)
    n, off, tail = len(names), 3, 2
    for thr in (2, C.THRESH):
        src = torch.full((off + n + tail, H, W), 1, dtype=torch.uint8, device=cuda)
        sl = slice(off, off + n)
        src[sl] = T(b, cuda)
        assert src[sl].data_ptr() % 2 == 1
        m1, m2 = torch.full_like(src, 7), torch.full_like(src, 7)
        c1 = torch.full((off + n + tail,), 7, dtype=torch.uint8, device=cuda)
        c2 = c1.clone()
        nb = torch.full((off + n + tail, 4), -7, dtype=torch.int32, device=cuda)
        for _ in range(2):
            hsam.remove_small_regions(src[sl], thr, "holes", out=(m1[sl], c1[sl]))
            hsam.remove_small_regions_boxes(m1[sl], thr, "islands", out=(m2[sl], c2[sl], nb[sl]))
        fresh = T(b, cuda)
        f1, fc1 = twice(hsam.remove_small_regions, fresh, thr, "holes")
        f2, fc2, fnb = twice(hsam.remove_small_regions_boxes, f1, thr, "islands")
        assert torch.equal(m1[sl], f1) and torch.equal(c1[sl], fc1)
        assert torch.equal(m2[sl], f2) and torch.equal(c2[sl], fc2) and torch.equal(nb[sl], fnb)
        for t, fill in ((m1, 7), (m2, 7), (c1, 7), (c2, 7), (nb, -7)):
            assert bool((t[:off] == fill).all()) and bool((t[off + n:] == fill).all()), "written outside the slice"
        r1, rc1 = oracle(b, thr, "holes")
        r2, rc2 = oracle(r1, thr, "islands")
        assert np.array_equal(f1.cpu().numpy(), r1) and np.array_equal(fc1.cpu().numpy().astype(bool), rc1)
        assert np.array_equal(f2.cpu().numpy(), r2) and np.array_equal(fc2.cpu().numpy().astype(bool), rc2)
        assert np.array_equal(fnb.cpu().numpy().astype(np.int64), S.mask_to_box(r2))


def test_small_shapes_after_the_largest_do_not_see_its_workspace(cuda):
    """the "sam_ccl" workspace is grow-only and only run starts are initialised in its label and area planes: the largest
    shape of the grid runs first, the smallest after it, then once more over a workspace of zeros"""
    H, W = 33, 6145
    names, b = C.batch(H, W)
    keep = [i for i, n in enumerate(names) if n.startswith(("speckle", "checker", "diag", "comb"))]
    big = T(b[keep], cuda)
    small = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 15), (1, 17), (16, 17), (17, 63), (2, 65)]

    def sweep():
        for h, w in small:
            sn, sb = C.batch(h, w)
            check_batch(cuda, sn, sb, C.thresholds(h, w))

    for mode in MODES:
        hsam.remove_small_regions_boxes(big, C.THRESH, mode)
    sweep()
    ws = ops.workspace(1, cuda, "sam_ccl")
    assert ws.numel() >= big.numel() * 8            # the large call's buffer is the one the small calls get
    ws.zero_()
    sweep()


def test_mask_boxes_stride_loop_and_unaligned_bases(cuda):
    """hgl_mask_boxes: masks of more than 64 x 256 x 16 pixels (a block's threads make further trips), mask bases that are no
    multiple of 16 bytes (the byte-wise path), and both at once"""
    rng = np.random.default_rng(12)
    H, W = 640, 700
    m = np.zeros((3, H, W), dtype=np.uint8)
    m[0, H - 1, W - 1] = 1                                  # one pixel, in the last trip of the loop
    m[1] = rng.random((H, W)) < 1e-4
    m[2, 500:630, 3:690] = rng.random((130, 687)) < 0.5     # nothing in the first trip
    m[2, 0, 350] = 255
    assert H * W > 64 * 256 * 16
    got = twice(hsam.mask_boxes, T(m, cuda)).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, S.mask_to_box(m != 0))
    for h, w in ((33, 65), (641, 411)):                     # odd H*W: every second mask starts at an odd address
        assert h * w % 2 == 1
        b = (rng.random((5, h, w)) < 0.01).astype(np.uint8)
        b[1] = 0
        b[2, h - 1, w - 1] = 2
        b[3, :, 0] = 1
        big = torch.zeros((6, h, w), dtype=torch.uint8, device=cuda)
        big[1:] = T(b, cuda)
        got = twice(hsam.mask_boxes, big[1:]).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, S.mask_to_box(b != 0)), (h, w)
