"""The polygon walk of the device rasteriser (csrc/poly_walk.h: vertex -> 5x grid, the steps of an edge, the predecessor of a
walk point, the crossing of a pair) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
(tests/native/poly_walk_sanitize.cpp) built with g++ -fsanitize=address,undefined -fno-sanitize-recover: every step of every
case on its own and in reverse order, toggles XORed into a plane, prefix parity, both combination rules -- bit-equal to the
host codec (hgl_gt_mask_from_polygons) on the 448 cases of tests/poly_cases.py and on the corners of the walk's arithmetic."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import poly_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# vertices at the edge of the codec's guard: 10^6 steps per edge, crossings far outside the image on every side
FAR = (50, 60, [[-99999.0, -99999.0, 99999.0, -99999.0, 99999.0, 99999.0, -99999.0, 99999.0], [-99999.0, 20.5, 99999.0, 21.5, 30.0, 99999.0]])
ONE_POINT = (8, 9, [[3.0, 4.0]])
# the degenerate edge (two vertices on one grid point) after a y-major edge that ends at a negative x, where the end of the walk
# along that edge is not the vertex ((int)(x + 0.5) truncates towards zero), and before one; then the same the other way round
DEGENERATE = (40, 30, [[-1.4, 30.0, -3.0, 2.0, -3.0, 2.0, 10.0, 12.0], [10.0, 12.0, -3.0, 2.0, -3.0, 2.0, -1.4, 30.0],
                       [-3.0, 2.0, -3.0, 2.0, -2.2, 35.0], [5.0, 5.0, 5.0, 5.0, 5.04, 5.04, 20.0, 30.0, 2.0, 25.0]])
EXTRA = [FAR, ONE_POINT, DEGENERATE]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_poly_walk") / "poly_walk_sanitize"
    # -ffp-contract=off: the walk's sums must round twice (poly_walk.h); g++ does not read the header's clang pragma
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "poly_walk_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_every_step_alone_equals_the_host_codec(harness, tmp_path):
    todo = PC.cases() + EXTRA
    assert len(PC.cases()) == 448
    src, dst = tmp_path / "cases.txt", tmp_path / "planes.bin"
    with open(src, "w") as f:
        for H, W, polys in todo:
            f.write(f"{H} {W} {len(polys)}\n")
            for p in polys:
                f.write(f"{len(p) // 2} " + " ".join(float(v).hex() for v in p) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(src), str(dst)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == str(len(todo))
    raw = np.fromfile(dst, dtype=np.uint8)
    want = PC.expected_all() + [PC.expected(H, W, polys) for H, W, polys in EXTRA]
    o = 0
    for k, ((H, W, _), (count, area)) in enumerate(zip(todo, want)):
        nbytes = (H * W + 7) // 8
        for rule in (0, 1):
            got = np.unpackbits(raw[o:o + nbytes], bitorder="little")[:H * W].reshape(W, H).T
            assert np.array_equal(got, PC.by_rule(count, rule)), (k, rule)
            o += nbytes
        assert int(raw[o:o + 8].view(np.int64)[0]) == area, k
        o += 8
    assert o == len(raw)
    # the corner cases do what they are here for
    assert want[-3][1] > 0 and want[-2][0].sum() == 0 and want[-1][0].max() >= 1
