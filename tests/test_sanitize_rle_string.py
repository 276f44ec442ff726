"""hgl_rle_from_string (csrc/gtmask.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, on the host: a harness of its own
(tests/native/rle_string_sanitize.cpp) built as tests/test_sanitize.py builds its one, fed the well-formed and the fuzzed
strings of that test's recipe with counts buffers of 0, m - 1, m and m + 3 words and the null-pointer size query.  The run must
be clean of sanitizer reports and give the counts the regular library gives."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybridgl_amd", "csrc")


def _fnv(b):
    h = 1469598103934665603
    for v in bytes(b):
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle") / "rle_string_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-Wno-attributes", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "native", "rle_string_sanitize.cpp"), os.path.join(CSRC, "gtmask.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def _rle_string(counts):
    """maskApi.c rleToString (:203-215): the encoder, used here to make well-formed inputs"""
    s = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = not ((x == -1 and (ch & 0x10)) or (x == 0 and not (ch & 0x10)))
            if more:
                ch |= 0x20
            s.append(chr(ch + 48))
    return "".join(s)


def _library(lib, s, cap):
    """(rc, m, hash of the counts written) from the regular library; cap -1 = null-pointer size query"""
    m = C.c_longlong(-1)
    b = s.encode("ascii")
    if cap < 0:
        rc = lib.hgl_rle_from_string(C.c_char_p(b), None, 0, C.byref(m))
        return (rc, m.value if rc == 0 else -1, _fnv(b""))
    buf = np.zeros(max(cap, 1), np.uint32)
    rc = lib.hgl_rle_from_string(C.c_char_p(b), buf.ctypes.data, cap, C.byref(m))
    if rc != 0:
        return (rc, -1, _fnv(b""))
    return (rc, m.value, _fnv(buf[:min(m.value, cap)].tobytes()))


def test_rle_from_string_is_clean_under_asan_ubsan(harness, tmp_path):
    from hybridgl_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2024)
    strings, well_formed = [], {}
    for i in range(300):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        if i % 3 == 0:                                       # well-formed
            cuts = np.sort(rng.integers(0, H * W + 1, size=int(rng.integers(0, 9))))
            counts = np.diff(np.concatenate([[0], cuts, [H * W]])).tolist()
            s = _rle_string(counts)
            well_formed[len(strings)] = counts
        else:                                                # fuzzed: random printable bytes, truncated groups, long chains
            s = "".join(chr(int(v)) for v in rng.integers(33, 127, size=int(rng.integers(0, 40))))
            if i % 3 == 2:
                s += "o" * int(rng.integers(0, 12))          # continuation bits with no end
        strings.append(s)
    strings += ["", "o", "oooooooo", "ooooooo0", "0" * 4000]
    lines, expect, n_ok = [], [], 0
    for k, s in enumerate(strings):
        rc, m, _ = _library(lib, s, -1)
        if k in well_formed:
            assert rc == 0 and m == len(well_formed[k])
            buf = np.zeros(m, np.uint32)
            mm = C.c_longlong(0)
            assert lib.hgl_rle_from_string(C.c_char_p(s.encode("ascii")), buf.ctypes.data, m, C.byref(mm)) == 0
            assert buf.tolist() == well_formed[k]
        n_ok += rc == 0
        m = max(m, 0)
        for cap in sorted({-1, 0, max(m - 1, 0), m, m + 3}):
            lines.append(f"{cap} {s if s else '<empty>'}")
            expect.append(_library(lib, s, cap))
    assert n_ok >= 100 and n_ok < len(strings)      # both the accepting and the rejecting path ran
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stderr[-4000:], r.stdout[-500:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = [l.split() for l in r.stdout.strip().splitlines()]
    assert len(got) == len(expect)
    for g, line, (rc, m, h) in zip(got, lines, expect):
        if rc != 0:
            assert int(g[0]) != 0, (line, g)
        else:
            assert (int(g[0]), int(g[1]), int(g[2])) == (0, m, h), (line, g, m, h)
