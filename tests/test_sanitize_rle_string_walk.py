"""The arithmetic of the device's COCO string codec (csrc/rle_string.h: the difference of a count, the length and the characters
of its group, the value of a group read back from its last byte, the long-group test, the un-delta as two running sums) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/rle_string_walk_sanitize.cpp) built with
g++ -fsanitize=address,undefined -fno-sanitize-recover=all and fed a case file: every function by itself, against the numpy
statement of the contract (tests/rle_string_cases.py).  Nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rle_string_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_rle_string_walk") / "rle_string_walk_sanitize"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rle_string_walk_sanitize.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def hexof(b):
    return bytes(b).hex() if len(b) else "-"


def test_every_function_alone_equals_the_contract(harness, tmp_path):
    rng = np.random.default_rng(5)
    lines, want = [], []
    xs = RC.boundary_deltas() + [1 << 29, -(1 << 29) - 1, (1 << 32) - 2] + [int(v) for v in rng.integers(-RC.M32, RC.M32 + 1, 300)]
    for x in xs:      # length and characters
        lines.append(f"X {x}")
        want.append(f"{RC.length(x)} {RC.group(x).hex()}")
        g = RC.group(x)      # the value of a group
        lines.append(f"G {g.hex()}")
        want.append(str(x & RC.M32))
    for L in range(1, 8):      # groups that no writer makes: high bytes, payload beyond the sign
        for _ in range(20):
            c = [int(v) | 32 for v in rng.integers(0, 256, L - 1)] + [int(rng.integers(0, 256)) & ~32]
            g = bytes((v + 48) & 0xFF for v in c)
            code, counts = RC.parse(g)
            assert code == 0 and len(counts) == 1
            lines.append(f"G {g.hex()}")
            want.append(str(counts[0]))
    sets = RC.write_sets()
    for name in ("deltas", "chunks", "mixed", "align"):      # whole strings
        slots, table = sets[name]
        for s in range(len(table)):
            if RC.entry_code(table[s], slots.shape[1]) == 0:
                c = slots[s, :table[s, 0]]
                lines.append(f"W {len(c)} " + " ".join(str(int(v)) for v in c))
                want.append(hexof(RC.encode(c)))
    todo = RC.good_strings()[-20:] + [s for s, _ in RC.bad_strings()] + RC.random_strings(400)
    todo += [RC.encode(RC.long_counts(n, n)) for n in (255, 256, 257, 513)]
    for k, s in enumerate(todo):      # reading, the un-delta in stretches of odd and even length
        code, counts = RC.parse(s)
        for stretch in (1, 2, 5, 256):
            lines.append(f"R {stretch} {hexof(s)}")
            want.append(f"{code} 0" if code else " ".join(str(v) for v in [0, len(counts)] + counts))
    for i0 in (0, 1, 2, 3, 256, 257):      # a stretch by itself, at either start parity, with carries that wrap
        for n in (0, 1, 2, 7):
            v = [int(x) for x in rng.integers(0, 1 << 32, n)]
            carry = [int(x) for x in rng.integers(0, 1 << 32, 2)]
            lines.append(f"U {i0} {n} {carry[0]} {carry[1]} " + " ".join(map(str, v)))
            out, c = [], list(carry)
            for j, x in enumerate(v):
                i = i0 + j
                if i == 0:
                    out.append(x)      # counts[0] = x_0, and no later count adds it
                else:
                    c[i & 1] = (c[i & 1] + x) & RC.M32
                    out.append(c[i & 1])
            want.append(" ".join(map(str, out + c)))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, str(src)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [g.strip() for g in r.stdout.strip().split("\n")]
    assert len(got) == len(want)
    for k, (g, w, line) in enumerate(zip(got, want, lines)):
        assert g == w, (k, line[:200], g[:200], w[:200])
