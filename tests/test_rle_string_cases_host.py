"""The numpy statement of the device string codec's contract (tests/rle_string_cases.py) against the host codec it must equal:
hgl_rle_to_string / hgl_rle_from_string (csrc/gtmask.cpp) through ctypes -- host functions, no device needed.  What holds here
is what the GPU test holds the kernels against."""
import ctypes as C

import numpy as np
import pytest

from hybridgl_amd import _lib

import rle_string_cases as RC


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def host_encode(lib, counts):
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    buf = C.create_string_buffer(7 * len(c) + 1)
    n = C.c_size_t(0)
    assert lib.hgl_rle_to_string(c.ctypes.data, len(c), buf, len(buf), C.byref(n)) == 0
    return buf.raw[:n.value]


def host_parse(lib, s):
    """(code, counts) with the contract's codes: 0, 2 truncated, 3 long"""
    assert 0 not in s
    m = C.c_longlong(-1)
    rc = lib.hgl_rle_from_string(C.c_char_p(s), None, 0, C.byref(m))
    if rc != 0:
        msg = lib.hgl_last_error()
        assert (b"truncated" in msg) != (b"more than 7" in msg), msg
        return (2 if b"truncated" in msg else 3), None
    buf = np.zeros(max(m.value, 1), np.uint32)
    assert lib.hgl_rle_from_string(C.c_char_p(s), buf.ctypes.data, len(buf), C.byref(m)) == 0
    return 0, [int(v) for v in buf[:m.value]]


def test_the_writer_of_the_contract_equals_the_host_codec(lib):
    seen = set()
    for name, (slots, table) in RC.write_sets().items():
        S, sw = slots.shape
        total = 0
        for s in range(S):
            if RC.entry_code(table[s], sw) == 0:
                c = slots[s, :table[s, 0]]
                want = host_encode(lib, c)
                assert RC.encode(c) == want, (name, s)
                total += len(want)
                seen |= {RC.length(RC.delta(c, i)) for i in range(len(c))}
        for cap in (total, total - 1, 0, total + 5):
            if cap < 0:
                continue
            out, offsets, status = RC.to_strings(slots, table, cap)
            assert offsets[S] == total and offsets[0] == 0 and (np.diff(offsets) >= 0).all()      # true also under a small cap
            covered = np.zeros(cap, bool)
            for s in range(S):
                code = RC.entry_code(table[s], sw)
                if code == 0 and offsets[s + 1] <= cap:
                    assert status[s] == 0 and bytes(out[offsets[s]:offsets[s + 1]]) == host_encode(lib, slots[s, :table[s, 0]])
                    covered[offsets[s]:offsets[s + 1]] = True
                else:
                    assert status[s] == (3 if code == 0 else code) and (code == 0 or offsets[s + 1] == offsets[s])
            assert (out[~covered] == RC.FENCE8).all()
            if cap == total - 1:
                assert status[np.flatnonzero(np.diff(offsets) > 0)[-1]] == 3
    assert seen == {1, 2, 3, 4, 5, 6, 7}


def test_the_boundaries_of_every_length():
    for k in range(1, 7):
        e = 1 << (5 * k - 1)
        assert [RC.length(x) for x in (e - 1, e, -e, -e - 1)] == [k, k + 1, k, k + 1]
    assert RC.length(RC.M32) == RC.length(-RC.M32) == 7 and RC.length(0) == 1
    xs = [RC.delta(c, 3) for c in map(RC.counts_with_delta, RC.boundary_deltas())]
    assert xs == RC.boundary_deltas()
    assert [len(RC.encode(RC.counts_of_string_length(L))) for L in range(1, 10)] == list(range(1, 10))


def test_the_reader_of_the_contract_equals_the_host_parser(lib):
    for s in RC.good_strings():
        code, counts = RC.parse(s)
        assert (code, counts) == host_parse(lib, s)
        assert code == 0
    for s, want in RC.bad_strings():
        assert RC.parse(s)[0] == want == host_parse(lib, s)[0], s
    accepted = 0
    rnd = RC.random_strings()
    assert len(rnd) == 2000
    for s in rnd:
        got = RC.parse(s)
        assert got == host_parse(lib, s), s
        accepted += got[0] == 0
    assert 200 < accepted < 1800      # both sides of the fence are well populated
    for e in range(255, 264):
        s = RC.straddle(e)
        c = RC.parse(s)[1]
        assert s[e] < 80 and all(b >= 80 for b in s[e - 6:e]) and c[e - 6] == (c[e - 8] - RC.M32) & RC.M32 and len(c) == e - 4
    assert RC.parse(b"") == (0, [])


def test_round_trips_and_the_index_two_rule():
    for slots, table in RC.write_sets().values():
        for s in range(len(table)):
            if RC.entry_code(table[s], slots.shape[1]) == 0:
                c = [int(v) for v in slots[s, :table[s, 0]]]
                assert RC.parse(RC.encode(c)) == (0, c)
    assert RC.parse(RC.encode([9, 5, 7, 2, 1])) == (0, [9, 5, 7, 2, 1])
    assert RC.encode([9, 5, 7]) == RC.group(9) + RC.group(5) + RC.group(7)      # index 2 is stored whole, not against index 0


def test_the_reader_sets():
    sets = RC.read_sets()
    for name, (data, offsets, S, sw) in sets.items():
        slots, table, status = RC.from_strings(data, offsets, S, sw)
        assert slots.shape == (S, sw)
        for s in range(S):
            code, n = int(status[s, 0]), int(status[s, 1])
            assert (slots[s, n if code == 0 else 0:] == RC.FENCE32).all()
            assert table[s].tolist() == ([n, 0, 0, 0] if code == 0 else [n, 2, 0, 0]) and (n == 0 or code in (0, 1))
    assert RC.from_strings(*sets["tight"])[2][:, :2].tolist() == [[1, 4], [0, 3], [1, 40], [0, 0], [1, 5]]
    assert RC.from_strings(*sets["broken"])[2][:, 0].tolist() == [0, 4, 0, 4]
    assert RC.from_strings(*sets["negative"])[2][:, 0].tolist() == [4, 0, 0, 0]
    codes = set(RC.from_strings(*sets["mixed"])[2][:, 0].tolist())
    assert codes == {0, 2, 3}
    assert sets["good"][2] > 700 and (RC.from_strings(*sets["good"])[2][:, 0] == 0).all()
