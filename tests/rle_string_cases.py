"""The contract of hgl_rle_to_strings_device / hgl_rle_from_strings_device (include/hybridgl.h, csrc/rle_string.hip) in numpy,
and the case tables that the host test (against hgl_rle_to_string / hgl_rle_from_string, no device needed) and the GPU test
share.  The arithmetic is stated here a second time, from the rules of csrc/rle_string.h and not from its code: one count at a
time, one group at a time."""
import numpy as np

FENCE8, FENCE32 = 0xA5, 0x7E7E7E7E
M32 = (1 << 32) - 1


# ---- the arithmetic

def delta(counts, i):
    return int(counts[i]) - (int(counts[i - 2]) if i > 2 else 0)


def length(x):
    k = 1
    while not (-(1 << (5 * k - 1)) <= x < (1 << (5 * k - 1))):
        k += 1
    return k


def group(x):
    k = length(x)
    return bytes(48 + ((x >> (5 * j)) & 31) + (32 if j < k - 1 else 0) for j in range(k))      # Python's >> is arithmetic


def encode(counts):
    return b"".join(group(delta(counts, i)) for i in range(len(counts)))


def parse(s):
    """(code, counts) of a byte string as the device reads it: 0 and the counts, 2 truncated, 3 long (no counts)"""
    xs, g = [], []
    for p, b in enumerate(s):
        c = (b - 48) & 0xFF
        if len(g) == 7:
            return 3, None      # an eighth character of the group exists
        g.append(c)
        if not c & 32:
            v = sum((cj & 31) << (5 * j) for j, cj in enumerate(g))
            if c & 16:
                v |= -1 << (5 * len(g))
            xs.append(v & M32)
            g = []
    if g:
        return 2, None
    counts = []
    for i, x in enumerate(xs):
        counts.append((x + (counts[i - 2] if i > 2 else 0)) & M32)
    return 0, counts


# ---- the two entries

def entry_code(row, sw):
    n, form = int(row[0]), int(row[1])
    if form == 1:
        return 1
    return 0 if form == 0 and 0 <= n <= sw else 2


def to_strings(slots, table, cap):
    """(bytes uint8 [cap] over FENCE8, offsets int64 [S+1], status int32 [S])"""
    S, sw = slots.shape
    out = np.full(cap, FENCE8, np.uint8)
    offsets, status = np.zeros(S + 1, np.int64), np.zeros(S, np.int32)
    strings = []
    for s in range(S):
        status[s] = entry_code(table[s], sw)
        strings.append(encode(slots[s, :table[s, 0]].astype(np.uint32)) if status[s] == 0 else b"")
        offsets[s + 1] = offsets[s] + len(strings[s])
    for s in range(S):
        if status[s] == 0:
            if offsets[s + 1] > cap:
                status[s] = 3
            else:
                out[offsets[s]:offsets[s + 1]] = np.frombuffer(strings[s], np.uint8)
    return out, offsets, status


def from_strings(data, offsets, S, sw):
    """(slots uint32 [S, sw] over FENCE32, table int32 [S,4], status int32 [S,4])"""
    slots = np.full((S, sw), FENCE32, np.uint32)
    table, status = np.zeros((S, 4), np.int32), np.zeros((S, 4), np.int32)
    for s in range(S):
        b0, b1 = int(offsets[s]), int(offsets[s + 1])
        if b0 < 0 or b0 > b1 or b1 > len(data):
            code, counts = 4, None
        else:
            code, counts = parse(bytes(data[b0:b1]))
        if code == 0 and len(counts) > sw:
            table[s], status[s] = (len(counts), 2, 0, 0), (1, len(counts), 0, 0)
        elif code == 0:
            slots[s, :len(counts)] = counts
            table[s], status[s] = (len(counts), 0, 0, 0), (0, len(counts), 0, 0)
        else:
            table[s], status[s] = (0, 2, 0, 0), (code, 0, 0, 0)
    return slots, table, status


# ---- the cases

def boundary_deltas():
    xs = [0, M32, -M32]
    for k in range(1, 7):
        e = 1 << (5 * k - 1)
        xs += [e - 1, e, e + 1, -e - 1, -e, -e + 1]
    return xs


def counts_with_delta(x):
    """four counts whose last stands in the string as the difference x"""
    return [0, -x, 0, 0] if x < 0 else [0, 0, 0, x]


def counts_of_string_length(L):
    """counts of one or two groups whose string has 1 <= L <= 9 bytes"""
    one = lambda k: 1 if k == 1 else 1 << (5 * (k - 1) - 1)
    return [one(L)] if L <= 7 else [one(7), one(L - 7)]


def long_counts(n, seed):
    rng = np.random.default_rng(seed)
    mag = rng.integers(0, 33, n)
    c = (rng.integers(0, 1 << 32, n, dtype=np.uint64) >> (32 - mag).astype(np.uint64)).astype(np.uint64)
    c[rng.random(n) < 0.2] = 0      # counts of 0
    return [int(v) for v in c]


def make_set(entries, sw=None):
    """entries: a list of counts, or ("form", form, n_counts) for an entry without counts -> (slots uint32, table int32)"""
    lists = [e for e in entries if not isinstance(e, tuple)]
    sw = max([len(e) for e in lists] + [1]) if sw is None else sw
    S = len(entries)
    rng = np.random.default_rng(S + sw)
    slots = rng.integers(0, 1 << 32, (S, sw), dtype=np.uint64).astype(np.uint32)      # words beyond n_counts: anything
    table = np.zeros((S, 4), np.int32)
    for s, e in enumerate(entries):
        if isinstance(e, tuple):
            table[s] = (e[2], e[1], 7, 0)
        else:
            slots[s, :len(e)] = np.asarray(e, np.uint64).astype(np.uint32)
            table[s] = (len(e), 0, 7, 0)
    return slots, table


def write_sets():
    """name -> (slots, table): every case of the writer, many per set"""
    deltas = [counts_with_delta(x) for x in boundary_deltas()]
    short = [[], [5], [5, 0], [0, 5, 7], [9, 5, 7, 2], [3, 9, 1, 4, 0xFFFFFFFF, 0, 0xFFFFFFFF]]      # index 2 adds nothing to index 0's
    chunks = [long_counts(n, n) for n in (255, 256, 257, 513)]      # slot_words == 513 == the longest entry's n_counts
    mixed = deltas[:6] + [("form", 1, 40), [1, 2, 3], ("form", 2, 3), [4], ("form", 3, 0), [], ("form", 0, -1), [6, 6],
                          ("form", 0, 99), ("form", 9, 1), [7]]
    align = [counts_of_string_length(L) for rep in range(9) for L in ([1, 2, 3, 4, 5, 6, 7, 8, 9] * 2)[rep:rep + 9]]
    return {
        "empty": make_set([], 3),
        "one": make_set([[12, 3, 400]]),
        "deltas": make_set(deltas + short),
        "chunks": make_set(chunks + short),
        "mixed": make_set(mixed, 8),
        "align": make_set(align),
        "many": make_set([[i * 37 % 5000] for i in range(600)]),      # the scan over the entries crosses 256 twice
    }


def straddle(e):
    """a string whose 7-character group ends at byte e: one-character groups before it, one behind it"""
    return b"1" * (e - 6) + group(-M32) + b"2"


def bad_strings():
    """(string, code): 3 long, 2 truncated"""
    o = b"o"      # 111: continues, payload 31
    return [(b"12" + o * 7 + b"1" + b"34", 3), (b"12" + o * 8 + b"1" + b"34", 3), (b"12" + o * 7 + b"1", 3), (b"12" + o * 8 + b"1", 3),
            (o * 8, 3), (o * 9, 3), (b"1" * 300 + o * 8, 3), (o, 2), (b"123" + o, 2), (o * 7, 2), (b"1" + o * 7, 2),
            (b"1" * 250 + o * 7, 2), (o * 8 + b"1" + o, 3)]


def high_bytes():
    """accepted strings with bytes outside 48 .. 111: only (b - 48) & 63 counts (0xD0: continues, payload 0; 0x0F: ends, sign)"""
    return [bytes([112, 127, 128, 200, 255, 48 + 15]), bytes([0xD0] * 6 + [0x0F]), bytes([0xD0, 0x9F, 0x8F]),
            bytes([240, 47, 1, 0x7F, 31, 0x0F])]


def random_strings(n=2000, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(0, 41))
        b = rng.integers(1, 256, L)
        if i % 3 == 0:      # mostly ending bytes, so that many strings are accepted
            b = np.where(rng.random(L) < 0.8, 48 + rng.integers(0, 32, L), b)
        out.append(bytes(b.astype(np.uint8)))
    return out


def good_strings():
    out = []
    for slots, table in write_sets().values():
        out += [encode(slots[s, :table[s, 0]]) for s in range(len(table)) if entry_code(table[s], slots.shape[1]) == 0]
    return out + [straddle(e) for e in range(255, 264)] + high_bytes() + [b""]


def pack(strings):
    """(data uint8, offsets int64 [S+1]) of strings back to back"""
    offsets = np.zeros(len(strings) + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in strings])
    return np.frombuffer(b"".join(strings), np.uint8).copy(), offsets


def read_sets():
    """name -> (data, offsets, S, slot_words): every case of the reader, many per set"""
    good = good_strings()
    most = max(len(parse(s)[1]) for s in good)
    bad = [s for s, _ in bad_strings()]
    mixed = [b"1", bad[0], b"23", bad[7], b"", bad[4], straddle(258), bad[9], b"456"]
    rnd = random_strings()
    tight = [encode(c) for c in ([1, 2, 3, 4], [1, 2, 3], [9] * 40, [], [5, 6, 7, 8, 9])]      # slot_words 3: n_counts - 1, n_counts, beyond
    d, o = pack([b"12", b"345", b"6", b"78"])
    broken = o.copy()
    broken[:] = (0, 5, 2, 3, 9)      # entry 0 overlaps but is inside; 1: begin > end; 2: good; 3: beyond the total
    neg = o.copy()
    neg[0] = -1
    return {
        "empty": pack([]) + (0, 3),
        "one": pack([encode([12, 3, 400])]) + (1, 3),
        "good": pack(good) + (len(good), most),
        "mixed": pack(mixed) + (len(mixed), 300),
        "random": pack(rnd) + (len(rnd), 41),
        "tight": pack(tight) + (len(tight), 3),
        "broken": (d, broken, 4, 5),
        "negative": (d, neg, 4, 5),
    }
