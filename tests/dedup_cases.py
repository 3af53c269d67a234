"""Cases of the duplicate suppression (aisx_dedup_*, include/aisx.h): a dict-based model written from the header's text,
with the key function restated here, and the scripts -- lists of calls over one handle -- that the host form, the lane
model of the kernel bodies and the device form are all run through.  TEST INFRASTRUCTURE."""
import numpy as np

REC_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu
COUNTS = ("in", "kept", "dup_call", "dup_window", "bad_len")
M64 = (1 << 64) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def key(payload):
    """include/aisx.h, aisx_dedup_key, restated"""
    p = bytes(payload)
    h = 0x9E3779B97F4A7C15 ^ ((len(p) * 0xFF51AFD7ED558CCD) & M64)
    for k in range(0, len(p), 8):
        w = int.from_bytes(p[k:k + 8], "little")  # (missing octets count as 0)
        h = ((h ^ w) * 0x9FB21C651E98DF25) & M64
        h ^= h >> 32
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & M64
    h ^= h >> 32
    return h or 1


def hash_bits(max_pdus):
    """slots of the device form's hashes: a power of two, at least 64 and at least 2 * max_pdus"""
    b = 6
    while (1 << b) < 2 * max_pdus:
        b += 1
    return b


def home(k, bits):
    """a key's home slot (k_dedup.h, dd_home): its top bits; the chain goes on at the next slot, round the end"""
    return k >> (64 - bits)


class Model:
    """the host form's contract, record by record, on a dict"""

    def __init__(self, window, length_max=64):
        self.window, self.length_max = window, length_max
        self.reset()

    def reset(self):
        self.kept, self.prev = {}, None  # key -> stamp of the call that kept it

    def update(self, recs, data, n, stamp, marks=None):
        """None when the stamp is refused, else (kept records, first, copies, kept marks or None, counts)"""
        if self.prev is not None and stamp <= self.prev:
            return None
        self.prev = stamp
        out, first, copies, om, here = [], [], [], [], {}
        cnt = dict.fromkeys(COUNTS, 0)
        cnt["in"] = n
        for i in range(n):
            ln, off = int(recs["len"][i]), int(recs["offset"][i])
            if not 0 <= ln <= self.length_max - 1:
                cnt["bad_len"] += 1
                first.append(len(out))
                out.append(i)
                copies.append(1)
                continue
            k = key(data[off:off + ln].tobytes())
            t = self.kept.get(k)
            if t is not None and stamp - self.window <= t <= stamp - 1:
                cnt["dup_window"] += 1
                first.append(-1 - (stamp - t))
            elif k in here:
                cnt["dup_call"] += 1
                first.append(here[k])
                copies[here[k]] += 1
            else:
                here[k] = len(out)
                first.append(len(out))
                out.append(i)
                copies.append(1)
                self.kept[k] = stamp
        cnt["kept"] = len(out)
        return (recs[out].copy(), np.array(first, dtype=np.int32), np.array(copies, dtype=np.int32),
                np.asarray(marks)[out].astype(np.int32) if marks is not None else None, [cnt[c] for c in COUNTS])


def assert_same_result(a, b, what=""):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert list(a[4]) == list(b[4]), (what, a[4], b[4])
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(a[1], b[1]), (what, a[1], b[1])
    assert np.array_equal(a[2], b[2]), (what, a[2], b[2])
    assert (a[3] is None) == (b[3] is None) and (a[3] is None or np.array_equal(a[3], b[3])), what


# ---- record lists --------------------------------------------------------------------------------------------------
def make_list(payloads, rng, max_pdus, lens=None, order="packed", marks=True):
    """records for `payloads` (bytes each), padded to max_pdus entries of rubbish: (recs, data, marks).  order: "packed"
    (one behind the other), "shuffled" (the payloads lie in another order than the records) or "shared" (equal payloads
    share ONE copy of the bytes, so several records have the same offset).  lens: a record's len where it shall differ
    from its payload's (a bad len: the bytes are then not read)."""
    n = len(payloads)
    recs = np.zeros(max(max_pdus, n), dtype=REC_DTYPE)
    recs["offset"], recs["len"], recs["chan"] = 1 << 40, 1 << 20, -7  # (what lies beyond the count is never read)
    place = list(rng.permutation(n)) if order == "shuffled" else list(range(n))
    blob, at, seen = bytearray(b"\xee" * 3), {}, {}
    for i in place:
        p = bytes(payloads[i])
        if order == "shared" and p in seen:
            at[i] = seen[p]
            continue
        at[i] = seen[p] = len(blob)
        blob += p
    blob += b"\xee" * 3
    for i in range(n):
        recs[i] = (int(rng.integers(0, 1 << 40)), at[i], int(rng.integers(0, 4)), len(payloads[i]))
    if lens:
        for i, ln in lens.items():
            recs["len"][i] = ln
    m = rng.integers(-1, 1 << 20, size=len(recs)).astype(np.int32) if marks else None
    return recs, np.frombuffer(bytes(blob), dtype=np.uint8).copy(), m


def pool(rng, k, lo=1, hi=63):
    """k distinct payloads of lo..hi octets (AIS: 21 typical)"""
    out = set()
    while len(out) < k:
        out.add(rng.integers(0, 256, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8).tobytes())
    return sorted(out)


def find_payloads(rng, bits, slot, k, length=21):
    """k distinct payloads whose keys have the home slot `slot` in a hash of 1 << bits slots, found by search"""
    out = []
    while len(out) < k:
        p = rng.integers(0, 256, size=length, dtype=np.uint8).tobytes()
        if home(key(p), bits) == slot and p not in out:
            out.append(p)
    return out


def call(payloads, rng, max_pdus, stamp, n=None, **kw):
    recs, data, marks = make_list(payloads, rng, max_pdus, **kw)
    return ("call", recs, data, len(payloads) if n is None else n, stamp, marks)


def scripts(seed, window, max_pdus, length_max=64):
    """{name: [op]}; an op is ("call", recs, data, n, stamp, marks) or ("reset",).  Every script starts on a fresh handle."""
    rng = np.random.default_rng(seed)
    big = max_pdus
    W = window
    P = pool(rng, 40)
    s = {}

    def pick(n, k=12):  # n payloads out of k of the pool: plenty of repeats
        return [P[int(j)] for j in rng.integers(0, min(k, len(P)), size=n)]

    for n in sorted({0, 1, min(64, big), min(65, big), big}):
        s["n%d" % n] = [call(pick(n), rng, big, 5), call(pick(n), rng, big, 6)]
    s["bad_count"] = [call(pick(min(3, big)), rng, big, 1), call(pick(big), rng, big, 2, n=-1), call(pick(big), rng, big, 3, n=big + 1),
                      call(pick(big), rng, big, 4)]
    s["distinct"] = [call(pool(rng, big, 21, 21), rng, big, 1)]
    s["all_same"] = [call([P[0]] * big, rng, big, 1)]
    runs = []  # runs of equal payloads across a wave boundary (lanes 60..70) and the workgroup boundary (250..256)
    for i in range(big):
        runs.append(P[1] if 60 <= i <= 70 else P[2] if i >= 250 else P[3] if 128 <= i < 192 else P[4 + i % 5])
    s["runs"] = [call(runs, rng, big, 1), call(runs[::-1], rng, big, 2)]
    z = bytes(8)
    lens = [z[:1], z[:2], z[:8], z[:1], b"", z[:2], b"", bytes(63), bytes(63), z[:8]][:max(1, min(10, big))]
    s["lengths"] = [call(lens, rng, big, 1), call(lens[::-1], rng, big, 2 + W)]
    if big >= 6:
        s["bad_len"] = [call([P[0], P[1], P[0], P[1], P[2], P[0]], rng, big, 1, lens={1: length_max, 3: -1, 4: 1 << 30}),
                        call([P[1], P[1]], rng, big, 2, lens={1: length_max + 5})]
        s["offsets"] = [call(pick(min(50, big), 6), rng, big, 1, order="shared"), call(pick(min(50, big), 6), rng, big, 2, order="shuffled")]
    a, b = P[5], P[6]
    s["window"] = ([call([a], rng, big, 10)] + [call([a, b][:big], rng, big, 10 + d) for d in range(1, W + 1)] +
                   [call([a], rng, big, 10 + W + 1), call([b], rng, big, 10 + W + 2)])
    # suppressed at s + 1: no refresh, so kept again at s + W + 1
    s["no_refresh"] = [call([a], rng, big, t) for t in sorted({0, 1, W + 1, 2 * W + 2})]
    s["gaps"] = [call([a], rng, big, -50), call([a], rng, big, -50 + W + 7), call([a], rng, big, 1000), call([a], rng, big, 1001)]
    lo = [INT32_MIN + d for d in range(W + 2)]
    hi = [INT32_MAX - (W + 1) + d for d in range(W + 2)]
    s["extreme_stamps"] = [call([a], rng, big, t) for t in lo] + [call([a], rng, big, t) for t in hi]
    s["refused_stamp"] = [call([a], rng, big, 7), call([b], rng, big, 7), call([b], rng, big, 6), call([b], rng, big, INT32_MIN),
                          call([a, b][:big], rng, big, 8)]
    s["reset"] = [call([a], rng, big, 7), ("reset",), call([a], rng, big, 3), call([a], rng, big, 4)]
    for k in range(3):  # seeded scripts of at most 8 calls
        ops, t = [], int(rng.integers(-5, 5))
        for _ in range(int(rng.integers(3, 9))):
            if rng.random() < 0.1:
                ops.append(("reset",))
                continue
            t = t + int(rng.integers(1, 3)) if rng.random() < 0.85 else t - int(rng.integers(0, 2))  # (some are refused)
            ops.append(call(pick(int(rng.integers(0, big + 1)), 30), rng, big, t,
                            order=("packed", "shuffled", "shared")[int(rng.integers(0, 3))]))
        s["random%d" % k] = ops
    return s


def chain_scripts(seed, window, max_pdus):
    """scripts whose payloads were searched for: a probe chain that wraps from the last slot to slot 0, and many keys with
    one home slot.  Returns ({name: [op]}, {name: payloads}); the tests assert the property of the payloads."""
    rng = np.random.default_rng(seed)
    bits = hash_bits(max_pdus)
    assert max_pdus >= 16
    wrap = find_payloads(rng, bits, (1 << bits) - 1, 3)
    crowd = find_payloads(rng, bits, 17, 8)
    s = {"wrap": [call(wrap, rng, max_pdus, 1), call(wrap[::-1] + wrap[:1], rng, max_pdus, 2), call(wrap, rng, max_pdus, 2 + window + 1)],
         "crowd": [call(crowd + crowd[::-1], rng, max_pdus, 1), call(crowd[::-1], rng, max_pdus, 2),
                   call(crowd[::2], rng, max_pdus, 3 + window)]}
    return s, {"wrap": wrap, "crowd": crowd}


def run_script(ops, forms, after=None):
    """runs the ops through every form (objects with call(recs, data, n, stamp, marks) -> result or None, and reset()) and
    compares the results call by call; returns the first form's results"""
    results = []
    for k, op in enumerate(ops):
        if op[0] == "reset":
            for f in forms:
                f.reset()
            continue
        rs = [f.call(*op[1:]) for f in forms]
        for r in rs[1:]:
            assert_same_result(rs[0], r, "op %d" % k)
        results.append(rs[0])
        if after:
            after(k, op, rs)
    return results
