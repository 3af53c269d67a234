"""Shared case data of the NMEA parser's tests: an independent pure-Python parser of the grammar include/aisx.h states
(line by line, by regular expression; it owes nothing to the C++), a standard six-bit armourer, and seeded generators
of text that exercises every rule: fragments, fills, tag blocks, line ends, every reject reason, broken groups and
over-long lines."""
import re

import numpy as np

COUNT_NAMES = ("FOUND", "KEPT", "BAD_INPUT", "LINES", "SENTENCES", "REJ_FORMAT", "REJ_CHECKSUM", "REJ_CHANNEL",
               "REJ_ARMOUR", "REJ_FRAGMENT", "REJ_LENGTH", "CARRIED")
DESIGNATORS = ["A", "B", "", "CHANNEL-16-BYTES"]
LENGTH_MAX = 64
MAX_LINE = 128

_SENT = re.compile(rb"(?:\\([^\\]*)\\)?!([A-Z0-9]{2})VDM,([1-9]),([1-9]),([0-9]?),([^,*]{0,16}),([^,]*),([0-5])\*([0-9A-Fa-f]{2})",
                   re.DOTALL)
_TIME = re.compile(rb"c:[0-9]{1,18}")


def _armour_ok(c):
    return 48 <= c <= 87 or 96 <= c <= 119


class PyParser:
    """the specification, restated: feed(bytes) -> (records, counts) per call; a record is (chan, len, end_bit, time,
    payload bytes)"""

    def __init__(self, designators=DESIGNATORS, length_max=LENGTH_MAX, max_line=MAX_LINE, ref_tail=False):
        self.desig = [d.encode() if isinstance(d, str) else bytes(d) for d in designators]
        self.length_max, self.max_line, self.ref_tail = length_max, max_line, ref_tail
        self.reset()

    def reset(self):
        self.buf, self.line, self.group = b"", 0, []

    def _message(self, sents, cnt, out):
        chars = b"".join(s["payload"] for s in sents)
        nbits = 6 * len(chars) - sents[-1]["fill"]
        n = (nbits + 7) // 8
        if nbits <= 0 or n > self.length_max - 1:
            cnt["REJ_LENGTH"] += 1
            return
        bits = ""
        for k, c in enumerate(chars):
            v = c - 48
            if v > 40:
                v -= 8
            if k == len(chars) - 1 and sents[-1]["tail_zero"]:
                v = 0
            bits += format(v & 63, "06b")
        bits = (bits[:nbits] + "0" * 8)[: 8 * n].ljust(8 * n, "0")
        cnt["FOUND"] += 1
        out.append((sents[0]["chan"], n, sents[-1]["line"], sents[0]["time"], int(bits, 2).to_bytes(n, "big")))

    def _line(self, ln, cnt, out):
        idx = self.line
        self.line += 1
        cnt["LINES"] += 1
        if len(ln) > self.max_line:
            cnt["REJ_FORMAT"] += 1
            return
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            return
        m = _SENT.fullmatch(ln)
        if not m:
            cnt["REJ_FORMAT"] += 1
            return
        tag, _, F, f, s, chan, payload, fill, hh = m.groups()
        F, f, fill = int(F), int(f), int(fill)
        if f > F:
            cnt["REJ_FORMAT"] += 1
            return
        body = ln[ln.index(b"!", 0 if tag is None else len(tag) + 2):]
        x = 0
        for c in body[1:-3]:
            x ^= c
        if x != int(hh, 16):
            cnt["REJ_CHECKSUM"] += 1
            return
        if chan not in self.desig:
            cnt["REJ_CHANNEL"] += 1
            return
        tail_zero = bool(self.ref_tail and f == F and fill > 0 and payload)
        if not all(_armour_ok(c) for c in (payload[:-1] if tail_zero else payload)):
            cnt["REJ_ARMOUR"] += 1
            return
        time = -1
        if tag is not None:
            t = tag[: tag.rindex(b"*")] if b"*" in tag else tag
            for fld in t.split(b","):
                if _TIME.fullmatch(fld):
                    time = int(fld[2:])
                    break
        cnt["SENTENCES"] += 1
        sn = dict(F=F, f=f, s=s, chan=self.desig.index(chan), fill=fill, time=time, line=idx, payload=payload,
                  tail_zero=tail_zero, text_len=len(ln))
        if self.group:
            h = self.group[0]
            if f == len(self.group) + 1 and F == h["F"] and s == h["s"] and sn["chan"] == h["chan"]:
                self.group.append(sn)
                if len(self.group) == F:
                    self._message(self.group, cnt, out)
                    self.group = []
                return
            cnt["REJ_FRAGMENT"] += len(self.group)
            self.group = []
        if F == 1:
            self._message([sn], cnt, out)
        elif f == 1:
            self.group = [sn]
        else:
            cnt["REJ_FRAGMENT"] += 1

    def feed(self, data, pdu_cap=None, bytes_cap=None):
        cnt = dict.fromkeys(COUNT_NAMES, 0)
        out = []
        self.buf += bytes(data)
        lines = self.buf.split(b"\n")
        self.buf = lines.pop()
        for ln in lines:
            self._line(ln, cnt, out)
        cnt["CARRIED"] = (len(self.buf) if len(self.buf) <= self.max_line else 0) + sum(s["text_len"] for s in self.group)
        kept, nb = 0, 0
        for r in out:
            if (pdu_cap is not None and kept >= pdu_cap) or (bytes_cap is not None and nb + r[1] > bytes_cap):
                break
            kept, nb = kept + 1, nb + r[1]
        cnt["KEPT"] = kept
        return out[:kept], cnt


# ---------------------------------------------------------------------------------------------------------------------
def checksum(body):
    """body: b"!....." up to and excluding '*' -> the two upper-case hex digits"""
    x = 0
    for c in body[1:]:
        x ^= c
    return b"%02X" % x


def sentence(F, f, s, chan, payload, fill, talker=b"AI", tag=None, lower_hex=False, kind=b"VDM"):
    body = b"!" + talker + kind + b",%d,%d,%s,%s,%s,%d" % (F, f, s, chan, payload, fill)
    cs = checksum(body)
    line = body + b"*" + (cs.lower() if lower_hex else cs)
    if tag is not None:
        line = b"\\" + tag + b"\\" + line
    return line


def armour_chars(bits):
    """the standard six-bit armouring of a bit sequence: (characters, fill)"""
    bits = list(bits)
    fill = (6 - len(bits) % 6) % 6
    bits += [0] * fill
    out = bytearray()
    for k in range(0, len(bits), 6):
        v = int("".join(str(b) for b in bits[k:k + 6]), 2)
        out.append(v + 48 + (8 if v > 39 else 0))
    return bytes(out), fill


def armour_std(bits, chan=b"A", splits=None, s=b"", tag=None, lower_hex=False, fill_everywhere=False):
    """the lines (without line ends) of one message; splits: the fragments' character counts (default: 56 each)"""
    chars, fill = armour_chars(bits)
    if splits is None:
        splits = [56] * (len(chars) // 56) + ([len(chars) % 56] if len(chars) % 56 else [])
    assert sum(splits) == len(chars) and 1 <= len(splits) <= 9
    F, out, k = len(splits), [], 0
    for f, n in enumerate(splits, 1):
        last = f == F
        out.append(sentence(F, f, s, chan, chars[k:k + n], fill if (last or fill_everywhere) else 0,
                            tag=tag if f == 1 else None, lower_hex=lower_hex))
        k += n
    return out


def bits_to_octets(bits):
    b = list(bits) + [0] * (-len(bits) % 8)
    return bytes(int("".join(str(x) for x in b[k:k + 8]), 2) for k in range(0, len(b), 8))


def random_message(rng, length_max=LENGTH_MAX, nfrag=None, nbits=None):
    """a good message: (lines, expected octets)"""
    if nbits is None:
        nbits = int(rng.integers(1, 8 * (length_max - 1) + 1))
    bits = rng.integers(0, 2, nbits).tolist()
    nchar = (nbits + 5) // 6
    if nfrag is None:
        nfrag = int(rng.integers(1, 10))
    nfrag = min(nfrag, nchar)
    cuts = sorted(rng.choice(np.arange(1, nchar), nfrag - 1, replace=False).tolist()) if nfrag > 1 else []
    splits = [b - a for a, b in zip([0] + cuts, cuts + [nchar])]
    chan = DESIGNATORS[int(rng.integers(0, len(DESIGNATORS)))].encode()
    s = b"" if nfrag == 1 and rng.random() < 0.7 else b"%d" % rng.integers(0, 10)
    tag = None
    r = rng.random()
    if r < 0.15:
        tag = b"c:%d*5A" % rng.integers(0, 10 ** 10)
    elif r < 0.25:
        tag = b"s:rcv,g:1-2-3,c:%d,n:4*00" % rng.integers(0, 10 ** 18)
    elif r < 0.3:
        tag = b"s:station*1F"
    elif r < 0.33:
        tag = b"c:12x,c:,c:1234567890123456789,c:77"
    return armour_std(bits, chan, splits, s, tag, lower_hex=rng.random() < 0.3, fill_everywhere=rng.random() < 0.5), bits_to_octets(bits)




GOOD = sentence(1, 1, b"", b"A", b"15M67FC000G?ufbE`FepT@3n00Sa", 0)


def planted_rejects(max_line=MAX_LINE):
    """every single reject reason, one line each: [(name, line, count name)]"""
    pay = b"15M67FC000G?ufbE`FepT@3n00Sa"
    ok = sentence(1, 1, b"", b"A", pay, 0)
    F = "REJ_FORMAT"
    out = [
        ("checksum", ok[:-2] + (b"00" if ok[-2:] != b"00" else b"01"), "REJ_CHECKSUM"),
        ("channel", sentence(1, 1, b"", b"C", pay, 0), "REJ_CHANNEL"),
        ("channel-prefix", sentence(1, 1, b"", b"CHANNEL-16-BYTE", pay, 0), "REJ_CHANNEL"),
        ("armour-X", sentence(1, 1, b"", b"A", pay[:5] + b"X" + pay[6:], 0), "REJ_ARMOUR"),
        ("armour-x", sentence(1, 1, b"", b"A", pay[:5] + b"x" + pay[6:], 0), "REJ_ARMOUR"),
        ("armour-slash", sentence(1, 1, b"", b"A", b"/" + pay, 0), "REJ_ARMOUR"),
        ("armour-star", sentence(1, 1, b"", b"A", pay[:9] + b"*" + pay[9:], 0), "REJ_ARMOUR"),
        ("armour-last", sentence(1, 1, b"", b"A", pay + b"~", 2), "REJ_ARMOUR"),
        ("vdo", sentence(1, 1, b"", b"A", pay, 0, kind=b"VDO"), F),
        ("gpgga", b"$GPGGA,123519,4807.038,N,01131.000,E,1,08,0.9,545.4,M,46.9,M,,*47", F),
        ("talker-lower", sentence(1, 1, b"", b"A", pay, 0, talker=b"ai"), F),
        ("F-zero", sentence(0, 1, b"", b"A", pay, 0), F),
        ("f-zero", sentence(1, 0, b"", b"A", pay, 0), F),
        ("f-above-F", sentence(2, 3, b"1", b"A", pay, 0), F),
        ("fill-6", sentence(1, 1, b"", b"A", pay, 6), F),
        ("s-two-digits", sentence(1, 1, b"12", b"A", pay, 0), F),
        ("s-letter", sentence(1, 1, b"x", b"A", pay, 0), F),
        ("chan-17", sentence(1, 1, b"", b"CHANNEL-16-BYTES7", pay, 0), F),
        ("chan-star", sentence(1, 1, b"", b"A*", pay, 0), F),
        ("extra-comma", sentence(1, 1, b"", b"A", pay[:4] + b"," + pay[4:], 0), F),
        ("missing-field", b"!AIVDM,1,1,A," + pay + b",0*00", F),
        ("trailing", ok + b" ", F),
        ("one-hex", ok[:-1], F),
        ("hex-g", ok[:-1] + b"G", F),
        ("no-star", ok.replace(b"*", b"+"), F),
        ("short", b"!AIVDM,1,1,,,,0*5", F),
        ("bang-only", b"!", F),
        ("tag-open", b"\\c:123*00!" + ok[1:], F),
        ("tag-then-junk", b"\\c:1\\x" + ok, F),
        ("leading-space", b" " + ok, F),
        ("cr-inside", ok[:20] + b"\r" + ok[20:], "REJ_CHECKSUM"),
        ("length-long", armour_std([1] * (8 * LENGTH_MAX), b"A", [86])[0], "REJ_LENGTH"),
        ("length-zero", sentence(1, 1, b"", b"A", b"", 0), "REJ_LENGTH"),
        ("length-negative", sentence(1, 1, b"", b"A", b"", 3), "REJ_LENGTH"),
        ("length-fill-eats-all", sentence(1, 1, b"", b"A", b"0", 5), None),  # one bit: a message
        ("overlong", b"#" * (max_line + 1), F),
        ("overlong-cr", b"#" * max_line + b"\r", F),
        ("overlong-5x", b"\\" * (5 * max_line), F),
    ]
    return out


def padded_to(line_len, rng=None):
    """a good single sentence of exactly line_len bytes: a tag block pads it"""
    base = sentence(1, 1, b"", b"B", b"15M67FC000G?ufbE`FepT@3n00Sa", 0)
    pad = line_len - len(base) - 2
    assert pad >= 8
    tag = b"c:4242," + b"t" * (pad - 7)
    return b"\\" + tag + b"\\" + base


def broken_groups(rng):
    """[(name, lines, messages expected, fragments rejected)]"""
    def frags(s=b"3", chan=b"A", F=3):
        bits = rng.integers(0, 2, 6 * 10 * F).tolist()
        return armour_std(bits, chan, [10] * F, s)

    a, b = frags(), frags()
    single = armour_std(rng.integers(0, 2, 168).tolist(), b"B")
    out = [
        ("whole", a, 1, 0),
        ("missing-2", [a[0], a[2]], 0, 2),
        ("missing-last-then-single", [a[0], a[1]] + single, 1, 2),
        ("repeated", [a[0], a[1], a[1], a[2]], 0, 4),
        ("out-of-order", [a[0], a[2], a[1]], 0, 3),
        ("changed-s", [a[0], frags(b"4")[1], a[2]], 0, 3),
        ("changed-s-empty", [a[0], frags(b"")[1], a[2]], 0, 3),
        ("changed-F", [a[0], frags(F=4)[1], a[2]], 0, 3),
        ("changed-chan", [a[0], frags(chan=b"B")[1], a[2]], 0, 3),
        ("new-head-inside", [a[0], a[1], b[0], b[1], b[2]], 1, 2),
        ("head-after-head", [a[0], b[0], b[1], b[2]], 1, 1),
        ("orphan-tail", [a[2]], 0, 1),
        ("reject-inside-does-not-break", [a[0], b"$GPGGA,1*00", a[1], b"", GOOD[:-1] + b"0", a[2]], 1, 0),
        ("single-inside-breaks", [a[0]] + single + [a[1], a[2]], 1, 3),
    ]
    return out


def text600():
    """about 600 bytes, eight lines: singles, a three-fragment group, a tag block, a reject, \\r\\n and an empty line"""
    rng = np.random.default_rng(600)
    g = armour_std(rng.integers(0, 2, 502).tolist(), b"B", [40, 30, 14], b"7",
                   tag=b"s:station-north-7,g:1-3-9912,c:1700000000,n:12345*2B")
    gga = b"$GPGGA,123519,4807.038,N,01131.000,E,1,08,0.9,545.4,M,46.9,M,,*47"
    lines = [b"\\s:station-north-7,n:12344*11\\" + GOOD + b"\r", g[0], g[1], b"", g[2] + b"\r", gga,
             sentence(1, 1, b"", b"CHANNEL-16-BYTES", b"H52KMeDU653hhhi0000000000000", 2, tag=b"c:99"),
             armour_std(rng.integers(0, 2, 8 * 63 - 2).tolist(), b"", [84], lower_hex=True)[0]]
    return b"".join(ln + b"\n" for ln in lines)


def build_cases(max_line=MAX_LINE):
    """[(name, text)]: every case is a whole text ending in a line end"""
    rng = np.random.default_rng(20240611)
    cases = []

    def text(lines, cr=False):
        return b"".join(ln + (b"\r\n" if cr else b"\n") for ln in lines)

    cases.append(("text600", text600()))
    for name, ln, _ in planted_rejects(max_line):
        cases.append(("reject-" + name, text([GOOD, ln, GOOD])))
    for name, lines, _, _ in broken_groups(rng):
        cases.append(("group-" + name, text(lines)))
    for n in (max_line, max_line - 1):
        cases.append(("line-%d" % n, text([padded_to(n)])))
    cases.append(("line-%d-cr" % (max_line - 1), text([padded_to(max_line - 1)], cr=True)))
    cases.append(("line-%d-cr" % max_line, text([padded_to(max_line)], cr=True)))  # one byte too long
    for nf in range(1, 10):
        lines, _ = random_message(rng, nfrag=nf, nbits=8 * 63 - nf)
        cases.append(("frags-%d" % nf, text(lines, cr=nf % 2 == 0)))
    for fill in range(6):
        lines, _ = random_message(rng, nfrag=2, nbits=6 * 20 - fill)
        cases.append(("fill-%d" % fill, text(lines)))
    # a long mixed stream
    lines = []
    rej = planted_rejects(max_line)
    brk = broken_groups(rng)
    for _ in range(160):
        r = rng.random()
        if r < 0.55:
            lines += random_message(rng)[0]
        elif r < 0.7:
            lines.append(rej[int(rng.integers(0, len(rej)))][1])
        elif r < 0.8:
            lines += brk[int(rng.integers(0, len(brk)))][1]
        elif r < 0.85:
            lines.append(b"")
        elif r < 0.9:
            lines.append(padded_to(int(rng.integers(max_line - 20, max_line + 1))))
        else:
            lines.append(bytes(rng.integers(0, 256, int(rng.integers(1, 90)), dtype=np.uint8)).replace(b"\n", b"?"))
    cases.append(("mixed", b"".join(ln + (b"\r\n" if rng.random() < 0.3 else b"\n") for ln in lines)))
    return cases


def random_cuts(rng, n, k):
    """k sorted cut positions in [0, n], ends added: the pieces' bounds"""
    c = sorted(rng.integers(0, n + 1, k).tolist())
    return [0] + c + [n]


def pieces(text, bounds):
    return [text[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


def mutations(rng, text, count):
    """seeded byte-level mutations of a text: truncations, random bytes, deletions, duplicated stretches"""
    out = []
    for _ in range(count):
        t = bytearray(text)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            t = t[: int(rng.integers(0, len(t) + 1))]
        elif kind == 1:
            for _ in range(int(rng.integers(1, 8))):
                t[int(rng.integers(0, len(t)))] = int(rng.integers(0, 256))
        elif kind == 2:
            a = int(rng.integers(0, len(t)))
            del t[a:a + int(rng.integers(1, 20))]
        else:
            a = int(rng.integers(0, len(t)))
            b = a + int(rng.integers(1, 40))
            t[a:a] = t[a:b]
        out.append(bytes(t))
    return out


def as_tuples(recs, data, times):
    """what the C forms return -> PyParser's record tuples"""
    return [(int(r["chan"]), int(r["len"]), int(r["end_bit"]), int(t), bytes(data[int(r["offset"]):int(r["offset"]) + int(r["len"])]))
            for r, t in zip(recs, times)]
