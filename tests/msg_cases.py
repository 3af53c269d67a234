"""Payloads for the message-field decoder's tests (tests/test_msg_model.py on the host function and the CPU lane
model, tests/test_gpu_msg_batch.py and tests/test_gpu_rx_decode.py on the device) and a table-driven pure-Python
decoder written from the ITU-R M.1371 layouts as the project's issue states them -- not from
gr-ais_amd/csrc/aisx_msgtab.h, which it checks.

Message bit i is bit 7 - i % 8 of payload octet i // 8.  A field is decoded only when all of its bits lie inside
8 * len; unsigned fields are big-endian, signed ones two's complement over their own width; a six-bit character v is
the byte v + 64 for v < 32 and v otherwise."""
import numpy as np

NA = -(1 << 31)
COLUMNS = ("TYPE", "REPEAT", "MMSI", "FLAGS", "NAV_STATUS", "ROT", "SOG", "ACCURACY", "LON", "LAT", "COG", "HEADING",
           "SECOND", "MANEUVER", "RAIM", "RADIO", "IMO", "AIS_VERSION", "SHIPTYPE", "TO_BOW", "TO_STERN", "TO_PORT",
           "TO_STARBOARD", "EPFD", "YEAR", "MONTH", "DAY", "HOUR", "MINUTE", "DRAUGHT", "DTE", "PART", "AID_TYPE",
           "OFF_POSITION", "VIRTUAL_AID", "ASSIGNED", "CS_FLAGS")
STRINGS = {"callsign": 7, "name": 20, "destination": 20}
REC_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu

HEADER = "TYPE 0:6, REPEAT 6:2, MMSI 8:30"
# layout -> (minimum bits, fields as "NAME start:width[ s]")
LAYOUTS = {
    "pos_a": (168, "NAV_STATUS 38:4, ROT 42:8 s, SOG 50:10, ACCURACY 60:1, LON 61:28 s, LAT 89:27 s, COG 116:12, "
                   "HEADING 128:9, SECOND 137:6, MANEUVER 143:2, RAIM 148:1, RADIO 149:19"),
    "base": (168, "YEAR 38:14, MONTH 52:4, DAY 56:5, HOUR 61:5, MINUTE 66:6, SECOND 72:6, ACCURACY 78:1, LON 79:28 s, "
                  "LAT 107:27 s, EPFD 134:4, RAIM 148:1, RADIO 149:19"),
    "static": (424, "AIS_VERSION 38:2, IMO 40:30, callsign 70:42, name 112:120, SHIPTYPE 232:8, TO_BOW 240:9, "
                    "TO_STERN 249:9, TO_PORT 258:6, TO_STARBOARD 264:6, EPFD 270:4, MONTH 274:4, DAY 278:5, HOUR 283:5, "
                    "MINUTE 288:6, DRAUGHT 294:8, destination 302:120, DTE 422:1"),
    "pos_b": (168, "SOG 46:10, ACCURACY 56:1, LON 57:28 s, LAT 85:27 s, COG 112:12, HEADING 124:9, SECOND 133:6, "
                   "CS_FLAGS 141:6, RAIM 147:1, RADIO 148:20"),
    "pos_b_ext": (312, "SOG 46:10, ACCURACY 56:1, LON 57:28 s, LAT 85:27 s, COG 112:12, HEADING 124:9, SECOND 133:6, "
                       "name 143:120, SHIPTYPE 263:8, TO_BOW 271:9, TO_STERN 280:9, TO_PORT 289:6, TO_STARBOARD 295:6, "
                       "EPFD 301:4, RAIM 305:1, DTE 306:1, ASSIGNED 307:1"),
    "aton": (272, "AID_TYPE 38:5, name 43:120, ACCURACY 163:1, LON 164:28 s, LAT 192:27 s, TO_BOW 219:9, TO_STERN 228:9, "
                  "TO_PORT 237:6, TO_STARBOARD 243:6, EPFD 249:4, SECOND 253:6, OFF_POSITION 259:1, RAIM 268:1, "
                  "VIRTUAL_AID 269:1, ASSIGNED 270:1"),
    "24a": (160, "PART 38:2, name 40:120"),
    "24b": (168, "PART 38:2, SHIPTYPE 40:8, callsign 90:42, TO_BOW 132:9, TO_STERN 141:9, TO_PORT 150:6, "
                 "TO_STARBOARD 156:6"),
    "24x": (160, "PART 38:2"),
    "long": (96, "ACCURACY 38:1, RAIM 39:1, NAV_STATUS 40:4, LON 44:18 s, LAT 62:17 s, SOG 79:6, COG 85:9"),
    "none": (38, ""),
}
TYPE_LAYOUT = {1: "pos_a", 2: "pos_a", 3: "pos_a", 4: "base", 11: "base", 5: "static", 18: "pos_b", 19: "pos_b_ext",
               21: "aton", 27: "long"}
# a representative type value for building payloads of a layout, with the part number for type 24
LAYOUT_TYPE = {"pos_a": (1, None), "base": (4, None), "static": (5, None), "pos_b": (18, None), "pos_b_ext": (19, None),
               "aton": (21, None), "24a": (24, 0), "24b": (24, 1), "24x": (24, 2), "long": (27, None), "none": (6, None)}


def fields(layout):
    """[(name, start, width, signed)] of a layout, the common header first"""
    out = []
    for part in (HEADER + (", " + LAYOUTS[layout][1] if LAYOUTS[layout][1] else "")).split(", "):
        tok = part.split()
        start, width = (int(v) for v in tok[1].split(":"))
        out.append((tok[0], start, width, len(tok) > 2 and tok[2] == "s"))
    return out


def bits_of(payload):
    return np.unpackbits(np.frombuffer(bytes(payload), dtype=np.uint8))  # (most significant bit of every octet first)


def _uint(bits, start, width):
    v = 0
    for b in bits[start:start + width]:
        v = 2 * v + int(b)
    return v


def _from27(name, v):
    """type 27's coarse units -> class-A units, by exact integer multiplication"""
    if name in ("LON", "LAT"):
        return v * 1000
    if name == "SOG":
        return 1023 if v == 63 else v * 10
    if name == "COG":
        return 3600 if v == 511 else v * 10
    return v


def decode_bits(bits):
    """the decoder's result for a message given as an array of bits: {column: int} for every column, and the
    three strings as bytes (b"" where not carried)"""
    n = len(bits)
    out = {c: NA for c in COLUMNS}
    out.update({s: b"" for s in STRINGS})
    mtype = _uint(bits, 0, 6) if n >= 6 else None
    layout = TYPE_LAYOUT.get(mtype, "none")
    if mtype == 24:
        part = _uint(bits, 38, 2) if n >= 40 else None
        layout = {0: "24a", 1: "24b"}.get(part, "24x")
    for name, start, width, signed in fields(layout):
        if start + width > n:
            continue
        if name in STRINGS:
            six = [_uint(bits, start + 6 * k, 6) for k in range(STRINGS[name])]
            out[name] = bytes(v + 64 if v < 32 else v for v in six)
            continue
        v = _uint(bits, start, width)
        if signed and v >= 1 << (width - 1):
            v -= 1 << width
        out[name] = _from27(name, v) if layout == "long" else v
    out["FLAGS"] = (1 if n >= LAYOUTS[layout][0] else 0) | (2 if layout == "none" else 0)
    return out


def decode(payload):
    return decode_bits(bits_of(payload))


def sentence_bits(sentence):
    """the payload characters of one !AIVDM sentence -> bits (six per character)"""
    chars = sentence.split(",")[5]
    out = []
    for ch in chars.encode("latin-1"):
        v = ch - 48
        if v > 40:
            v -= 8
        out += [(v >> k) & 1 for k in range(5, -1, -1)]
    return np.array(out, dtype=np.uint8)


# sentences published with their decoded values (the offsets above were checked against them)
PUBLISHED = [
    ("177KQJ5000G?tO`K>RA1wUbN0TKH", dict(TYPE=1, MMSI=477553000, NAV_STATUS=5, ROT=0, SOG=0, LON=-73407500, LAT=28549700,
                                       COG=510, HEADING=181, SECOND=15, RADIO=149208)),
    ("13HOI:0P0000VOHLCnHQKwvL05Ip", dict(TYPE=1, MMSI=227006760, NAV_STATUS=0, ROT=-128, LON=78828, LAT=29685346, COG=367,
                                       HEADING=511, SECOND=14, RADIO=22136)),
    ("B52K>;h00Fc>jpUlNV@ikwpUoP06", dict(TYPE=18, MMSI=338087471, SOG=1, LON=-44443279, LAT=24410724, COG=796, HEADING=511,
                                       SECOND=49, RADIO=917510)),
]


def chars_to_payload(chars):
    """payload characters (a multiple of four, so whole octets) -> payload bytes"""
    b = sentence_bits(",,,,," + chars + ",0*00")
    assert len(b) % 8 == 0
    return np.packbits(b).tobytes()


# ---- case generator -----------------------------------------------------------------------------------------------
def _put(bits, start, width, v):
    for k in range(width):
        if start + k < len(bits):
            bits[start + k] = (v >> (width - 1 - k)) & 1


def build(layout, values, length, rng):
    """a payload of `length` octets of the layout's representative type: random bits, then the given field values
    ({name: transmitted integer, two's complement taken here; strings as lists of six-bit values})"""
    bits = rng.integers(0, 2, 8 * length).astype(np.uint8)
    mtype, part = LAYOUT_TYPE[layout]
    _put(bits, 0, 6, mtype)
    if part is not None:
        _put(bits, 38, 2, part)
    for name, start, width, signed in fields(layout):
        if name not in values or name == "TYPE" or (name == "PART"):
            continue
        if name in STRINGS:
            for k, v in enumerate(values[name]):
                _put(bits, start + 6 * k, 6, v)
        else:
            _put(bits, start, width, values[name] & ((1 << width) - 1))
    return np.packbits(bits).tobytes() if length else b""


# the not-available codes of the fields that have one (transmitted integers)
NOT_AVAILABLE = {"ROT": -128, "SOG": 1023, "LON": 181 * 600000, "LAT": 91 * 600000, "COG": 3600, "HEADING": 511, "SECOND": 60,
                 "NAV_STATUS": 15, "YEAR": 0, "MONTH": 0, "DAY": 0, "HOUR": 24, "MINUTE": 60, "EPFD": 0, "SHIPTYPE": 0,
                 "DRAUGHT": 0, "IMO": 0}
NOT_AVAILABLE_27 = {"LON": 181 * 600, "LAT": 91 * 600, "SOG": 63, "COG": 511, "NAV_STATUS": 15}


def _choices(layout):
    """four value sets for a layout: every field's zero, maximum, most negative value and not-available code"""
    zero, top, low, na = {}, {}, {}, {}
    na_codes = NOT_AVAILABLE_27 if layout == "long" else NOT_AVAILABLE
    for name, start, width, signed in fields(layout):
        if name in STRINGS:
            n = STRINGS[name]
            zero[name], top[name], low[name], na[name] = [0] * n, [63] * n, [32] * n, [31, 32] * (n // 2) + [0] * (n % 2)
            continue
        zero[name] = 0
        top[name] = (1 << (width - 1)) - 1 if signed else (1 << width) - 1
        low[name] = -(1 << (width - 1)) if signed else 1
        na[name] = na_codes.get(name, top[name])
    return [zero, top, low, na]


def layout_cases(rng):
    """for every layout and each of its four value sets: the minimum length minus one octet, the minimum length,
    plus one octet, and 62 octets"""
    out = []
    for layout, (min_bits, _) in LAYOUTS.items():
        m = (min_bits + 7) // 8
        for values in _choices(layout):
            for length in (m - 1, m, m + 1, 62):
                out.append(build(layout, values, length, rng))
    return out


def edge_cases(rng):
    out = []
    for length in (0, 1, 4, 5):  # the header boundary at 38 bits
        for mtype in (1, 5, 24, 6):
            out.append(build({1: "pos_a", 5: "static", 24: "24b", 6: "none"}[mtype], {}, length, rng))
    for length in (1, 5, 12, 20, 21, 34, 39, 53, 54, 62, 63):
        out.append(b"\x00" * length)
        out.append(b"\xff" * length)
    return out


def random_cases(rng, per_type=3):
    """random payloads of every type value 0..63, lengths 1..63"""
    out = []
    for mtype in range(64):
        for _ in range(per_type):
            p = bytearray(rng.integers(0, 256, int(rng.integers(1, 64))).astype(np.uint8).tobytes())
            p[0] = (mtype << 2) | (p[0] & 3)
            out.append(bytes(p))
    return out


def all_payloads(rng):
    return layout_cases(rng) + edge_cases(rng) + random_cases(rng)


def pack(payloads, rng, nchan=3, max_pdus=None, shuffle=True):
    """payloads -> (REC_DTYPE array, payload bytes): record i is payloads[i], the payloads laid out in a shuffled
    order with gaps of 0 .. 5 bytes of 0xA5 between them, so that offsets are neither ordered nor contiguous and a
    payload sits at every byte alignment"""
    n = len(payloads)
    recs = np.zeros(max(n, max_pdus or 0, 1), dtype=REC_DTYPE)
    order = rng.permutation(n) if shuffle else np.arange(n)
    data = bytearray(b"\xa5" * int(rng.integers(0, 4)))
    for i in order:
        p = payloads[i]
        recs[i] = (1000 + 3 * i, len(data), i % nchan, len(p))
        data += bytes(p) + b"\xa5" * int(rng.integers(0, 6))
    return recs, np.frombuffer(bytes(data) + b"\xa5" * 8, dtype=np.uint8).copy()


def row_of(d):
    """a decoded dict (this module's or ais_amd.msg_decode's) -> a comparable tuple"""
    return tuple(int(d[c]) for c in COLUMNS) + tuple(bytes(d[s]) for s in STRINGS)
