"""Host-side tail of the receive chain (python/radio.py:64-73): the HDLC deframer
`digital.hdlc_deframer_bp(11, 64)` and `ais.pdu_to_nmea(designator)`
(lib/pdu_to_nmea_impl.cc), and behind them the ITU-R M.1371 field decoder
`msg_decode`.  Per-packet work on the CPU, in libaisx.so's host code; no GPU
needed."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


RULE_DTYPE = np.dtype([("payload_octets", "<i4"), ("reserved", "<i4"), ("type_mask", "<u8")])  # aisx_hdlc_rule
ANY_TYPE = (1 << 64) - 1
# Single-bit repair rules for the ITU-R M.1371 messages of fixed length: {payload octets: the message types sent at that
# length}.  168 bits: 1-3 and 4 / 11, 9, 18, 24 part B; 424: 5; 312: 19; 160: 24 part A; 96: 27.
AIS_REPAIR_RULES = {21: (1, 2, 3, 4, 9, 11, 18, 24), 53: (5,), 39: (19,), 20: (24,), 12: (27,)}
# The error events a repair can look for (a mask; include/aisx.h, AISX_HDLC_EV_*): one wrong bit, two adjacent wrong bits
# (one wrong decision of the differential slicer) and two wrong bits two apart (the sequence detector's error event).
# events= everywhere defaults to REPAIR_SINGLE, the single-bit repair; AIS_REPAIR_EVENTS holds all three.
REPAIR_SINGLE, REPAIR_PAIR, REPAIR_SKIP = _lib.AISX_HDLC_EV_SINGLE, _lib.AISX_HDLC_EV_PAIR, _lib.AISX_HDLC_EV_SKIP
AIS_REPAIR_EVENTS = REPAIR_SINGLE | REPAIR_PAIR | REPAIR_SKIP
_PATTERNS = ((1,), (1, 1), (1, 0, 1))  # by event id, the first flipped bit first


def repair_mark(mark):
    """a repair mark (work(with_repairs=True), pdus(with_repairs=True), popped_repairs()) -> (first_bit, pattern_bits):
    the index in the frame (payload + FCS, bit 0 the first received) of the first flipped bit, and the pattern that was
    flipped from there on as a tuple of 0 / 1 -- (1,), (1, 1) or (1, 0, 1); (-1, ()) for a frame delivered as received"""
    mark = int(mark)
    if mark < 0:
        return -1, ()
    if (mark >> 16) >= len(_PATTERNS):
        raise ValueError("repair_mark: %d is not a repair mark" % mark)
    return mark & 0xFFFF, _PATTERNS[mark >> 16]


def event_table(events):
    """aisx_hdlc_event_table: uint16 [65536], for every FCS syndrome the enabled event nearest the frame's end as
    id << 14 | distance of its last flipped bit + 1, 0 for none"""
    t = np.zeros(65536, dtype=np.uint16)
    check(_lib.lib(device=False).aisx_hdlc_event_table(int(events), t.ctypes.data_as(C.c_void_p)), "event_table")
    return t


def repair_rules(rules):
    """rules as the deframers take them -> an aisx_hdlc_rule array: None or empty (repair off), a dict {payload octets:
    iterable of message types, or None / ANY_TYPE for any content}, or a sequence of (payload octets, type mask)"""
    if rules is None:
        return np.zeros(0, dtype=RULE_DTYPE)
    if isinstance(rules, np.ndarray) and rules.dtype == RULE_DTYPE:
        return np.ascontiguousarray(rules)
    items = list(rules.items()) if isinstance(rules, dict) else list(rules)
    out = np.zeros(len(items), dtype=RULE_DTYPE)
    for k, (octets, types) in enumerate(items):
        if types is None:
            types = ANY_TYPE
        if not isinstance(types, (int, np.integer)):
            mask = 0
            for t in types:
                if not 0 <= int(t) < 64:
                    raise ValueError("repair rules: a message type is 0..63, got %r" % (t,))
                mask |= 1 << int(t)
            types = mask
        out[k] = (int(octets), 0, int(types) & ANY_TYPE)
    return out


class hdlc_deframer_bp:
    """digital.hdlc_deframer_bp(length_min, length_max).  repair: repair rules (repair_rules() says how they are
    written, AIS_REPAIR_RULES is a ready set): a frame whose CRC fails by one wrong bit -- with events=, by one of the
    error events of that mask (AIS_REPAIR_EVENTS: all) -- of a length and message type the rules allow, is put right
    and delivered; work(bits, with_repairs=True) marks those."""

    def __init__(self, length_min, length_max, repair=None, events=REPAIR_SINGLE):
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_hdlc_create(C.byref(h), int(length_min), int(length_max)), "hdlc_deframer_bp")
        self._h = h
        self._max = int(length_max)
        if repair is not None:
            self.set_repair(repair, events)

    def set_repair(self, rules, events=REPAIR_SINGLE):
        """from the next frame that closes on; None or empty: off.  ValueError for rules the handle cannot take (more
        than 16, a length outside [length_min - 2, length_max - 2] or given twice) or a mask that is 0 or has unknown
        bits: it keeps what it had."""
        r = repair_rules(rules)
        L = _lib.lib(device=False)
        if events == REPAIR_SINGLE:
            rc = L.aisx_hdlc_set_repair(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size)
        else:
            rc = L.aisx_hdlc_set_repair_events(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size, int(events))
        check(rc, "hdlc_deframer_bp.set_repair")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib(device=False).aisx_hdlc_destroy(h)
            self._h = None

    def work(self, bits, with_repairs=False):
        """bits: unpacked bits (one per item).  Returns the list of PDUs (bytes) whose CRC checked -- or, with repair
        rules, was made to by flipping one bit or one error event.  with_repairs=True: (PDUs, marks), a mark -1 for a
        frame delivered as received, else the index of the first flipped bit in the frame (payload + FCS, bit 0 the
        first received) | event id << 16: for a single bit its index, and repair_mark() reads any."""
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        maxp = b.size // 16 + 2
        buf = np.zeros(maxp * (self._max + 2), dtype=np.uint8)
        offs = np.zeros(maxp + 1, dtype=np.int32)
        n = C.c_int(0)
        if not with_repairs:
            check(_lib.lib(device=False).aisx_hdlc_work(self._h, b.ctypes.data_as(C.c_void_p), b.size, buf.ctypes.data_as(C.c_void_p),
                                            buf.size, offs.ctypes.data_as(C.c_void_p), maxp, C.byref(n)), "hdlc work")
            return [bytes(buf[offs[k]:offs[k + 1]]) for k in range(n.value)]
        fix = np.full(maxp, -1, dtype=np.int32)
        check(_lib.lib(device=False).aisx_hdlc_work_repair(self._h, b.ctypes.data_as(C.c_void_p), b.size, buf.ctypes.data_as(C.c_void_p),
                                                           buf.size, offs.ctypes.data_as(C.c_void_p), fix.ctypes.data_as(C.c_void_p),
                                                           maxp, C.byref(n)), "hdlc work")
        return [bytes(buf[offs[k]:offs[k + 1]]) for k in range(n.value)], [int(v) for v in fix[: n.value]]


class mlse_detector:
    """The 4-state sequence detector behind the timing recovery, on the host (aisx_mlse_*): the recovery's symbols (one
    per symbol, complex64) to the bit stream the demod's bit tail gives (NRZI decoded, inverted; bit n belongs to symbol
    n), the levels decided by a Viterbi search over the differential phase of BT = bt GMSK instead of one phase step
    each.  Blocks of 64 symbols are decided once 16 more have arrived: work() returns the bits of the blocks that
    became complete (any split of a stream into calls gives the same bits), flush() those of the rest and leaves the
    detector as new.

        bits = np.concatenate([det.work(syms), det.flush()])
        pdus = ais_amd.hdlc_deframer_bp(11, 64).work(bits)"""

    def __init__(self, bt=0.4):
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_mlse_create(C.byref(h), float(bt)), "mlse_detector")
        self._h = h
        self.bt = float(bt)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib(device=False).aisx_mlse_destroy(h)
            self._h = None

    def model(self):
        """(c0, c1, rot): the phase a level adds to its own symbol and to each neighbour, in quarter turns, and the
        float32 (cos, sin) of the eight level triples as rot[p][q][r]"""
        c0, c1 = C.c_double(), C.c_double()
        rot = np.zeros((2, 2, 2, 2), dtype=np.float32)
        check(_lib.lib(device=False).aisx_mlse_model(self._h, C.byref(c0), C.byref(c1), rot.ctypes.data_as(C.c_void_p)), "mlse_detector.model")
        return c0.value, c1.value, rot

    def reset(self):
        check(_lib.lib(device=False).aisx_mlse_reset(self._h), "mlse_detector.reset")

    def work(self, syms):
        s = np.ascontiguousarray(syms, dtype=np.complex64).ravel()
        bits = np.zeros(s.size + _lib.MLSE_BLOCK + _lib.MLSE_OVERLAP, dtype=np.uint8)
        n = C.c_int(0)
        check(_lib.lib(device=False).aisx_mlse_work(self._h, s.ctypes.data_as(C.c_void_p), s.size, bits.ctypes.data_as(C.c_void_p),
                                                    bits.size, C.byref(n)), "mlse_detector.work")
        return bits[: n.value].copy()

    def flush(self):
        bits = np.zeros(_lib.MLSE_BLOCK + _lib.MLSE_OVERLAP, dtype=np.uint8)
        n = C.c_int(0)
        check(_lib.lib(device=False).aisx_mlse_flush(self._h, bits.ctypes.data_as(C.c_void_p), bits.size, C.byref(n)), "mlse_detector.flush")
        return bits[: n.value].copy()


class pdu_to_nmea:
    """`ais.pdu_to_nmea(designator)`: msg_to_sentence(pdu) gives the reference's text byte for byte, its three defects
    included (a wrong last payload character when len % 3 != 0, the fill count on every fragment, no message id).
    standard=True gives the standard form instead (aisx_pdu_to_nmea_std, include/aisx.h): exact armouring, the fill
    count on the last fragment, a tag block \\s:station,c:time*HH\\ before every fragment (station: 0..15 bytes of A-Z
    a-z 0-9 _ -; time: -1 for none, else 0 .. 10^18 - 1) and, on messages of more than one sentence, a message id that
    the object counts 0..9 round (next_id; msg_to_sentence(pdu, time=...) overrides the time for one message).  At most
    378 octets in that form."""

    def __init__(self, designator, standard=False, station="", time=-1):
        self.designator = str(designator)
        self.standard, self.station, self.time = bool(standard), str(station), int(time)
        self.next_id = 0

    def msg_to_sentence(self, pdu, time=None):
        p = np.frombuffer(bytes(pdu), dtype=np.uint8)
        out = C.create_string_buffer(4096)
        if self.standard:
            n = check(_lib.lib(device=False).aisx_pdu_to_nmea_std(self.designator.encode(), p.ctypes.data_as(C.c_void_p), p.size,
                                                                  self.next_id, self.station.encode(),
                                                                  self.time if time is None else int(time), out, 4096),
                      "pdu_to_nmea")
            if 6 * 56 < 8 * p.size:  # (more than one sentence: the id is taken)
                self.next_id = (self.next_id + 1) % 10
            return out.raw[:n].decode("latin-1")
        n = check(_lib.lib(device=False).aisx_pdu_to_nmea(self.designator.encode(), p.ctypes.data_as(C.c_void_p), p.size, out, 4096),
                  "pdu_to_nmea")
        return out.raw[:n].decode("latin-1")


def _designators(designators):
    if isinstance(designators, (str, bytes)):
        designators = [designators]
    return [d.encode() if isinstance(d, str) else bytes(d) for d in designators]


_PDU_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu


class nmea_to_pdu:
    """!AIVDM text back into PDUs on the host (aisx_nmea_parse_*, whose grammar include/aisx.h states): the inverse of
    pdu_to_nmea for text from anywhere -- archives, other receivers, ais_rx's own output.  designators: the channel
    field's text per channel index (a sentence whose field equals none is rejected); messages of at most
    length_max - 1 octets; lines of at most max_line bytes.  The text is a byte stream: work() takes it in pieces cut
    anywhere, an open multi-sentence group and a partial line wait for the next call.  ref_tail=True reads this
    project's own armouring, whose last payload character is not standard when fill > 0: that character then counts
    as six zero bits.

        recs, data, times, counts = ais_amd.nmea_to_pdu(["A", "B"], 64).work(text)

    recs: a PDU_DTYPE array (chan, len, offset into data, end_bit = line index of the message's last sentence);
    times: the tag block's c: value of each message's first sentence, -1 without one; counts: a dict by the names of
    _lib.AISX_NMEAP_NAMES.  The last line must end in a newline to be seen: there is no flush."""

    def __init__(self, designators, length_max, max_line=512, ref_tail=False):
        d = _designators(designators)
        arr = (C.c_char_p * len(d))(*d)
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_nmea_parse_create(C.byref(h), arr, len(d), int(length_max), int(max_line),
                                                            _lib.AISX_NMEA_PARSE_REF_TAIL if ref_tail else 0), "nmea_to_pdu")
        self._h = h
        self.length_max, self.max_line = int(length_max), int(max_line)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib(device=False).aisx_nmea_parse_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib(device=False).aisx_nmea_parse_reset(self._h), "nmea_to_pdu.reset")

    def work(self, text, pdu_cap=None, bytes_cap=None, overflow_ok=False):
        """text: bytes.  pdu_cap / bytes_cap: by default what the text can hold at most, so nothing overflows; with
        smaller ones OverflowError when not every message was kept -- or with overflow_ok=True the prefix that was
        (counts tells FOUND and KEPT).  The state advances either way."""
        t = bytes(text)
        if pdu_cap is None:
            pdu_cap = t.count(b"\n") + 1
        if bytes_cap is None:
            bytes_cap = pdu_cap * (self.length_max - 1)
        recs = np.zeros(max(pdu_cap, 1), dtype=_PDU_DTYPE)
        data = np.zeros(max(bytes_cap, 1), dtype=np.uint8)
        times = np.zeros(max(pdu_cap, 1), dtype=np.int64)
        cnt = np.zeros(_lib.AISX_NMEAP_NCNT, dtype=np.int32)
        rc = _lib.lib(device=False).aisx_nmea_parse_work(self._h, t, len(t), recs.ctypes.data_as(C.c_void_p), int(pdu_cap),
                                                         data.ctypes.data_as(C.c_void_p), int(bytes_cap),
                                                         times.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "nmea_to_pdu.work")
        k = int(cnt[1])
        recs = recs[:k].copy()
        nb = int(recs["offset"][-1] + recs["len"][-1]) if k else 0
        return recs, data[:nb].copy(), times[:k].copy(), {n: int(v) for n, v in zip(_lib.AISX_NMEAP_NAMES, cnt)}


# what a duplicate suppression's call reports, in the order of include/aisx.h's AISX_DEDUP_CNT_*
DEDUP_COUNTS = ("in", "kept", "dup_call", "dup_window", "bad_len")


def dedup_key(payload):
    """aisx_dedup_key: the 64-bit key two payloads share when the duplicate suppression takes them for the same"""
    p = np.frombuffer(bytes(payload), dtype=np.uint8)
    k = C.c_uint64(0)
    check(_lib.lib(device=False).aisx_dedup_key(p.ctypes.data_as(C.c_void_p), p.size, C.byref(k)), "dedup_key")
    return k.value


class pdu_dedup:
    """PDUs heard by several receivers, suppressed on the host (aisx_dedup_*, plain C++: the specification of
    pdu_dedup_batch, include/aisx.h states the rule): of the records of a call that carry one payload the first is kept
    and counts the others; a payload kept in one of the last `window` calls (0..15) is suppressed altogether, and a
    suppressed payload does not renew what is remembered.  A record of more than length_max - 1 octets is passed
    through.  Stamps must rise from call to call (IndexError otherwise, and nothing changes).

        dd = ais_amd.pdu_dedup(window=2)
        kept, first, copies = dd.work(payloads, stamp)   # payloads[k] for k in kept: what to deliver
        dd.counts                                        # {"in", "kept", "dup_call", "dup_window", "bad_len"}

    first[i]: the position in `kept` of the record that stands for payload i, or -1 - age when it was kept `age` calls
    ago; copies[j]: how many records of this call kept[j] stands for."""

    def __init__(self, window, length_max=64):
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_dedup_create(C.byref(h), int(window), int(length_max)), "pdu_dedup")
        self._h = h
        self.window, self.length_max = int(window), int(length_max)
        self.counts = dict.fromkeys(DEDUP_COUNTS, 0)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib(device=False).aisx_dedup_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib(device=False).aisx_dedup_reset(self._h), "pdu_dedup.reset")

    def work_records(self, recs, data, stamp, marks=None):
        """recs: a PDU_DTYPE array whose offset / len point into data (uint8); marks: one int32 per record, carried along.
        Returns (kept records, first, copies, kept marks or None) and sets self.counts."""
        r = np.ascontiguousarray(recs, dtype=_PDU_DTYPE)
        d = np.ascontiguousarray(data, dtype=np.uint8)
        n = len(r)
        m = np.ascontiguousarray(marks, dtype=np.int32) if marks is not None else None
        if m is not None and len(m) < n:
            raise ValueError("pdu_dedup.work_records: %d marks for %d records" % (len(m), n))
        out, first = np.zeros(max(n, 1), dtype=_PDU_DTYPE), np.zeros(max(n, 1), dtype=np.int32)
        copies, om = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        cnt = np.zeros(len(DEDUP_COUNTS), dtype=np.int32)
        check(_lib.lib(device=False).aisx_dedup_update(self._h, r.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), n,
                                                       m.ctypes.data_as(C.c_void_p) if m is not None else None, int(stamp),
                                                       out.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p),
                                                       copies.ctypes.data_as(C.c_void_p), om.ctypes.data_as(C.c_void_p),
                                                       cnt.ctypes.data_as(C.c_void_p)), "pdu_dedup.work")
        self.counts = {k: int(v) for k, v in zip(DEDUP_COUNTS, cnt)}
        k = int(cnt[1])
        return out[:k].copy(), first[:n].copy(), copies[:k].copy(), om[:k].copy() if m is not None else None

    def work(self, payloads, stamp):
        """payloads: a sequence of bytes.  Returns (kept_indices, first, copies) as int32 arrays and sets self.counts."""
        payloads = [bytes(p) for p in payloads]
        recs = np.zeros(len(payloads), dtype=_PDU_DTYPE)
        recs["len"] = [len(p) for p in payloads]
        recs["offset"] = np.concatenate([[0], np.cumsum(recs["len"])[:-1]]) if len(payloads) else []
        recs["end_bit"] = np.arange(len(payloads))  # (carried along: which input record a kept one was)
        data = np.frombuffer(b"".join(payloads) + b"\0", dtype=np.uint8)
        out, first, copies, _ = self.work_records(recs, data, stamp)
        return out["end_bit"].astype(np.int32), first, copies


# the columns of a decoded message, in the order of include/aisx.h's AISX_MSG_COL_*
MSG_COLUMNS = ("TYPE", "REPEAT", "MMSI", "FLAGS", "NAV_STATUS", "ROT", "SOG", "ACCURACY", "LON", "LAT", "COG", "HEADING",
               "SECOND", "MANEUVER", "RAIM", "RADIO", "IMO", "AIS_VERSION", "SHIPTYPE", "TO_BOW", "TO_STERN", "TO_PORT",
               "TO_STARBOARD", "EPFD", "YEAR", "MONTH", "DAY", "HOUR", "MINUTE", "DRAUGHT", "DTE", "PART", "AID_TYPE",
               "OFF_POSITION", "VIRTUAL_AID", "ASSIGNED", "CS_FLAGS")
MSG_NA = _lib.AISX_MSG_NA
# one row on the host: an int32 per column (lower-case names) and the three strings
MSG_DTYPE = np.dtype([(c.lower(), "<i4") for c in MSG_COLUMNS] + [("callsign", "S7"), ("name", "S20"), ("destination", "S20")])


def msg_strings(strs):
    """a row's 48 bytes of strings -> (callsign, name, destination) as bytes of 7, 20 and 20 characters ('@' and
    blanks kept), b"" where the message does not carry the string (the slot is all NUL): what a MSG_DTYPE row gives"""
    b = bytes(strs)
    return b[0:7].rstrip(b"\0"), b[8:28].rstrip(b"\0"), b[28:48].rstrip(b"\0")


def msg_decode(payload):
    """aisx_msg_decode for one PDU: a dict with every column of MSG_COLUMNS as an int (the transmitted integer,
    MSG_NA where the message does not carry the field or the payload does not hold all of its bits) and "callsign",
    "name", "destination" as bytes"""
    p = np.frombuffer(bytes(payload), dtype=np.uint8)
    cols = np.zeros(len(MSG_COLUMNS), dtype=np.int32)
    strs = np.zeros(_lib.AISX_MSG_STR, dtype=np.uint8)
    check(_lib.lib(device=False).aisx_msg_decode(p.ctypes.data_as(C.c_void_p), p.size, cols.ctypes.data_as(C.c_void_p),
                                                 strs.ctypes.data_as(C.c_void_p)), "msg_decode")
    out = {name: int(v) for name, v in zip(MSG_COLUMNS, cols)}
    out["callsign"], out["name"], out["destination"] = msg_strings(strs)
    return out


MSG_ENC_NO_MMSI, MSG_ENC_NO_LAYOUT, MSG_ENC_RANGE = _lib.AISX_MSG_ENC_NO_MMSI, _lib.AISX_MSG_ENC_NO_LAYOUT, _lib.AISX_MSG_ENC_RANGE
MSG_ENC_BAD_CHAR, MSG_ENC_BAD_ROW = _lib.AISX_MSG_ENC_BAD_CHAR, _lib.AISX_MSG_ENC_BAD_ROW


def msg_row(row):
    """a msg_decode dict or one MSG_DTYPE record -> (int32 cols [ncol], uint8 strs [48]); a column the dict does not
    name is MSG_NA, a string it does not name is empty"""
    is_dict = isinstance(row, dict)
    cols = np.full(len(MSG_COLUMNS), MSG_NA, dtype=np.int32)
    strs = np.zeros(_lib.AISX_MSG_STR, dtype=np.uint8)
    for k, c in enumerate(MSG_COLUMNS):
        if not is_dict:
            cols[k] = row[c.lower()]
        elif c in row:
            cols[k] = row[c]
    for name, lo, w in (("callsign", 0, 7), ("name", 8, 20), ("destination", 28, 20)):
        s = bytes(row[name]) if not is_dict or name in row else b""
        if len(s) > w:
            raise ValueError("msg_encode: %s holds %d characters, the slot %d" % (name, len(s), w))
        strs[lo:lo + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return cols, strs


def msg_encode(row, as_type=0, as_part=-1):
    """aisx_msg_encode, the inverse of msg_decode: a msg_decode dict or one MSG_DTYPE record -> (payload bytes,
    status).  The type is as_type when that is in 1..63, else the row's TYPE; for type 24 the part is as_part when
    that is >= 0, else the row's PART.  A column that is MSG_NA takes the protocol's "not available" value.  status
    is 0 or a sum of MSG_ENC_* (NO_MMSI, NO_LAYOUT, RANGE, BAD_CHAR); the payload of a refused row is b""."""
    cols, strs = msg_row(row)
    pdu = np.zeros(_lib.AISX_MSG_ENC_PITCH, dtype=np.uint8)
    n, st = C.c_int(0), C.c_int(0)
    check(_lib.lib(device=False).aisx_msg_encode(cols.ctypes.data_as(C.c_void_p), strs.ctypes.data_as(C.c_void_p), int(as_type),
                                                 int(as_part), pdu.ctypes.data_as(C.c_void_p), pdu.size, C.byref(n), C.byref(st)),
          "msg_encode")
    return pdu[: n.value].tobytes(), st.value


def msg_table(cols, strs, n):
    """int32 [ncol][>= n] and uint8 [>= n][48] on the host -> a MSG_DTYPE array of n rows"""
    out = np.zeros(n, dtype=MSG_DTYPE)
    for k, c in enumerate(MSG_COLUMNS):
        out[c.lower()] = cols[k, :n]
    s = np.ascontiguousarray(strs[:n])
    out["callsign"] = s[:, 0:7].copy().view("S7").ravel()
    out["name"] = s[:, 8:28].copy().view("S20").ravel()
    out["destination"] = s[:, 28:48].copy().view("S20").ravel()
    return out
