"""Host-side tail of the receive chain (python/radio.py:64-73): the HDLC deframer
`digital.hdlc_deframer_bp(11, 64)` and `ais.pdu_to_nmea(designator)`
(lib/pdu_to_nmea_impl.cc), and behind them the ITU-R M.1371 field decoder
`msg_decode`.  Per-packet work on the CPU, in libaisx.so's host code; no GPU
needed."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


class hdlc_deframer_bp:
    def __init__(self, length_min, length_max):
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_hdlc_create(C.byref(h), int(length_min), int(length_max)), "hdlc_deframer_bp")
        self._h = h
        self._max = int(length_max)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib(device=False).aisx_hdlc_destroy(h)
            self._h = None

    def work(self, bits):
        """bits: unpacked bits (one per item).  Returns the list of PDUs (bytes) whose CRC checked."""
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        maxp = b.size // 16 + 2
        buf = np.zeros(maxp * (self._max + 2), dtype=np.uint8)
        offs = np.zeros(maxp + 1, dtype=np.int32)
        n = C.c_int(0)
        check(_lib.lib(device=False).aisx_hdlc_work(self._h, b.ctypes.data_as(C.c_void_p), b.size, buf.ctypes.data_as(C.c_void_p),
                                        buf.size, offs.ctypes.data_as(C.c_void_p), maxp, C.byref(n)), "hdlc work")
        return [bytes(buf[offs[k]:offs[k + 1]]) for k in range(n.value)]


class pdu_to_nmea:
    def __init__(self, designator):
        self.designator = str(designator)

    def msg_to_sentence(self, pdu):
        p = np.frombuffer(bytes(pdu), dtype=np.uint8)
        out = C.create_string_buffer(4096)
        n = check(_lib.lib(device=False).aisx_pdu_to_nmea(self.designator.encode(), p.ctypes.data_as(C.c_void_p), p.size, out, 4096),
                  "pdu_to_nmea")
        return out.raw[:n].decode("latin-1")


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
