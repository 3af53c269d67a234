"""The receive chain's tail on the device, for every channel of a chain step at once, behind
`ais_demod.work_pipelined`: the batched HDLC deframer (aisx_hdlc_batch_*, `hdlc_deframer_bp(11, 64)`,
python/radio.py:64) and, queued behind it on the same stream, the batched `pdu_to_nmea` (aisx_nmea_batch_*,
python/radio.py:73) and the batched ITU-R M.1371 field decoder (aisx_msg_batch_*).  One copy per step brings back the
PDUs, a newline-terminated NMEA stream or a table of decoded messages -- or the table stays on the device as tensors.
Behind the decoder, the vessel table (aisx_track_*): the latest state per MMSI, kept in device memory and merged from
every step's decoded rows, of which only the vessels a step touched are read back."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check

PDU_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class hdlc_deframer_batch:
    """One `hdlc_deframer_bp(length_min, length_max)` per channel, nchan channels of at most max_bits bits per
    call, at most max_pdus PDUs per call (the rest are counted, not kept).  Per channel the results are exactly
    those of the host deframer fed the same bits call by call; records are ordered by channel, then by end_bit
    (the index of the closing bit in the channel's stream, counted from creation / reset).

    Behind the pipelined chain, on a stream `s` of the caller's:

        r = dem.work_pipelined(x_k, x_next)              # step k
        dem.wait(r["step"], stream=s)                    # 1. s waits for step k (the host does not block)
        hd.work(r["bits"], r["produced"], stream=s)      # 2. deframe step k on s, counts read on the device
        ...issue step k + 1, then...
        recs, data = hd.pdus(stream=s)                   # 3. step k's PDUs, read while step k + 1 runs

    The chain's own bit-tail stream is not enough on its own: a step whose front end emitted no whole vector
    writes its zero counts on another of the chain's streams; aisx_chain_wait orders every path.  A step's
    outputs rotate through AISX_CHAIN_DEPTH sets, so work() must be queued before the call that reuses them."""

    def __init__(self, length_min, length_max, nchan, max_bits, max_pdus, repair=None, events=1):
        h = C.c_void_p()
        check(_lib.lib().aisx_hdlc_batch_create(C.byref(h), int(length_min), int(length_max), int(nchan), int(max_bits),
                                                int(max_pdus)), "hdlc_deframer_batch")
        self._h = h
        self.nchan, self.max_bits, self.max_pdus = int(nchan), int(max_bits), int(max_pdus)
        self.length_min, self.length_max = int(length_min), int(length_max)
        self.found = 0  # PDUs the last call found (kept or not)
        self._recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)  # read-back buffers, reused by every call
        self._data = np.zeros(self.max_pdus * (self.length_max - 1) + 1, dtype=np.uint8)
        self._fix = None  # read-back buffer of the repair marks, made on first use
        if repair is not None:
            self.set_repair(repair, events)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_hdlc_batch_destroy(h)
            self._h = None

    def set_repair(self, rules, events=1):
        """Repair by CRC syndrome for every channel (hdlc_deframer_bp.set_repair's rules and events -- by default the
        single wrong bit --, its results): waits for the handle's queued work, applies from the next work() on.  None or
        empty: off."""
        from .framing import REPAIR_SINGLE, repair_rules

        r = repair_rules(rules)
        if events == REPAIR_SINGLE:
            rc = _lib.lib().aisx_hdlc_batch_set_repair(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size)
        else:
            rc = _lib.lib().aisx_hdlc_batch_set_repair_events(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size,
                                                             int(events))
        check(rc, "hdlc_deframer_batch.set_repair")

    def repairs_device(self):
        """device address of the last call's repair marks (int32 [max_pdus], entry k for record k of results_device():
        -1 = delivered as received, else the first flipped bit's index in the frame | event id << 16)"""
        p = C.c_void_p()
        check(_lib.lib().aisx_hdlc_batch_repairs_device(self._h, C.byref(p)), "hdlc_deframer_batch.repairs_device")
        return p.value

    def reset(self):
        check(_lib.lib().aisx_hdlc_batch_reset(self._h), "hdlc_deframer_batch.reset")

    def work(self, bits, produced, stream=None):
        """bits: uint8 device tensor [nchan][>= max_bits], row c holding produced[c] bits (int32 device tensor
        [nchan]).  Queued on `stream` (default: the current one); nothing waits."""
        if bits.dtype != torch.uint8 or not bits.is_cuda or bits.dim() != 2 or bits.shape[0] != self.nchan or bits.stride(1) != 1:
            raise ValueError("hdlc_deframer_batch.work: bits must be a uint8 device tensor [nchan][n] with unit item stride")
        if produced.dtype != torch.int32 or not produced.is_cuda or produced.numel() != self.nchan or not produced.is_contiguous():
            raise ValueError("hdlc_deframer_batch.work: produced must be a contiguous int32 device tensor [nchan]")
        check(_lib.lib().aisx_hdlc_batch_process(self._h, bits.data_ptr(), bits.stride(0), produced.data_ptr(),
                                                 _stream_ptr(stream)), "hdlc_deframer_batch.work")

    def results_device(self):
        """device addresses of the last call's records (aisx_pdu [max_pdus]), bytes and counts (int [3]: found,
        kept, bad-count flag)"""
        p, b, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(_lib.lib().aisx_hdlc_batch_results_device(self._h, C.byref(p), C.byref(b), C.byref(n)),
              "hdlc_deframer_batch.results_device")
        return p.value, b.value, n.value

    def pdus(self, stream=None, as_list=False, overflow_ok=False, with_repairs=False):
        """The last call's PDUs (synchronises `stream`): (records, bytes) with records a PDU_DTYPE array (chan,
        end_bit, len, offset into bytes), or with as_list=True a list of (chan, end_bit, payload bytes).  When
        more than max_pdus were found, OverflowError -- or with overflow_ok=True the first max_pdus (self.found
        tells how many there were).  ValueError when a call since the last read met a count outside
        [0, max_bits] (that channel was not advanced).  with_repairs=True: a third item, the records' repair marks
        (int32 array: -1 = delivered as received, else the first flipped bit's index | event id << 16, which
        ais_amd.repair_mark reads) -- in the list form a fourth field."""
        recs, data = self._recs, self._data
        n = C.c_int(0)
        rc = _lib.lib().aisx_hdlc_batch_read(self._h, recs.ctypes.data_as(C.c_void_p), self.max_pdus,
                                             data.ctypes.data_as(C.c_void_p), data.size, C.byref(n), _stream_ptr(stream))
        self.found = n.value
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "hdlc_deframer_batch.pdus")
        recs = recs[: min(n.value, self.max_pdus)].copy()
        nb = int(recs["offset"][-1] + recs["len"][-1]) if len(recs) else 0
        data = data[:nb].copy()
        if with_repairs:
            if self._fix is None:
                self._fix = np.zeros(self.max_pdus, dtype=np.int32)
            m = C.c_int(0)
            rc = _lib.lib().aisx_hdlc_batch_read_repairs(self._h, self._fix.ctypes.data_as(C.c_void_p), self.max_pdus, C.byref(m),
                                                         _stream_ptr(stream))
            if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
                check(rc, "hdlc_deframer_batch.pdus")
            fix = self._fix[: len(recs)].copy()
            if as_list:
                return [(int(r["chan"]), int(r["end_bit"]), bytes(data[r["offset"]:r["offset"] + r["len"]]), int(f))
                        for r, f in zip(recs, fix)]
            return recs, data, fix
        if as_list:
            return [(int(r["chan"]), int(r["end_bit"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
        return recs, data


class mlse_detector_batch:
    """ais_amd.mlse_detector for nchan channels of at most max_syms symbols per call on the device (aisx_mlse_batch_*):
    per channel exactly the host form's bits, call by call.  Between the pipelined chain and the deframer, on a stream
    `s` of the caller's (the deframer's max_bits = max_syms + 79: a call also decides symbols it carried):

        r = dem.work_pipelined(x_k, x_next, want_syms=True)
        dem.wait(r["step"], stream=s)
        bits, nbits = det.process(r["syms"], r["produced"], stream=s)
        hd.work(bits, nbits, stream=s)

    process() returns the handle's own output tensors, which the next process() or flush() overwrites."""

    def __init__(self, nchan, max_syms, bt=0.4):
        h = C.c_void_p()
        check(_lib.lib().aisx_mlse_batch_create(C.byref(h), float(bt), int(nchan), int(max_syms)), "mlse_detector_batch")
        self._h = h
        self.nchan, self.max_syms, self.bt = int(nchan), int(max_syms), float(bt)
        self.max_bits = self.max_syms + _lib.MLSE_BLOCK + _lib.MLSE_OVERLAP - 1
        self._bits = torch.zeros((self.nchan, self.max_bits), dtype=torch.uint8, device="cuda")
        self._nbits = torch.zeros(self.nchan, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the fills ran on torch's stream; the first call may be queued on any)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_mlse_batch_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_mlse_batch_reset(self._h), "mlse_detector_batch.reset")

    def process(self, syms, nsyms, stream=None):
        """syms: complex64 device tensor [nchan][>= max_syms], row c holding nsyms[c] symbols (int32 device tensor
        [nchan]).  Queued on `stream` (default: the current one); nothing waits.  Returns (bits, nbits): uint8
        [nchan][max_syms + 79] and int32 [nchan], as hdlc_deframer_batch.work takes them."""
        if syms.dtype != torch.complex64 or not syms.is_cuda or syms.dim() != 2 or syms.shape[0] != self.nchan or syms.stride(1) != 1:
            raise ValueError("mlse_detector_batch.process: syms must be a complex64 device tensor [nchan][n] with unit item stride")
        if nsyms.dtype != torch.int32 or not nsyms.is_cuda or nsyms.numel() != self.nchan or not nsyms.is_contiguous():
            raise ValueError("mlse_detector_batch.process: nsyms must be a contiguous int32 device tensor [nchan]")
        check(_lib.lib().aisx_mlse_batch_process(self._h, syms.data_ptr(), syms.stride(0) if self.nchan > 1 else max(syms.stride(0), self.max_syms),
                                                 nsyms.data_ptr(), self._bits.data_ptr(), self._bits.stride(0), self._nbits.data_ptr(),
                                                 _stream_ptr(stream)), "mlse_detector_batch.process")
        return self._bits, self._nbits

    def flush(self, stream=None):
        """the bits of every channel's undecided symbols (at most 79 each); the channels are left as new"""
        check(_lib.lib().aisx_mlse_batch_flush(self._h, self._bits.data_ptr(), self._bits.stride(0), self._nbits.data_ptr(),
                                               _stream_ptr(stream)), "mlse_detector_batch.flush")
        return self._bits, self._nbits

    def status(self, stream=None):
        """0, or AISX_MLSE_ST_BAD_COUNT when a call since the last read met a count outside [0, max_syms] (that channel
        took no symbols); synchronises `stream`"""
        st = C.c_int(0)
        check(_lib.lib().aisx_mlse_batch_status(self._h, C.byref(st), _stream_ptr(stream)), "mlse_detector_batch.status")
        return st.value


def nmea_text_len(length, dlen):
    """what pdu_to_nmea's msg_to_sentence returns for a payload of `length` octets and a designator of dlen bytes,
    in characters (fragments of 56 payload characters, separated by '\n'); 0 for an empty payload"""
    if length <= 0:
        return 0
    P = (8 * length + 5) // 6
    F = (P + 55) // 56
    return F * (18 + (2 if F >= 10 else 1) + dlen) + max(F - 9, 0) + P - 1


def nmea_std_text_len(length, dlen, slen=0, time=-1):
    """nmea_text_len for the standard form (pdu_to_nmea(..., standard=True)): a payload of `length` octets (at most
    378), a designator of dlen bytes, a station of slen bytes and a time (-1: none)"""
    if length <= 0:
        return 0
    P = (8 * length + 5) // 6
    F = (P + 55) // 56
    fields = (2 + slen if slen else 0) + (1 if slen and time >= 0 else 0) + (2 + len(str(int(time))) if time >= 0 else 0)
    return F * ((fields + 5 if fields else 0) + 18 + (F > 1) + dlen) + P + F - 1


def _text_end(offset, length):
    """where a pdu_to_nmea_batch record's text ends in the text buffer: behind its newline, which an empty text lacks
    (integers, numpy or torch values alike)"""
    return offset + length + (length > 0)


class _DevMem:  # device memory a handle owns, for torch.as_tensor: a view keeps the handle alive through `owner`
    def __init__(self, owner, ptr, shape, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3)


class pdu_to_nmea_batch:
    """`pdu_to_nmea(designator)` for every PDU of a device list at once: per record, byte for byte what
    ais_amd.pdu_to_nmea(designator of its channel).msg_to_sentence(payload) returns, followed by one '\n'; the
    records' texts one behind the other (by channel, then end bit, as the deframer orders them), so the text up to
    the last record's end is a ready-to-write NMEA stream.  designators: one str for every channel, or a sequence
    of nchan str (0..16 bytes each); at most max_pdus records per call of at most length_max - 1 payload octets;
    text_cap bytes of text (0: the worst case, nothing can overflow).

    Queued behind the deframer on the caller's stream `s`, the pipelined chain's PDUs become text on the device:

        hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, max_pdus)
        nm = ais_amd.pdu_to_nmea_batch(["A", "B"] * (nchan // 2), nchan, max_pdus, 64)
        r = dem.work_pipelined(x_k, x_next)              # step k
        recs, text = nm.sentences(stream=s)              # step k - 1's text, read while step k runs
        dem.wait(r["step"], stream=s)
        hd.work(r["bits"], r["produced"], stream=s)      # deframe step k on s
        nm.work(hd, stream=s)                            # and armour its PDUs, still on s: nothing waits
        sys.stdout.buffer.write(text)                    # (records: chan, end_bit, offset / len of each text)

    The read of step k - 1 comes before step k's work is queued: both handles' results are replaced by it.

    standard=True: per record the text of ais_amd.pdu_to_nmea(designator, standard=True, station=stations[chan],
    time=...) instead -- exact armouring, tag blocks, message ids (length_max <= 379).  stations: None, one str for
    every channel or nchan str.  set_time(t) sets the c: value of the following calls (a launch parameter: nothing
    waits); the ids run 0..9 round over the multi-sentence records written, call after call, from a counter in device
    memory that next_id() reads and reset() zeroes."""

    def __init__(self, designators, nchan, max_pdus, length_max, text_cap=0, standard=False, stations=None):
        nchan = int(nchan)
        if isinstance(designators, (str, bytes)):
            designators = [designators] * nchan
        designators = [d.encode() if isinstance(d, str) else bytes(d) for d in designators]
        if len(designators) != nchan:
            raise ValueError("pdu_to_nmea_batch: %d designators for %d channels" % (len(designators), nchan))
        arr = (C.c_char_p * nchan)(*designators)
        h = C.c_void_p()
        self.standard = bool(standard)
        if stations is not None and not standard:
            raise ValueError("pdu_to_nmea_batch: stations belong to the standard form (standard=True)")
        if standard:
            if stations is None or isinstance(stations, (str, bytes)):
                stations = [stations or ""] * nchan
            stations = [s.encode() if isinstance(s, str) else bytes(s) for s in stations]
            if len(stations) != nchan:
                raise ValueError("pdu_to_nmea_batch: %d stations for %d channels" % (len(stations), nchan))
            check(_lib.lib().aisx_nmea_batch_create_std(C.byref(h), arr, (C.c_char_p * nchan)(*stations), nchan, int(max_pdus),
                                                        int(length_max), int(text_cap)), "pdu_to_nmea_batch")
            self.stations = [s.decode("latin-1") for s in stations]
        else:
            check(_lib.lib().aisx_nmea_batch_create(C.byref(h), arr, nchan, int(max_pdus), int(length_max), int(text_cap)),
                  "pdu_to_nmea_batch")
        self._h = h
        self.nchan, self.max_pdus, self.length_max = nchan, int(max_pdus), int(length_max)
        self.designators = [d.decode("latin-1") for d in designators]
        self.found = 0  # PDUs the last call's producer found (armoured or not)
        if standard:
            worst = self.max_pdus * (nmea_std_text_len(self.length_max - 1, max(len(d) for d in designators),
                                                       max(len(s) for s in stations), 10 ** 18 - 1) + 1)
        else:
            worst = self.max_pdus * (nmea_text_len(self.length_max - 1, max(len(d) for d in designators)) + 1)
        self.text_cap = worst if int(text_cap) == 0 or int(text_cap) > worst else int(text_cap)  # (the handle's)
        self._recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)  # read-back buffers, reused by every call
        self._text = np.zeros(self.text_cap, dtype=np.uint8)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_nmea_batch_destroy(h)
            self._h = None

    def set_time(self, t):
        """standard form: the c: value of the following calls' tag blocks (-1: none); nothing waits"""
        check(_lib.lib().aisx_nmea_batch_set_time(self._h, int(t)), "pdu_to_nmea_batch.set_time")

    def reset(self):
        """standard form: the id counter back to 0, the time to -1; waits for the handle's queued work"""
        check(_lib.lib().aisx_nmea_batch_reset(self._h), "pdu_to_nmea_batch.reset")

    def next_id(self, stream=None):
        """standard form: the id the next multi-sentence record gets (synchronises `stream`)"""
        n = C.c_int(0)
        check(_lib.lib().aisx_nmea_batch_next_id(self._h, C.byref(n), _stream_ptr(stream)), "pdu_to_nmea_batch.next_id")
        return n.value

    def work(self, deframer, stream=None):
        """Armours the PDUs of the deframer's last call (queued on `stream`, default the current one; nothing
        waits): records count + 1, PDUs found count + 0, so the deframer's overflow shows in sentences()."""
        p, b, n = deframer.results_device()
        self.work_device(p, b, n + 4, n, stream)

    def work_device(self, pdus_ptr, bytes_ptr, npdus_ptr, nfound_ptr=None, stream=None):
        """Device addresses: records in the aisx_pdu layout, their payload bytes, ONE int = records to armour and
        optionally ONE int = PDUs the producer found.  Queued on `stream`; the counts are read on the device."""
        check(_lib.lib().aisx_nmea_batch_process(self._h, C.c_void_p(pdus_ptr), C.c_void_p(bytes_ptr),
                                                 C.c_void_p(npdus_ptr), C.c_void_p(nfound_ptr) if nfound_ptr else None,
                                                 _stream_ptr(stream)), "pdu_to_nmea_batch.work")

    def results_device(self):
        """device addresses of the last call's records (aisx_pdu [max_pdus]: offset / len of each text), text and
        counts (int [3]: found, records written, bad-input flag)"""
        p, t, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(_lib.lib().aisx_nmea_batch_results_device(self._h, C.byref(p), C.byref(t), C.byref(n)),
              "pdu_to_nmea_batch.results_device")
        return p.value, t.value, n.value

    def sentences(self, stream=None, as_list=False, overflow_ok=False):
        """The last call's text (synchronises `stream`): (records, text bytes) with records a PDU_DTYPE array
        (chan, end_bit, offset / len of the text in text bytes), or with as_list=True a list of (chan, end_bit,
        str).  When fewer records were armoured than PDUs found (the deframer's or this handle's overflow),
        OverflowError -- or with overflow_ok=True the ones armoured (self.found tells how many there were).
        ValueError when a call since the last read met a bad count, channel or length (those gave no text)."""
        recs, text = self._recs, self._text
        n, f = C.c_int(0), C.c_int(0)
        rc = _lib.lib().aisx_nmea_batch_read(self._h, recs.ctypes.data_as(C.c_void_p), self.max_pdus,
                                             text.ctypes.data_as(C.c_void_p), text.size, C.byref(n), C.byref(f),
                                             _stream_ptr(stream))
        self.found = f.value
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "pdu_to_nmea_batch.sentences")
        recs = recs[: n.value].copy()
        nt = int(_text_end(recs["offset"][-1], recs["len"][-1])) if len(recs) else 0
        text = text[:nt].tobytes()
        if as_list:
            return [(int(r["chan"]), int(r["end_bit"]), text[r["offset"]:r["offset"] + r["len"]].decode("latin-1"))
                    for r in recs]
        return recs, text


class nmea_to_pdu_batch:
    """ais_amd.nmea_to_pdu on the device (aisx_nmea_parse_batch_*): per call at most max_bytes bytes of text holding at
    most max_lines line ends, at most max_pdus records; records, bytes, times and counts are the host form's with
    pdu_cap = max_pdus, bit for bit and call by call, however the text is cut into calls.  results_device() gives
    (pdus, bytes, count) as hdlc_deframer_batch's does, so every stage behind the deframer takes this handle in its
    place.  Replaying recorded text into the vessel table, chunk by chunk on a stream `s`:

        ps = ais_amd.nmea_to_pdu_batch(["A", "B"], 64, max_bytes, max_lines, max_pdus)
        md = ais_amd.pdu_decode_batch(2, max_pdus, 64)
        vt = ais_amd.vessel_table_batch(capacity, max_pdus)
        for stamp, chunk in enumerate(chunks):           # bytes cut anywhere; the last one ends in a newline
            ps.work(chunk, stream=s)                     # text -> PDUs
            md.work(ps, stream=s)                        # PDUs -> fields
            vt.work(md, stamp, stream=s, deframer=ps)    # fields -> vessels; nothing waits
        vessels = vt.vessels(stream=s)

    A call whose text breaks a bound (more than max_bytes bytes or max_lines line ends) is refused on the device and
    advances nothing; messages() then raises ValueError."""

    def __init__(self, designators, length_max, max_bytes, max_lines, max_pdus, max_line=512, ref_tail=False):
        from .framing import _designators

        d = _designators(designators)
        arr = (C.c_char_p * len(d))(*d)
        h = C.c_void_p()
        check(_lib.lib().aisx_nmea_parse_batch_create(C.byref(h), arr, len(d), int(length_max), int(max_line),
                                                      _lib.AISX_NMEA_PARSE_REF_TAIL if ref_tail else 0, int(max_bytes),
                                                      int(max_lines), int(max_pdus)), "nmea_to_pdu_batch")
        self._h = h
        self.nchan, self.length_max, self.max_line = len(d), int(length_max), int(max_line)
        self.max_bytes, self.max_lines, self.max_pdus = int(max_bytes), int(max_lines), int(max_pdus)
        self.found = 0
        self._text = self._n = self._src = None  # the device copy of host text, made on first use
        self._recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)
        self._data = np.zeros(self.max_pdus * (self.length_max - 1) + 1, dtype=np.uint8)
        self._times = np.zeros(self.max_pdus, dtype=np.int64)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_nmea_parse_batch_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_nmea_parse_batch_reset(self._h), "nmea_to_pdu_batch.reset")

    def work(self, text, nbytes=None, stream=None):
        """text: a contiguous uint8 device tensor, or host bytes (copied into a buffer of the handle's, at most
        max_bytes of them).  nbytes: optionally a one-element int64 device tensor holding the byte count (read when the
        work runs); by default the text's size.  Queued on `stream` (default: the current one); nothing waits.  Host
        bytes go through ONE staging tensor of the handle's: such calls stay on one stream, or are separated by a
        read (a handle's calls are ordered by its state anyway: the carry of one call is the next one's input)."""
        s = stream if stream is not None else torch.cuda.current_stream()
        if isinstance(text, (bytes, bytearray, memoryview)):
            t = bytes(text)
            if len(t) > self.max_bytes:
                raise ValueError("nmea_to_pdu_batch.work: %d bytes of text, max_bytes is %d" % (len(t), self.max_bytes))
            if self._text is None:
                self._text = torch.zeros(self.max_bytes, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
            with torch.cuda.stream(s):
                if t:
                    self._text[: len(t)].copy_(torch.frombuffer(bytearray(t), dtype=torch.uint8))
                n = torch.tensor([len(t)], dtype=torch.int64).to("cuda")
            text, nbytes = self._text, n
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("nmea_to_pdu_batch.work: text must be a contiguous uint8 device tensor or bytes")
        if nbytes is None:
            with torch.cuda.stream(s):
                nbytes = torch.tensor([text.numel()], dtype=torch.int64).to("cuda")
        if nbytes.dtype != torch.int64 or not nbytes.is_cuda or nbytes.numel() != 1:
            raise ValueError("nmea_to_pdu_batch.work: nbytes must be a one-element int64 device tensor")
        self._n, self._src = nbytes, text  # (kept alive until the next call)
        self.work_device(text.data_ptr() if text.numel() else self._dummy().data_ptr(), nbytes.data_ptr(), s)

    def work_nmea(self, armourer, stream=None):
        """Parses the text of a pdu_to_nmea_batch's last call where it is (create the parser with ref_tail=True, and with
        max_bytes >= the armourer's text_cap).  The armourer keeps no text length on the device, so it is worked out
        there from its last written record (_text_end, the rule its own sentences() reads the text by) with a few
        tensor operations on `stream`: nothing waits."""
        s = stream if stream is not None else torch.cuda.current_stream()
        p, t, n = armourer.results_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        raw = torch.as_tensor(_DevMem(armourer, p, (armourer.max_pdus, PDU_DTYPE.itemsize), "|u1"), device=dev)
        cnt = torch.as_tensor(_DevMem(armourer, n, (3,), "<i4"), device=dev)

        def field(row, name):  # one field of a record, by PDU_DTYPE's own offsets
            dt, off = PDU_DTYPE.fields[name][:2]
            return row[off:off + dt.itemsize].view(torch.int64 if dt.itemsize == 8 else torch.int32).to(torch.int64)

        with torch.cuda.stream(s):
            k = cnt[1:2].to(torch.int64)
            last = raw.index_select(0, (k - 1).clamp(min=0))[0]
            nbytes = torch.where(k > 0, _text_end(field(last, "offset"), field(last, "len")), torch.zeros_like(k))
        self._n, self._src = nbytes, armourer
        self.work_device(t, nbytes.data_ptr(), s)

    def _dummy(self):
        if self._text is None:
            self._text = torch.zeros(self.max_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        return self._text

    def work_device(self, text_ptr, nbytes_ptr, stream=None):
        """Device addresses: the text and ONE int64 = its byte count.  Queued on `stream`; the count is read on the
        device, and no byte at or beyond it is."""
        check(_lib.lib().aisx_nmea_parse_batch_process(self._h, C.c_void_p(text_ptr), C.c_void_p(nbytes_ptr), _stream_ptr(stream)),
              "nmea_to_pdu_batch.work")

    def _results(self):
        p, b, n, t = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(_lib.lib().aisx_nmea_parse_batch_results_device(self._h, C.byref(p), C.byref(b), C.byref(n), C.byref(t)),
              "nmea_to_pdu_batch.results_device")
        return p.value, b.value, n.value, t.value

    def results_device(self):
        """device addresses of the last call's records (aisx_pdu [max_pdus]), bytes and counts (int
        [AISX_NMEAP_NCNT], beginning found, kept, bad-input flag), as hdlc_deframer_batch.results_device()"""
        return self._results()[:3]

    def times_device(self):
        """device address of the last call's times (int64 [max_pdus], entry k for record k)"""
        return self._results()[3]

    def messages(self, stream=None, overflow_ok=False):
        """The last call's results on the host (synchronises `stream`): (records, bytes, times, counts) as
        nmea_to_pdu.work gives them.  OverflowError when more than max_pdus messages were found -- or with
        overflow_ok=True the first max_pdus (self.found tells how many there were); ValueError when a call since the
        last read was refused."""
        cnt = np.zeros(_lib.AISX_NMEAP_NCNT, dtype=np.int32)
        rc = _lib.lib().aisx_nmea_parse_batch_read(self._h, self._recs.ctypes.data_as(C.c_void_p), self.max_pdus,
                                                   self._data.ctypes.data_as(C.c_void_p), self._data.size,
                                                   self._times.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                                   _stream_ptr(stream))
        self.found = int(cnt[0])
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "nmea_to_pdu_batch.messages")
        k = int(cnt[1])
        recs = self._recs[:k].copy()
        nb = int(recs["offset"][-1] + recs["len"][-1]) if k else 0
        return recs, self._data[:nb].copy(), self._times[:k].copy(), {n: int(v) for n, v in zip(_lib.AISX_NMEAP_NAMES, cnt)}


class pdu_decode_batch:
    """The ITU-R M.1371 fields of every PDU of a device list at once (aisx_msg_batch_*): row i is exactly
    ais_amd.msg_decode(payload of record i), as a struct-of-arrays table in device memory -- int32
    cols[len(MSG_COLUMNS)][max_pdus] and uint8 strs[max_pdus][48] -- so that a column is a torch tensor.  At most
    max_pdus records per call on nchan channels, of at most length_max - 1 payload octets.

    Queued behind the deframer on the caller's stream `s` (beside or instead of pdu_to_nmea_batch):

        md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
        hd.work(r["bits"], r["produced"], stream=s)      # deframe step k on s
        md.work(hd, stream=s)                            # and decode its PDUs, still on s: nothing waits
        c = md.columns(stream=s)                         # device views: c["MMSI"], c["LON"], ... c["strs"]
        near = c["MMSI"][(c["LAT"] > lat0) & (c["LAT"] < lat1)]

    Values are the transmitted integers; MSG_NA (-2**31) marks a column the message does not carry."""

    def __init__(self, nchan, max_pdus, length_max):
        h = C.c_void_p()
        check(_lib.lib().aisx_msg_batch_create(C.byref(h), int(nchan), int(max_pdus), int(length_max)), "pdu_decode_batch")
        self._h = h
        self.nchan, self.max_pdus, self.length_max = int(nchan), int(max_pdus), int(length_max)
        self.found = 0  # PDUs the last call's producer found (decoded or not)
        self._cols = self._strs = None  # read-back buffers, made on first use

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_msg_batch_destroy(h)
            self._h = None

    def work(self, deframer, stream=None):
        """Decodes the PDUs of the deframer's last call (queued on `stream`, default the current one; nothing
        waits): records count + 1, PDUs found count + 0, so the deframer's overflow shows in messages()."""
        p, b, n = deframer.results_device()
        self.work_device(p, b, n + 4, n, stream)

    def work_device(self, pdus_ptr, bytes_ptr, npdus_ptr, nfound_ptr=None, stream=None):
        """Device addresses: records in the aisx_pdu layout, their payload bytes, ONE int = records to decode and
        optionally ONE int = PDUs the producer found.  Queued on `stream`; the counts are read on the device."""
        check(_lib.lib().aisx_msg_batch_process(self._h, C.c_void_p(pdus_ptr), C.c_void_p(bytes_ptr), C.c_void_p(npdus_ptr),
                                                C.c_void_p(nfound_ptr) if nfound_ptr else None, _stream_ptr(stream)),
              "pdu_decode_batch.work")

    def results_device(self):
        """device addresses of the last call's columns (int32 [ncol][col_stride]), the column stride in items, the
        strings (char [max_pdus][48]) and the counts (int [3]: found, rows written, bad-input flag)"""
        c, s, n, stride = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_long()
        check(_lib.lib().aisx_msg_batch_results_device(self._h, C.byref(c), C.byref(stride), C.byref(s), C.byref(n)),
              "pdu_decode_batch.results_device")
        return c.value, stride.value, s.value, n.value

    def _views(self):
        from .framing import MSG_COLUMNS

        c, stride, s, n = self.results_device()
        dev = torch.device("cuda", torch.cuda.current_device())

        class _Mem:  # (the handle owns the memory: a view keeps the handle alive through `owner`)
            def __init__(self, owner, ptr, shape, typestr):
                self.owner = owner
                self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3)

        cols = torch.as_tensor(_Mem(self, c, (len(MSG_COLUMNS), stride), "<i4"), device=dev)
        strs = torch.as_tensor(_Mem(self, s, (self.max_pdus, _lib.AISX_MSG_STR), "|u1"), device=dev)
        cnt = torch.as_tensor(_Mem(self, n, (3,), "<i4"), device=dev)
        return cols, strs, cnt

    def columns(self, stream=None):
        """The last call's table where it is: {column name: int32 device tensor [kept]} for every name of
        MSG_COLUMNS, and "strs": uint8 device tensor [kept, 48] -- views of the handle's buffers, which the next
        work() overwrites.  Waits on `stream` only to learn the row count; self.found = PDUs the producer found."""
        from .framing import MSG_COLUMNS

        cols, strs, cnt = self._views()
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            found, kept, _ = cnt.cpu().tolist()
        self.found = found
        kept = max(0, min(kept, self.max_pdus))
        out = {name: cols[k, :kept] for k, name in enumerate(MSG_COLUMNS)}
        out["strs"] = strs[:kept]
        return out

    def messages(self, stream=None, overflow_ok=False):
        """The last call's table on the host (synchronises `stream`): a MSG_DTYPE structured array, one int32 field
        per column (lower-case names) and callsign / name / destination as S7 / S20 / S20.  When fewer rows were
        written than PDUs found (the deframer's overflow), OverflowError -- or with overflow_ok=True the rows
        written (self.found tells how many there were).  ValueError when a call since the last read met a bad
        count, channel or length (such a record's row has FLAGS = 4 and no fields)."""
        from .framing import MSG_COLUMNS, msg_table

        if self._cols is None:
            self._cols = np.zeros((len(MSG_COLUMNS), self.max_pdus), dtype=np.int32)
            self._strs = np.zeros((self.max_pdus, _lib.AISX_MSG_STR), dtype=np.uint8)
        n, f = C.c_int(0), C.c_int(0)
        rc = _lib.lib().aisx_msg_batch_read(self._h, self._cols.ctypes.data_as(C.c_void_p), self.max_pdus,
                                            self._strs.ctypes.data_as(C.c_void_p), self.max_pdus, C.byref(n), C.byref(f),
                                            _stream_ptr(stream))
        self.found = f.value
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "pdu_decode_batch.messages")
        return msg_table(self._cols, self._strs, n.value)


# the columns of a vessel, in the order of include/aisx.h's AISX_MSG_COL_* and AISX_TRK_COL_*, and the counts of AISX_TRK_CNT_*
def _track_names():
    from .framing import MSG_COLUMNS

    return tuple(MSG_COLUMNS) + ("COUNT", "STAMP", "POS_STAMP", "CHAN")


TRACK_COLUMNS = _track_names()
TRACK_COUNTS = ("vessels", "merged", "skipped", "dropped", "changed", "removed", "full", "bad_input")
# one vessel on the host: an int32 per column (lower-case names) and the three strings; a changed vessel also has its index
TRACK_DTYPE = np.dtype([(c.lower(), "<i4") for c in TRACK_COLUMNS] + [("callsign", "S7"), ("name", "S20"), ("destination", "S20")])
TRACK_CHANGED_DTYPE = np.dtype([("vessel", "<i4")] + TRACK_DTYPE.descr)


def _track_table(cols, strs, n, idx=None):
    """int32 [ncol][>= n] and uint8 [>= n][48] on the host -> a TRACK_DTYPE array of n vessels (TRACK_CHANGED_DTYPE
    with their indices when idx is given)"""
    out = np.zeros(n, dtype=TRACK_DTYPE if idx is None else TRACK_CHANGED_DTYPE)
    if idx is not None:
        out["vessel"] = idx[:n]
    for k, c in enumerate(TRACK_COLUMNS):
        out[c.lower()] = cols[k, :n]
    s = np.ascontiguousarray(strs[:n])
    out["callsign"] = s[:, 0:7].copy().view("S7").ravel()
    out["name"] = s[:, 8:28].copy().view("S20").ravel()
    out["destination"] = s[:, 28:48].copy().view("S20").ravel()
    return out


def _rows_of(messages):
    """a MSG_DTYPE array (pop_messages' / messages') -> (int32 cols [ncol][n], uint8 strs [n][48])"""
    from .framing import MSG_COLUMNS

    m = np.asarray(messages)
    cols = np.ascontiguousarray(np.stack([m[c.lower()] for c in MSG_COLUMNS]).astype(np.int32)) if len(m) else \
        np.zeros((len(MSG_COLUMNS), 0), dtype=np.int32)
    strs = np.zeros((len(m), _lib.AISX_MSG_STR), dtype=np.uint8)
    for name, lo, w in (("callsign", 0, 7), ("name", 8, 20), ("destination", 28, 20)):
        if len(m):
            strs[:, lo:lo + w] = np.frombuffer(m[name].astype("S%d" % w).tobytes(), dtype=np.uint8).reshape(len(m), w)
    return cols, strs


class vessel_table:
    """The vessel table on the host (aisx_track_*, plain C++: the specification of vessel_table_batch): the latest
    state per MMSI, at most `capacity` vessels, vessel v the v-th distinct MMSI accepted.  update() merges the rows of
    a decoded table in row order -- a column that is not MSG_NA and a string slot that is carried replace the vessel's,
    so type 5 / 24 static data and type 1-3 / 18 / 19 positions meet in one row; expire() forgets the vessels whose
    last update is older than a stamp.  Values are kept as transmitted (the protocol's own "not available" codes are
    values like any other)."""

    def __init__(self, capacity):
        h = C.c_void_p()
        check(_lib.lib(device=False).aisx_track_create(C.byref(h), int(capacity)), "vessel_table")
        self._h = h
        self.capacity = int(capacity)
        self.counts = dict.fromkeys(TRACK_COUNTS, 0)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib(device=False).aisx_track_destroy(h)
            self._h = None

    def _set_counts(self, cnt):
        self.counts = {k: int(v) for k, v in zip(TRACK_COUNTS, cnt)}
        return self.counts

    def update(self, cols, strs, stamp, recs=None):
        """cols: int32 [len(MSG_COLUMNS)][n], strs: uint8 [n][48] (or cols a MSG_DTYPE array and strs None); recs: the
        rows' PDU_DTYPE records, for CHAN.  Returns the counts of this call as a dict of TRACK_COUNTS."""
        if strs is None:
            cols, strs = _rows_of(cols)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        strs = np.ascontiguousarray(strs, dtype=np.uint8)
        n = cols.shape[1]
        if strs.shape != (n, _lib.AISX_MSG_STR) or (recs is not None and len(recs) < n):
            raise ValueError("vessel_table.update: need cols [ncol][n], strs [n][48] and, if any, n records")
        r = np.ascontiguousarray(recs, dtype=PDU_DTYPE) if recs is not None else None
        cnt = np.zeros(len(TRACK_COUNTS), dtype=np.int32)
        check(_lib.lib(device=False).aisx_track_update(self._h, cols.ctypes.data_as(C.c_void_p), n,
                                                       strs.ctypes.data_as(C.c_void_p),
                                                       r.ctypes.data_as(C.c_void_p) if r is not None else None, n, int(stamp),
                                                       cnt.ctypes.data_as(C.c_void_p)), "vessel_table.update")
        return self._set_counts(cnt)

    def expire(self, min_stamp):
        """forgets every vessel whose STAMP is below min_stamp; returns how many"""
        cnt = np.zeros(len(TRACK_COUNTS), dtype=np.int32)
        check(_lib.lib(device=False).aisx_track_expire(self._h, int(min_stamp), cnt.ctypes.data_as(C.c_void_p)), "vessel_table.expire")
        return self._set_counts(cnt)["removed"]

    def arrays(self):
        """(cols int32 [len(TRACK_COLUMNS)][nvessels], strs uint8 [nvessels][48], changed int32 [nchanged]): copies"""
        c, s, i = C.c_void_p(), C.c_void_p(), C.c_void_p()
        stride, nv, nc = C.c_long(), C.c_int(), C.c_int()
        L = _lib.lib(device=False)
        check(L.aisx_track_data(self._h, C.byref(c), C.byref(stride), C.byref(s), C.byref(nv)), "vessel_table")
        check(L.aisx_track_changed(self._h, C.byref(i), C.byref(nc)), "vessel_table")
        ncol = len(TRACK_COLUMNS)
        cols = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_int32)), shape=(ncol, stride.value))[:, : nv.value].copy()
        strs = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_uint8)), shape=(stride.value, _lib.AISX_MSG_STR))[: nv.value].copy()
        chg = np.ctypeslib.as_array(C.cast(i, C.POINTER(C.c_int32)), shape=(nc.value,)).copy() if nc.value else np.zeros(0, np.int32)
        return cols, strs, chg

    def vessels(self):
        """the table as a TRACK_DTYPE array, one row per vessel"""
        cols, strs, _ = self.arrays()
        return _track_table(cols, strs, cols.shape[1])

    def changed(self):
        """the vessels the last update merged a row into, ordered by the first row that touched each: a
        TRACK_CHANGED_DTYPE array (field "vessel" = the index)"""
        cols, strs, chg = self.arrays()
        return _track_table(cols[:, chg], strs[chg], len(chg), chg)


class vessel_table_batch:
    """The vessel table in device memory (aisx_track_batch_*): the same table as vessel_table, bit for bit, updated from
    the decoder's rows by kernels queued behind it -- at most max_rows rows per call -- so that the per-PDU table never
    has to leave the device.  Only what a step changed is read back:

        md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
        vt = ais_amd.vessel_table_batch(1 << 20, max_pdus)
        hd.work(r["bits"], r["produced"], stream=s)      # deframe step k on s
        md.work(hd, stream=s)                            # decode its PDUs
        vt.work(md, stamp=k, stream=s, deframer=hd)      # and merge them, still on s: nothing waits
        for v in vt.changed(stream=s):                   # the vessels step k touched (v["vessel"] = the index)
            ...
        vt.expire(k - 600, stream=s)                     # now and then: forget who fell silent

    results_device() gives the table where it is, as torch views."""

    def __init__(self, capacity, max_rows):
        h = C.c_void_p()
        check(_lib.lib().aisx_track_batch_create(C.byref(h), int(capacity), int(max_rows)), "vessel_table_batch")
        self._h = h
        self.capacity, self.max_rows = int(capacity), int(max_rows)
        self.counts = dict.fromkeys(TRACK_COUNTS, 0)
        self._cols = self._strs = self._idx = None  # read-back buffers of changed(), made on first use

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_track_batch_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_track_batch_reset(self._h), "vessel_table_batch.reset")

    def work(self, decoder, stamp, stream=None, deframer=None):
        """Merges the rows of the decoder's last call (queued on `stream`, default the current one; nothing waits),
        count + 1 of them; deframer: the one whose records the decoder read, for the CHAN column."""
        c, stride, s, n = decoder.results_device()
        self.work_device(c, stride, s, n + 4, stamp, deframer.results_device()[0] if deframer is not None else None, stream)

    def work_device(self, cols_ptr, col_stride, strs_ptr, nrows_ptr, stamp, pdus_ptr=None, stream=None):
        """Device addresses: int32 cols [len(MSG_COLUMNS)][col_stride], char strs [rows][48], ONE int = rows to merge
        and optionally the rows' aisx_pdu records.  Queued on `stream`; the count is read on the device."""
        check(_lib.lib().aisx_track_batch_process(self._h, C.c_void_p(cols_ptr), int(col_stride), C.c_void_p(strs_ptr),
                                                  C.c_void_p(pdus_ptr) if pdus_ptr else None, C.c_void_p(nrows_ptr), int(stamp),
                                                  _stream_ptr(stream)), "vessel_table_batch.work")

    def expire(self, min_stamp, stream=None):
        """queues the removal of every vessel whose STAMP is below min_stamp (counts()["removed"] tells how many)"""
        check(_lib.lib().aisx_track_batch_expire(self._h, int(min_stamp), _stream_ptr(stream)), "vessel_table_batch.expire")

    def get_counts(self, stream=None):
        """the counts as a dict of TRACK_COUNTS (synchronises `stream`)"""
        cnt = np.zeros(len(TRACK_COUNTS), dtype=np.int32)
        check(_lib.lib().aisx_track_batch_counts(self._h, cnt.ctypes.data_as(C.c_void_p), _stream_ptr(stream)),
              "vessel_table_batch.counts")
        self.counts = {k: int(v) for k, v in zip(TRACK_COUNTS, cnt)}
        return self.counts

    def results_device(self):
        """torch views of the table where it is: {"cols": int32 [len(TRACK_COLUMNS)][capacity], "strs": uint8
        [capacity][48], "changed": int32 [max_rows], "count": int32 [len(TRACK_COUNTS)]}.  An expire() moves the table
        to the handle's other buffer: ask again after one."""
        c, s, i, n, stride = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_long()
        check(_lib.lib().aisx_track_batch_results_device(self._h, C.byref(c), C.byref(stride), C.byref(s), C.byref(i), C.byref(n)),
              "vessel_table_batch.results_device")
        dev = torch.device("cuda", torch.cuda.current_device())

        class _Mem:  # (the handle owns the memory: a view keeps the handle alive through `owner`)
            def __init__(self, owner, ptr, shape, typestr):
                self.owner = owner
                self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3)

        return {"cols": torch.as_tensor(_Mem(self, c.value, (len(TRACK_COLUMNS), stride.value), "<i4"), device=dev),
                "strs": torch.as_tensor(_Mem(self, s.value, (self.capacity, _lib.AISX_MSG_STR), "|u1"), device=dev),
                "changed": torch.as_tensor(_Mem(self, i.value, (self.max_rows,), "<i4"), device=dev),
                "count": torch.as_tensor(_Mem(self, n.value, (len(TRACK_COUNTS),), "<i4"), device=dev)}

    def arrays(self, first=0, n=None, stream=None):
        """(cols int32 [len(TRACK_COLUMNS)][k], strs uint8 [k][48]) of vessels [first, first + n) that exist
        (synchronises `stream`); self.nvessels = vessels in the table"""
        n = self.capacity if n is None else int(n)
        cols = np.zeros((len(TRACK_COLUMNS), max(n, 1)), dtype=np.int32)
        strs = np.zeros((max(n, 1), _lib.AISX_MSG_STR), dtype=np.uint8)
        nv = C.c_int(0)
        check(_lib.lib().aisx_track_batch_read(self._h, int(first), n, cols.ctypes.data_as(C.c_void_p), cols.shape[1],
                                               strs.ctypes.data_as(C.c_void_p), C.byref(nv), _stream_ptr(stream)),
              "vessel_table_batch.vessels")
        self.nvessels = nv.value
        k = max(0, min(n, nv.value - int(first)))
        return cols[:, :k], strs[:k]

    def vessels(self, first=0, n=None, stream=None):
        """vessels [first, first + n) as a TRACK_DTYPE array (synchronises `stream`).  ValueError when a call since the
        last read met a row count outside [0, max_rows] (it merged nothing)."""
        cols, strs = self.arrays(first, n, stream)
        return _track_table(cols, strs, cols.shape[1])

    def changed_arrays(self, cap=None, stream=None):
        """(idx int32 [k], cols int32 [len(TRACK_COLUMNS)][k], strs uint8 [k][48]) of the last update's changed list,
        gathered on the device (synchronises `stream`).  OverflowError when more than `cap` vessels changed
        (self.nchanged tells how many)."""
        if self._cols is None:
            self._idx = np.zeros(self.max_rows, dtype=np.int32)
            self._cols = np.zeros((len(TRACK_COLUMNS), self.max_rows), dtype=np.int32)
            self._strs = np.zeros((self.max_rows, _lib.AISX_MSG_STR), dtype=np.uint8)
        cap = self.max_rows if cap is None else min(int(cap), self.max_rows)
        nc = C.c_int(0)
        rc = _lib.lib().aisx_track_batch_read_changed(self._h, self._idx.ctypes.data_as(C.c_void_p), self._cols.ctypes.data_as(C.c_void_p),
                                                      self.max_rows, self._strs.ctypes.data_as(C.c_void_p), cap, C.byref(nc),
                                                      _stream_ptr(stream))
        self.nchanged = nc.value
        check(rc, "vessel_table_batch.changed")
        k = nc.value
        return self._idx[:k].copy(), self._cols[:, :k].copy(), self._strs[:k].copy()

    def changed(self, cap=None, stream=None):
        """the vessels the last update merged a row into, ordered by the first row that touched each: a
        TRACK_CHANGED_DTYPE array (field "vessel" = the index)"""
        idx, cols, strs = self.changed_arrays(cap, stream)
        return _track_table(cols, strs, len(idx), idx)


ENCODE_COUNTS = ("found", "records", "bad_input", "encoded", "refused")


class pdu_encode_batch:
    """ais_amd.msg_encode for every row of a table in device memory at once (aisx_msg_enc_batch_*): the inverse of
    pdu_decode_batch.  Record i of the list it makes is exactly msg_encode(row i) -- or of row idx[i] with an index
    list --, at most max_rows records per call from a table of table_rows rows (the decoder's max_pdus, the vessel
    table's capacity) on nchan channels.  The list has the layout every stage behind the deframer takes: record i has
    end_bit = i, offset = 56 * i and the length msg_encode gives, 0 for a refused row (status() tells why), for which
    the armouring stage writes nothing.  results_device() gives (pdus, bytes, count) as the deframer's does.

    A snapshot of the vessel table as !AIVDM text, without the table leaving the device:

        vt = ais_amd.vessel_table_batch(capacity, max_pdus)
        enc = ais_amd.pdu_encode_batch(nchan, capacity, capacity)
        nm = ais_amd.pdu_to_nmea_batch("A", nchan, capacity, 64, standard=True)
        enc.work(vt, as_type=1, stream=s)                # every vessel as a position report (as_type=5: static data)
        nm.work_device(*enc.results_device(), stream=s)  # pdus, bytes, count: all records, none found beyond them
        recs, text = nm.sentences(stream=s)

    and what a step changed, on their channels: enc.work(vt, as_type=1, changed_only=True, chan="table", stream=s).
    A vessel that lacks a column gets the protocol's "not available" value; one whose columns do not fit the type
    (a class-B vessel's missing NAV_STATUS is fine, a 30-bit IMO is not asked for by type 1) is refused, not truncated."""

    def __init__(self, nchan, max_rows, table_rows):
        h = C.c_void_p()
        check(_lib.lib().aisx_msg_enc_batch_create(C.byref(h), int(nchan), int(max_rows), int(table_rows)), "pdu_encode_batch")
        self._h = h
        self.nchan, self.max_rows, self.table_rows = int(nchan), int(max_rows), int(table_rows)
        self.max_pdus = self.max_rows  # (what the stages behind call a list's capacity)
        self.counts = dict.fromkeys(ENCODE_COUNTS, 0)
        self._keep = None  # what the last call reads, kept alive until the next
        self._recs = self._data = self._st = None  # read-back buffers, made on first use

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_msg_enc_batch_destroy(h)
            self._h = None

    def work(self, table, as_type=0, as_part=-1, changed_only=False, chan=None, stream=None):
        """Encodes the rows of `table` (queued on `stream`, default the current one; nothing waits):
          - a pdu_decode_batch: the rows of its last call;
          - a vessel_table_batch: every vessel, or with changed_only=True the last update's changed list, in its
            order; chan="table" takes each vessel's CHAN column as its channel;
          - device tensors (cols int32 [ncol][col_stride], strs uint8 [rows][48] or None, nrows int32 [1][, idx int32
            [rows]]).
        chan: None (channel 0) or an int32 device tensor, indexed by record without an index list and by table row with
        one."""
        idx = None
        if isinstance(table, pdu_decode_batch):
            c, stride, s, n = table.results_device()
            n += 4
        elif isinstance(table, vessel_table_batch):
            r = table.results_device()
            c, stride, s = r["cols"].data_ptr(), r["cols"].shape[1], r["strs"].data_ptr()
            n = r["count"].data_ptr() + 4 * TRACK_COUNTS.index("changed" if changed_only else "vessels")
            idx = r["changed"].data_ptr() if changed_only else None
            if isinstance(chan, str):
                if chan != "table":
                    raise ValueError("pdu_encode_batch.work: chan is None, \"table\" or an int32 device tensor")
                chan = r["cols"][TRACK_COLUMNS.index("CHAN")]
        else:
            cols, strs, nrows = table[:3]
            it = table[3] if len(table) > 3 else None
            for name, t, dt in (("cols", cols, torch.int32), ("strs", strs, torch.uint8), ("nrows", nrows, torch.int32), ("idx", it, torch.int32)):
                if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
                    raise ValueError("pdu_encode_batch.work: %s must be a contiguous %s device tensor" % (name, dt))
            if cols.dim() != 2 or cols.shape[0] < len(TRACK_COLUMNS) - 4 or nrows.numel() != 1:
                raise ValueError("pdu_encode_batch.work: need cols [ncol][col_stride] and ONE row count")
            c, stride, s, n = cols.data_ptr(), cols.shape[1], strs.data_ptr() if strs is not None else None, nrows.data_ptr()
            idx = it.data_ptr() if it is not None else None
        if changed_only and not isinstance(table, vessel_table_batch):
            raise ValueError("pdu_encode_batch.work: changed_only belongs to a vessel_table_batch")
        if chan is not None and (isinstance(chan, str) or chan.dtype != torch.int32 or not chan.is_cuda or not chan.is_contiguous()):
            raise ValueError("pdu_encode_batch.work: chan is None, \"table\" (of a vessel_table_batch) or an int32 device tensor")
        self._keep = (table, chan)
        self.work_device(c, stride, s, n, idx, chan.data_ptr() if chan is not None else None, as_type, as_part, stream)

    def work_device(self, cols_ptr, col_stride, strs_ptr, nrows_ptr, idx_ptr=None, chan_ptr=None, as_type=0, as_part=-1, stream=None):
        """Device addresses: int32 cols [ncol][col_stride] (col_stride >= table_rows), char strs [table_rows][48]
        (4-byte aligned, or None), ONE int = records to make, optionally int32 idx [records] and int32 chan.  Queued
        on `stream`; the count is read on the device."""
        check(_lib.lib().aisx_msg_enc_batch_process(self._h, C.c_void_p(cols_ptr), int(col_stride),
                                                    C.c_void_p(strs_ptr) if strs_ptr else None,
                                                    C.c_void_p(idx_ptr) if idx_ptr else None, C.c_void_p(nrows_ptr),
                                                    C.c_void_p(chan_ptr) if chan_ptr else None, int(as_type), int(as_part),
                                                    _stream_ptr(stream)), "pdu_encode_batch.work")

    def _results(self):
        v = [C.c_void_p() for _ in range(4)]
        check(_lib.lib().aisx_msg_enc_batch_results_device(self._h, *[C.byref(x) for x in v]), "pdu_encode_batch.results_device")
        return tuple(x.value for x in v)

    def results_device(self):
        """device addresses of the last call's records (aisx_pdu [max_rows]), bytes and counts (int [5]: records twice,
        the bad-count flag, rows encoded, rows refused), as hdlc_deframer_batch.results_device(); as the arguments of a
        work_device() behind, (pdus, bytes, count) say: count + 0 records, none found beyond them"""
        return self._results()[:3]

    def status_device(self):
        """device address of the last call's status (int32 [max_rows], entry i for record i)"""
        return self._results()[3]

    def _read(self, stream):
        if self._recs is None:
            self._recs = np.zeros(self.max_rows, dtype=PDU_DTYPE)
            self._data = np.zeros(self.max_rows * _lib.AISX_MSG_ENC_PITCH, dtype=np.uint8)
            self._st = np.zeros(self.max_rows, dtype=np.int32)
        n = C.c_int(0)
        cnt = np.zeros(len(ENCODE_COUNTS), dtype=np.int32)
        rc = _lib.lib().aisx_msg_enc_batch_read(self._h, self._recs.ctypes.data_as(C.c_void_p), self._st.ctypes.data_as(C.c_void_p),
                                                self.max_rows, self._data.ctypes.data_as(C.c_void_p), self._data.size, C.byref(n),
                                                cnt.ctypes.data_as(C.c_void_p), _stream_ptr(stream))
        self.counts = {k: int(v) for k, v in zip(ENCODE_COUNTS, cnt)}
        check(rc, "pdu_encode_batch")
        k = n.value
        return self._recs[:k].copy(), self._data[: k * _lib.AISX_MSG_ENC_PITCH].copy(), self._st[:k].copy()

    def pdus(self, stream=None, as_list=False):
        """The last call's list on the host (synchronises `stream`): (records, bytes) with records a PDU_DTYPE array
        (chan, end_bit = i, len, offset = 56 i into bytes), or with as_list=True a list of (chan, end_bit, payload
        bytes).  self.counts has the call's counts.  ValueError when a call since the last read met a row count outside
        [0, max_rows] (it made no records)."""
        recs, data, _ = self._read(stream)
        if as_list:
            return [(int(r["chan"]), int(r["end_bit"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
        return recs, data

    def status(self, stream=None):
        """the last call's status per record (synchronises `stream`): an int32 array, 0 or a sum of MSG_ENC_*"""
        return self._read(stream)[2]


class pdu_dedup_batch:
    """ais_amd.pdu_dedup in device memory (aisx_dedup_batch_*): the same kept records, first, copies, marks and counts,
    bit for bit, for at most max_pdus records per call, by kernels queued between a producer of a PDU list (the deframer,
    nmea_to_pdu_batch) and the stages behind it.  results_device() gives (pdus, bytes, count) as the deframer's does, so
    those stages take this handle in the deframer's place:

        dd = ais_amd.pdu_dedup_batch(window=2, max_pdus=max_pdus, length_max=64)
        hd.work(r["bits"], r["produced"], stream=s)      # deframe step k on s
        dd.work(hd, stamp=k, stream=s)                   # keep one copy of every payload
        nm.work(dd, stream=s)                            # text of the kept records only
        md.work(dd, stream=s)
        vt.work(md, k, stream=s, deframer=dd)            # COUNT counts transmissions, not receptions

    The handle holds window + 1 sets of remembered keys of 2 * max_pdus slots or more (8 bytes each)."""

    def __init__(self, window, max_pdus, length_max=64):
        h = C.c_void_p()
        check(_lib.lib().aisx_dedup_batch_create(C.byref(h), int(window), int(max_pdus), int(length_max)), "pdu_dedup_batch")
        self._h = h
        self.window, self.max_pdus, self.length_max = int(window), int(max_pdus), int(length_max)
        self.found = 0  # the last read's d_count[0]: records kept + what the producer found beyond what it handed over
        self.counts = None
        self._keep = None  # what the last call reads, kept alive until the next

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_dedup_batch_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_dedup_batch_reset(self._h), "pdu_dedup_batch.reset")

    def work(self, producer, stamp, stream=None, marks=None):
        """Takes the PDUs of the producer's last call -- anything with the deframer's results_device() -- queued on
        `stream` (default the current one; nothing waits): records count + 1, PDUs found count + 0.  marks: an int32
        device tensor with one entry per record, or a device address (hdlc_deframer_batch.repairs_device()), carried
        along to the kept records.  IndexError when stamp is not above the previous call's (nothing is queued)."""
        p, b, n = producer.results_device()
        self._keep = (producer, marks)
        if marks is not None and not isinstance(marks, int):
            if marks.dtype != torch.int32 or not marks.is_cuda or not marks.is_contiguous():
                raise ValueError("pdu_dedup_batch.work: marks must be a contiguous int32 device tensor or a device address")
            marks = marks.data_ptr()
        self.work_device(p, b, n + 4, n, stamp, marks, stream)

    def work_device(self, pdus_ptr, bytes_ptr, npdus_ptr, nfound_ptr, stamp, marks_ptr=None, stream=None):
        """Device addresses: records in the aisx_pdu layout, their payload bytes, ONE int = records, optionally ONE int =
        PDUs the producer found and optionally int32 marks.  Queued on `stream`; the counts are read on the device."""
        check(_lib.lib().aisx_dedup_batch_process(self._h, C.c_void_p(pdus_ptr), C.c_void_p(bytes_ptr), C.c_void_p(npdus_ptr),
                                                  C.c_void_p(nfound_ptr) if nfound_ptr else None,
                                                  C.c_void_p(marks_ptr) if marks_ptr else None, int(stamp), _stream_ptr(stream)),
              "pdu_dedup_batch.work")

    def _results(self):
        v = [C.c_void_p() for _ in range(6)]
        check(_lib.lib().aisx_dedup_batch_results_device(self._h, *[C.byref(x) for x in v]), "pdu_dedup_batch.results_device")
        return tuple(x.value for x in v)

    def results_device(self):
        """device addresses of the last call's kept records (aisx_pdu [max_pdus]), the producer's bytes and the counts
        (int [8]: found, kept, bad-count flag, then DEDUP_COUNTS), as hdlc_deframer_batch.results_device()"""
        return self._results()[:3]

    def extras_device(self):
        """device addresses of first, copies and the kept records' marks (int32 [max_pdus] each)"""
        return self._results()[3:]

    def _read(self, stream, overflow_ok):
        from .framing import DEDUP_COUNTS

        recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)
        copies, marks, first = (np.zeros(self.max_pdus, dtype=np.int32) for _ in range(3))
        cnt = np.zeros(len(DEDUP_COUNTS), dtype=np.int32)
        f = C.c_int(0)
        rc = _lib.lib().aisx_dedup_batch_read(self._h, recs.ctypes.data_as(C.c_void_p), copies.ctypes.data_as(C.c_void_p),
                                              marks.ctypes.data_as(C.c_void_p), self.max_pdus, first.ctypes.data_as(C.c_void_p),
                                              self.max_pdus, cnt.ctypes.data_as(C.c_void_p), C.byref(f), _stream_ptr(stream))
        self.found = f.value
        self.counts = {k: int(v) for k, v in zip(DEDUP_COUNTS, cnt)}
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "pdu_dedup_batch")
        k, n = self.counts["kept"], self.counts["in"]
        return recs[:k], first[:n], copies[:k], marks[:k]

    def pdus(self, stream=None, overflow_ok=False):
        """the last call's kept records, a PDU_DTYPE array whose offsets point into the producer's bytes (synchronises
        `stream`).  OverflowError when the producer found more than it handed over (overflow_ok=True: the records all the
        same), ValueError when a call since the last read met a record count outside [0, max_pdus]."""
        return self._read(stream, overflow_ok)[0]

    def first(self, stream=None, overflow_ok=False):
        """first[i] of every record of the last call, as pdu_dedup gives it (synchronises `stream`)"""
        return self._read(stream, overflow_ok)[1]

    def copies(self, stream=None, overflow_ok=False):
        """copies[j] of every kept record of the last call (synchronises `stream`)"""
        return self._read(stream, overflow_ok)[2]

    def marks(self, stream=None, overflow_ok=False):
        """the kept records' marks of the last call, where it was given marks (synchronises `stream`)"""
        return self._read(stream, overflow_ok)[3]

    def get_counts(self, stream=None):
        """the last call's counts as a dict of DEDUP_COUNTS (synchronises `stream`)"""
        self._read(stream, True)
        return self.counts
