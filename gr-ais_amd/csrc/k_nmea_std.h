// k_nmea_std.h -- the batched NMEA armouring in the STANDARD form (the device form of aisx_pdu_to_nmea_std,
// aisx_framing.cpp, which is its specification): beside k_nmea.h, whose text stays the reference's byte for byte, the
// sentences a standard decoder reads -- the exact last payload character, the fill count on the last fragment only,
// a sequential message id on multi-sentence messages, and a tag block (\s:station,c:time*HH\) before every sentence.
// Records, text layout, counts and the bad-input flag are k_nmea.h's.
//
//   scan   as nmea_scan_body, with the standard form's closed-form length (nms_text_len) and a second scanned
//          quantity: the multi-sentence records before a record.  The written records are a prefix of the list, so
//          a written record's id is (the handle's counter + that count) mod 10, and the counter -- count[3], in
//          device memory -- advances by the multi-sentence records among the written.  No atomic decides an id.
//   write  one wave per record: the tag block (at most 43 bytes, the same before every fragment) once, one byte per
//          lane, its checksum an XOR over the wave; then every fragment's line -- tag block, sentence, newline, at
//          most 135 bytes -- three bytes per lane, 64 apart, with the sentence's checksum a second XOR over the wave.
#pragma once
#include "k_nmea.h"

namespace aisx {

constexpr int NMS_STATION = 15;     // station bytes per channel at most
constexpr int NMS_STRIDE = 16;      // ... and their stride in the handle's buffer (not NUL-terminated on the device)
constexpr int NMS_MAX_OCTETS = 378; // nine fragments of 56 characters: fragment numbers stay one digit
constexpr int NMS_TIME_DIGITS = 18; // what the parser reads of a c: value at most
constexpr long long NMS_TIME_END = 1000000000000000000ll; // 10^18
constexpr int NMS_LINE = 135;       // tag block + sentence + newline at most
constexpr int NMS_W_BYTES = 3;      // bytes per lane and fragment in the write kernel (3 * 64 >= NMS_LINE)
static_assert(NMS_W_BYTES * 64 >= NMS_LINE, "a lane's bytes cover the longest line");

AISX_HD int nms_time_digits(long long t) // decimal digits of a c: value, 0 for none (t < 0)
{
    int n = 0;
    for (; t >= 0 && (n == 0 || t > 0); t /= 10)
        n++;
    return n;
}

// bytes of the tag block of a station of slen bytes and a time of tdig digits: '\' fields '*' HH '\', 0 without fields
AISX_HD int nms_fields_len(int slen, int tdig) { return (slen ? 2 + slen : 0) + (slen && tdig ? 1 : 0) + (tdig ? 2 + tdig : 0); }
AISX_HD int nms_tag_len(int slen, int tdig)
{
    const int fl = nms_fields_len(slen, tdig);
    return fl ? fl + 5 : 0;
}

// What aisx_pdu_to_nmea_std returns for a payload of len octets (at most NMS_MAX_OCTETS), a designator of dlen bytes
// and a tag block of tag bytes; 0 for len = 0, which it refuses.  A fragment of n payload characters is
// tag + 18 + (1 with an id) + dlen + n long, and fragments are separated by '\n'.
AISX_HD int nms_text_len(int len, int dlen, int tag)
{
    if (len <= 0)
        return 0;
    const int P = nm_chars(len), F = (P + NM_FRAG - 1) / NM_FRAG;
    return F * (tag + 18 + (F > 1 ? 1 : 0) + dlen) + P + F - 1;
}

AISX_HD unsigned nms_armour(unsigned v) { return v + (v < 40 ? 48u : 56u); } // the inverse of the parser's rule

// group k of the payload: message bits 6k .. 6k + 5, most significant first, zero from bit 8 len on
AISX_HD unsigned nms_group(const unsigned char* pay, int len, int k)
{
    const int s = 6 * k, i = s >> 3;
    unsigned w = (unsigned)pay[i] << 8;
    if (i + 1 < len)
        w |= pay[i + 1];
    return (w >> (10 - (s & 7))) & 63u;
}

struct NmeaStdScanParams {
    NmeaScanParams s;          // (count[3]: the handle's message-id counter)
    const unsigned char* slen; // [nchan] station lengths
    unsigned char* ids;        // [max_pdus] the id of every written multi-sentence record
    int tdig;                  // digits of the call's time, 0 for none
};

struct NmeaStdWriteParams {
    NmeaWriteParams w;
    const char* station;       // [nchan][NMS_STRIDE]
    const unsigned char* slen;
    const unsigned char* ids;
    int tdig;
    unsigned bcd_hi;           // the time's decimal digits, four bits each: digits 16, 17 here, 0 .. 15 in bcd_lo
    unsigned long long bcd_lo;
};

AISX_HD unsigned nms_hex(unsigned x) { return x < 10 ? '0' + x : 'A' + x - 10; }

// one workgroup (any multiple of 64 threads): nmea_scan_body with the standard form's lengths and the ids
template <class Ctx>
AISX_DI void nmea_std_scan_body(Ctx& cx, const NmeaStdScanParams& q)
{
    const NmeaScanParams& p = q.s;
    const int t = cx.tid(), T = cx.nthreads(), w = t >> 6, l = t & 63, nw = T >> 6;
    int* wtot = (int*)cx.lds();   // [2][2][nw] wave totals of a tile (alternating tiles): text bytes, multi-sentence records
    int* shared = wtot + 4 * nw;  // [0] records written, [1] bad record seen, [2] multi-sentence records before the cut (-1: no cut)
    int n = *p.npdus;
    const bool bad_count = n < 0 || n > p.max_pdus;
    if (bad_count)
        n = 0;
    const int id0 = p.count[3];
    if (t == 0) {
        shared[0] = n;
        shared[1] = 0;
        shared[2] = -1;
    }
    cx.sync();
    long long base = 0; // text bytes of the tiles before
    int mbase = 0;      // multi-sentence records of the tiles before
    const int TL = T * NM_ITEMS;
    for (int t0 = 0, tile = 0; t0 < n; t0 += TL, tile++) {
        const int i0 = t0 + t * NM_ITEMS;
        HdlcRec r[NM_ITEMS];
        int slot[NM_ITEMS], sum = 0, msum = 0;
        unsigned multi = 0; // bit j: record i0 + j takes more than one sentence
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NM_ITEMS; j++)
            if (i0 + j < n)
                r[j] = p.in[i0 + j];
#pragma unroll
        for (int j = 0; j < NM_ITEMS; j++) {
            slot[j] = 0;
            if (i0 + j < n) {
                const int c = r[j].chan, len = r[j].len;
                if (c < 0 || c >= p.nchan || len < 0 || len > p.max_len) {
                    bad = true; // (no text, no id)
                } else {
                    const int tl = nms_text_len(len, p.dlen[c], nms_tag_len(q.slen[c], q.tdig));
                    slot[j] = tl ? tl + 1 : 0; // (the text and its newline; an empty payload has neither)
                    if (nm_chars(len) > NM_FRAG) {
                        multi |= 1u << j;
                        msum++;
                    }
                }
            }
            sum += slot[j];
        }
        if (bad)
            shared[1] = 1;
        const int incl = nm_wave_incl_sum(cx, sum), mincl = nm_wave_incl_sum(cx, msum);
        int* wt = wtot + (tile & 1) * 2 * nw;
        if (l == 63) {
            wt[w] = incl;
            wt[nw + w] = mincl;
        }
        cx.sync();
        long long st = base + incl - sum, tile_tot = 0;
        int mi = mbase + mincl - msum, mtile = 0;
        for (int v = 0; v < nw; v++) {
            const int x = wt[v], y = wt[nw + v];
            if (v < w) {
                st += x;
                mi += y;
            }
            tile_tot += x;
            mtile += y;
        }
#pragma unroll
        for (int j = 0; j < NM_ITEMS; j++) {
            const int i = i0 + j;
            if (i < n) {
                const long long end = st + slot[j];
                const bool m = (multi >> j) & 1u;
                if (end <= p.text_cap) {
                    HdlcRec o;
                    o.end_bit = r[j].end_bit;
                    o.offset = st;
                    o.chan = r[j].chan;
                    o.len = slot[j] ? slot[j] - 1 : 0;
                    p.out[i] = o;
                    if (m)
                        q.ids[i] = (unsigned char)((id0 + mi) % 10);
                } else if (st <= p.text_cap) {
                    shared[0] = i; // the first record that does not fit (there is one such record at most)
                    shared[2] = mi;
                }
                st = end;
                mi += m;
            }
        }
        base += tile_tot;
        mbase += mtile;
    }
    cx.sync();
    if (t == 0) {
        p.count[0] = bad_count ? 0 : (p.nfound ? *p.nfound : n);
        p.count[1] = shared[0];
        if (bad_count || shared[1])
            p.count[2] = 1;
        p.count[3] = (id0 + (shared[2] >= 0 ? shared[2] : mbase)) % 10;
    }
}

// one wave per record (a grid-stride loop over the records written): the record's fragments one after another
template <class Ctx>
AISX_DI void nmea_std_write_body(Ctx& cx, const NmeaStdWriteParams& q)
{
    const NmeaWriteParams& p = q.w;
    const int l = cx.tid() & 63;
    const int kept = p.count[1];
    for (int i = cx.bx() * (cx.nthreads() >> 6) + cx.wave_id(); i < kept; i += p.nwaves) {
        const HdlcRec o = p.out[i];
        if (o.len <= 0) // (an empty payload, or a record the scan refused)
            continue;
        const HdlcRec r = p.in[i];
        const int L = r.len, D = p.dlen[r.chan], S = q.slen[r.chan], td = q.tdig;
        const unsigned char* pay = p.bytes + r.offset;
        const char* des = p.desig + (long)r.chan * NM_DESIG;
        const char* sta = q.station + (long)r.chan * NMS_STRIDE;
        const int P = nm_chars(L), F = (P + NM_FRAG - 1) / NM_FRAG, fill = 6 * P - 8 * L;
        const int s = F > 1 ? 1 : 0, seq = s ? q.ids[i] : 0;
        // the tag block, byte l in lane l: '\' at 0, the fields at [1, fl], '*' at fl + 1, HH, '\' at Tg - 1
        const int fl = nms_fields_len(S, td), Tg = fl ? fl + 5 : 0;
        unsigned tch = 0;
        if (Tg) {
            const int c0 = fl - td; // "c:" stands at c0 - 1, c0, the time's digits behind it (no time: c0 = fl, not reached)
            if (l == 0 || l == Tg - 1)
                tch = '\\';
            else if (l <= fl) {
                if (S && l <= 2 + S)
                    tch = l == 1 ? 's' : l == 2 ? ':' : (unsigned char)sta[l - 3];
                else if (l < c0)
                    tch = l == c0 - 1 ? 'c' : ',';
                else if (l == c0)
                    tch = ':';
                else {
                    const int d = fl - l; // the digit's decimal place
                    tch = '0' + (unsigned)((d < 16 ? q.bcd_lo >> (4 * d) : (unsigned long long)q.bcd_hi >> (4 * (d - 16))) & 15u);
                }
            } else if (l == fl + 1)
                tch = '*';
            unsigned ts = l >= 1 && l <= fl ? tch : 0;
            for (int m = 32; m >= 1; m >>= 1)
                ts ^= (unsigned)cx.shfl_xor_i32((int)ts, m);
            if (l == fl + 2 || l == fl + 3)
                tch = nms_hex(l == fl + 2 ? (ts >> 4) & 15u : ts & 15u);
        }
        char* dst = p.text + o.offset;
        for (int f = 0; f < F; f++) {
            const int nf = P - f * NM_FRAG < NM_FRAG ? P - f * NM_FRAG : NM_FRAG;
            const int d0 = 12 + s;        // designator
            const int a = d0 + D;         // ',' before the payload
            const int b = a + 1 + nf;     // ',' before the fill count
            const int H = b + 5;          // '\n' (the sentence is [0, H) behind the tag block)
            unsigned ch[NMS_W_BYTES], sum = 0;
#pragma unroll
            for (int h = 0; h < NMS_W_BYTES; h++) {
                const int g = l + 64 * h - Tg; // position in the sentence
                unsigned v = 0;
                if (g < 0)
                    v = tch;
                else if (g == 0)
                    v = '!';
                else if (g < 7)
                    v = (unsigned char)"AIVDM,"[g - 1];
                else if (g == 7)
                    v = '0' + F;
                else if (g == 9)
                    v = '1' + f;
                else if (g < d0)
                    v = s && g == 11 ? '0' + seq : ',';
                else if (g < a)
                    v = (unsigned char)des[g - d0];
                else if (g == a || g == b)
                    v = ',';
                else if (g < b)
                    v = nms_armour(nms_group(pay, L, f * NM_FRAG + g - a - 1));
                else if (g == b + 1)
                    v = '0' + (f == F - 1 ? fill : 0);
                else if (g == b + 2)
                    v = '*';
                else if (g == H)
                    v = '\n';
                if (g >= 1 && g <= b + 1)
                    sum ^= v;
                ch[h] = v;
            }
            for (int m = 32; m >= 1; m >>= 1)
                sum ^= (unsigned)cx.shfl_xor_i32((int)sum, m);
#pragma unroll
            for (int h = 0; h < NMS_W_BYTES; h++) {
                const int g = l + 64 * h - Tg;
                if (g == b + 3 || g == b + 4)
                    ch[h] = nms_hex(g == b + 3 ? (sum >> 4) & 15u : sum & 15u);
                if (g <= H)
                    dst[g + Tg] = (char)ch[h];
            }
            dst += Tg + H + 1;
        }
    }
}

// ------------------------------------------------------------------
// The launch plan of a standard-form aisx_nmea_batch_* handle (host only): NmeaPlan's, with the stations, the ids
// and the form's own worst case.  aisx_nmea.hip runs it on device memory, tests/emul_nmea_std on host memory.
// ------------------------------------------------------------------

// a station is 0..15 bytes of A-Z a-z 0-9 _ -
inline bool nms_station_ok(const char* s)
{
    if (!s)
        return false;
    const size_t n = strnlen(s, NMS_STATION + 1);
    if (n > (size_t)NMS_STATION)
        return false;
    for (size_t k = 0; k < n; k++) {
        const char c = s[k];
        if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '-'))
            return false;
    }
    return true;
}

inline bool nms_time_ok(long long t) { return t >= -1 && t < NMS_TIME_END; }

// the index of the first station that is missing or not one, -1 when there is none (stations == nullptr: no stations)
inline int nms_bad_station(const char* const* stations, int nchan)
{
    for (int c = 0; stations && c < nchan; c++)
        if (!nms_station_ok(stations[c]))
            return c;
    return -1;
}

enum { NM_K_STD_SCAN = 2, NM_K_STD_WRITE };

struct NmeaStdBufs {
    NmeaBufs b;                // (count[3]: the message-id counter)
    const char* station;
    const unsigned char* slen;
    unsigned char* ids;
};

struct NmeaStdCall {
    NmeaStdScanParams s;
    NmeaStdWriteParams w;
};

struct NmeaStdPlan : NmeaPlan {
    std::vector<char> station_host;       // what the handle's station and slen buffers hold
    std::vector<unsigned char> slen_host;
    PlanBuf station, slen, ids;

    // the argument check of aisx_nmea_batch_create_std but the designators' and the stations' own
    static const char* check(const char* const* designators, int nchan, int max_pdus, int length_max, long text_cap)
    {
        static_assert(NMS_MAX_OCTETS == 378, "the bound in the text below");
        if (const char* why = NmeaPlan::check(designators, nchan, max_pdus, length_max, text_cap))
            return why;
        if (length_max - 1 > NMS_MAX_OCTETS)
            return "the standard form takes payloads of at most 378 octets (nine sentences): length_max <= 379";
        return nullptr;
    }
    NmeaStdPlan(const char* const* designators, const char* const* stations, int nchan_, int max_pdus_, int length_max, long text_cap_,
                int scan_t_ = NM_SCAN_T, int write_t_ = NM_W_T, int max_groups = NM_W_MAX_GROUPS)
        : NmeaPlan(designators, nchan_, max_pdus_, length_max, 0, scan_t_, write_t_, max_groups)
    {
        station_host.assign((size_t)nchan * NMS_STRIDE, 0);
        slen_host.assign(nchan, 0);
        int max_dlen = 0, max_slen = 0;
        nm_bad_designator(designators, nchan, &max_dlen);
        for (int c = 0; stations && c < nchan; c++) {
            slen_host[c] = (unsigned char)strlen(stations[c]);
            memcpy(station_host.data() + (size_t)c * NMS_STRIDE, stations[c], slen_host[c]);
            max_slen = slen_host[c] > max_slen ? slen_host[c] : max_slen;
        }
        // the worst case: every record as long as a payload can be, the longest designator and station, 18 digits of time
        const long long worst = (long long)max_pdus * (nms_text_len(length_max - 1, max_dlen, nms_tag_len(max_slen, NMS_TIME_DIGITS)) + 1);
        text_cap = text_cap_ == 0 || text_cap_ > worst ? worst : text_cap_;
        text = { (size_t)text_cap, false };
        station = { station_host.size(), false };
        slen = { slen_host.size(), false };
        ids = { (size_t)max_pdus, false };
    }

    // time: -1 or the c: value of this call's tag blocks (nms_time_ok)
    template <class Launch>
    bool process(const NmeaStdBufs& b, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound,
                 long long time, Launch&& launch) const
    {
        const NmeaCall base = call(b.b, pdus, bytes, npdus, nfound);
        NmeaStdCall c;
        c.s.s = base.s;
        c.s.slen = b.slen;
        c.s.ids = b.ids;
        c.s.tdig = nms_time_digits(time);
        c.w.w = base.w;
        c.w.station = b.station;
        c.w.slen = b.slen;
        c.w.ids = b.ids;
        c.w.tdig = c.s.tdig;
        c.w.bcd_lo = 0;
        c.w.bcd_hi = 0;
        for (int d = 0; d < c.s.tdig; d++, time /= 10) {
            if (d < 16)
                c.w.bcd_lo |= (unsigned long long)(time % 10) << (4 * d);
            else
                c.w.bcd_hi |= (unsigned)(time % 10) << (4 * (d - 16));
        }
        return launch(PlanLaunch{ NM_K_STD_SCAN, 1, 1, scan_t, (4 * (scan_t / 64) + 4) * 4 }, c) &&
               launch(PlanLaunch{ NM_K_STD_WRITE, write_groups, 1, write_t, 0 }, c);
    }
};

} // namespace aisx
