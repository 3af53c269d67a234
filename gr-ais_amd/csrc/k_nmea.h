// k_nmea.h -- batched NMEA armouring (the device form of aisx_pdu_to_nmea, aisx_framing.cpp, which is its
// specification): for every PDU record of a device list in the aisx_pdu layout (what the batched HDLC deframer
// returns), the !AIVDM sentence(s) byte for byte as the host function writes them, each record's text followed by
// one '\n', the records' texts one behind the other.
//
//   scan   one workgroup: a record's text length is a closed form of its payload length and its designator's
//          length (nm_text_len), so no payload is read here; an exclusive scan of the lengths in tiles of
//          NM_ITEMS consecutive records per thread places every record, and the records whose text (and newline)
//          end within text_cap -- a prefix -- are written to the output list with their text's offset and length;
//   write  one wave per record: every fragment's up to 93 characters, two per lane in consecutive bytes, the
//          payload characters from bits 6k .. 6k + 5 of the payload; the checksum is an XOR over the wave.
// No atomic decides where anything goes.
#pragma once
#include <string.h>

#include <vector>

#include "aisx_common.h"
#include "k_hdlc.h"

namespace aisx {

constexpr int NM_DESIG = 16;       // designator bytes per channel (at most; not NUL-terminated on the device)
constexpr int NM_FRAG = 56;        // payload characters per fragment
constexpr int NM_MAX_OCTETS = 1024; // length_max bound (the deframer's)
constexpr int NM_SCAN_T = 1024;
constexpr int NM_ITEMS = 8;        // consecutive records per thread and tile of the scan
constexpr int NM_W_T = 256;        // write kernel: four waves per workgroup
constexpr int NM_W_MAX_GROUPS = 4096;

struct NmeaScanParams {
    const HdlcRec* in;
    const int* npdus;          // one int on the device: records to armour
    const int* nfound;         // optional: PDUs the producer found
    const unsigned char* dlen; // [nchan] designator lengths
    int nchan, max_pdus, max_len; // max_len = length_max - 1 payload octets
    long long text_cap;
    HdlcRec* out;              // [max_pdus] offset / len of the text, chan / end_bit of the input
    int* count;                // [0] found, [1] records written, [2] set after bad input (cleared by the read)
};

struct NmeaWriteParams {
    const HdlcRec* in;
    const unsigned char* bytes;
    const HdlcRec* out;
    const int* count;
    const char* desig;         // [nchan][NM_DESIG]
    const unsigned char* dlen;
    char* text;
    int nwaves;                // waves in the grid (records are taken in strides of it)
};

AISX_HD int nm_digits(int v) { return v >= 10 ? 2 : 1; } // (fragment numbers are at most 25)
AISX_HD int nm_chars(int len) { return (8 * len + 5) / 6; } // payload characters of len octets
AISX_HD int nm_fill(int len) { return (6 - (8 * len) % 6) % 6; }

// What aisx_pdu_to_nmea returns for a payload of len octets and a designator of dlen bytes (0 for len = 0, which
// it refuses).  A fragment of n payload characters is 16 + digits(fragments) + digits(its number) + dlen + n long,
// and fragments are separated by '\n'.
AISX_HD int nm_text_len(int len, int dlen)
{
    if (len <= 0)
        return 0;
    const int P = nm_chars(len), F = (P + NM_FRAG - 1) / NM_FRAG;
    return F * (18 + nm_digits(F) + dlen) + (F > 9 ? F - 9 : 0) + P - 1;
}

// one payload character from a six-bit value (aisx_framing.cpp: armour), the signed-char quirk included
AISX_HD unsigned nm_armour(unsigned group)
{
    const int c = (int)(signed char)(unsigned char)group;
    return (unsigned char)(c + (c > 39 ? 56 : 48));
}

// group k of the payload: bits 6k .. 6k + 5, most significant first; the padded last group keeps the reference's
// quirk (its bits at the top of the group, shifted up by the fill count once more, in eight bits)
AISX_HD unsigned nm_group(const unsigned char* pay, int len, int k)
{
    const int s = 6 * k, i = s >> 3, held = 8 * len - s;
    if (held >= 6) {
        unsigned w = (unsigned)pay[i] << 8;
        if (i + 1 < len)
            w |= pay[i + 1];
        return (w >> (10 - (s & 7))) & 63u;
    }
    const int fill = 6 - held;
    const unsigned top = (pay[i] & ((1u << held) - 1u)) << fill;
    return (top << fill) & 0xFFu;
}

template <class Ctx>
AISX_DI int nm_wave_incl_sum(Ctx& cx, int v)
{
    const int l = cx.tid() & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int u = cx.shfl_i32(v, l >= d ? l - d : l);
        if (l >= d)
            v += u;
    }
    return v;
}

// one workgroup (any multiple of 64 threads): sizes, placement, the text_cap prefix, the counts
template <class Ctx>
AISX_DI void nmea_scan_body(Ctx& cx, const NmeaScanParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), w = t >> 6, l = t & 63, nw = T >> 6;
    int* wtot = (int*)cx.lds();   // [2][nw] wave totals of a tile (alternating tiles)
    int* shared = wtot + 2 * nw;  // [0] records written, [1] bad record seen
    int n = *p.npdus;
    const bool bad_count = n < 0 || n > p.max_pdus;
    if (bad_count)
        n = 0;
    if (t == 0) {
        shared[0] = n;
        shared[1] = 0;
    }
    cx.sync();
    long long base = 0; // text bytes of the tiles before
    const int TL = T * NM_ITEMS;
    for (int t0 = 0, tile = 0; t0 < n; t0 += TL, tile++) {
        const int i0 = t0 + t * NM_ITEMS;
        HdlcRec r[NM_ITEMS];
        int slot[NM_ITEMS], sum = 0;
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
                    bad = true; // (no text)
                } else {
                    const int tl = nm_text_len(len, p.dlen[c]);
                    slot[j] = tl ? tl + 1 : 0; // (the text and its newline; an empty payload has neither)
                }
            }
            sum += slot[j];
        }
        if (bad)
            shared[1] = 1;
        const int incl = nm_wave_incl_sum(cx, sum);
        int* wt = wtot + (tile & 1) * nw;
        if (l == 63)
            wt[w] = incl;
        cx.sync();
        long long st = base + incl - sum, tile_tot = 0;
        for (int v = 0; v < nw; v++) {
            const int x = wt[v];
            if (v < w)
                st += x;
            tile_tot += x;
        }
#pragma unroll
        for (int j = 0; j < NM_ITEMS; j++) {
            const int i = i0 + j;
            if (i < n) {
                const long long end = st + slot[j];
                if (end <= p.text_cap) {
                    HdlcRec o;
                    o.end_bit = r[j].end_bit;
                    o.offset = st;
                    o.chan = r[j].chan;
                    o.len = slot[j] ? slot[j] - 1 : 0;
                    p.out[i] = o;
                } else if (st <= p.text_cap) {
                    shared[0] = i; // the first record that does not fit (there is one such record at most)
                }
                st = end;
            }
        }
        base += tile_tot;
    }
    cx.sync();
    if (t == 0) {
        p.count[0] = bad_count ? 0 : (p.nfound ? *p.nfound : n);
        p.count[1] = shared[0];
        if (bad_count || shared[1])
            p.count[2] = 1;
    }
}

// one wave per record (a grid-stride loop over the records written): the record's fragments one after another
template <class Ctx>
AISX_DI void nmea_write_body(Ctx& cx, const NmeaWriteParams& p)
{
    const int l = cx.tid() & 63;
    const int kept = p.count[1];
    for (int i = cx.bx() * (cx.nthreads() >> 6) + cx.wave_id(); i < kept; i += p.nwaves) {
        const HdlcRec o = p.out[i];
        if (o.len <= 0) // (an empty payload, or a record the scan refused)
            continue;
        const HdlcRec r = p.in[i];
        const int L = r.len, D = p.dlen[r.chan];
        const unsigned char* pay = p.bytes + r.offset;
        const char* des = p.desig + (long)r.chan * NM_DESIG;
        const int P = nm_chars(L), F = (P + NM_FRAG - 1) / NM_FRAG, dF = nm_digits(F), fill = nm_fill(L);
        char* dst = p.text + o.offset;
        for (int f = 0; f < F; f++) {
            const int nf = P - f * NM_FRAG < NM_FRAG ? P - f * NM_FRAG : NM_FRAG;
            const int num = f + 1, df = nm_digits(num);
            const int d0 = 10 + dF + df;  // designator
            const int a = d0 + D;         // ',' before the payload
            const int b = a + 1 + nf;     // ',' before the fill count
            const int H = b + 5;          // '\n' (the fragment's text is [0, H))
            unsigned ch[2], sum = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int q = l + 64 * h;
                unsigned v = 0;
                if (q == 0)
                    v = '!';
                else if (q < 7)
                    v = (unsigned char)"AIVDM,"[q - 1];
                else if (q < 7 + dF)
                    v = '0' + (dF == 2 && q == 7 ? F / 10 : F % 10);
                else if (q == 7 + dF)
                    v = ',';
                else if (q < 8 + dF + df)
                    v = '0' + (df == 2 && q == 8 + dF ? num / 10 : num % 10);
                else if (q < d0)
                    v = ',';
                else if (q < a)
                    v = (unsigned char)des[q - d0];
                else if (q == a || q == b)
                    v = ',';
                else if (q < b)
                    v = nm_armour(nm_group(pay, L, f * NM_FRAG + q - a - 1));
                else if (q == b + 1)
                    v = '0' + fill;
                else if (q == b + 2)
                    v = '*';
                else if (q == H)
                    v = '\n';
                if (q >= 1 && q <= b + 1)
                    sum ^= v;
                ch[h] = v;
            }
            for (int m = 32; m >= 1; m >>= 1)
                sum ^= (unsigned)cx.shfl_xor_i32((int)sum, m);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int q = l + 64 * h;
                if (q == b + 3 || q == b + 4) {
                    const unsigned x = q == b + 3 ? (sum >> 4) & 15u : sum & 15u;
                    ch[h] = x < 10 ? '0' + x : 'A' + x - 10;
                }
                if (q <= H)
                    dst[q] = (char)ch[h];
            }
            dst += H + 1;
        }
    }
}

// ------------------------------------------------------------------
// The launch plan of aisx_nmea_batch_* (host only): the argument checks, the derived sizes, the buffers and the
// per-call sequence.  aisx_nmea.hip runs it on device memory, tests/emul_nmea on host memory.
// ------------------------------------------------------------------

// the designator check of aisx_nmea_batch_create, aisx_nmea_parse_batch_create and aisx_rx_create: the index of the
// first one that is missing or longer than NM_DESIG bytes, -1 when there is none; *max_dlen: the longest
inline int nm_bad_designator(const char* const* designators, int nchan, int* max_dlen = nullptr)
{
    int longest = 0;
    for (int c = 0; c < nchan; c++) {
        const size_t n = designators[c] ? strnlen(designators[c], NM_DESIG + 1) : NM_DESIG + 1;
        if (n > (size_t)NM_DESIG)
            return c;
        longest = (int)n > longest ? (int)n : longest;
    }
    if (max_dlen)
        *max_dlen = longest;
    return -1;
}

// checked designators as the kernels read them: desig [nchan][NM_DESIG] (not NUL-terminated), dlen [nchan]
inline void nm_pack_designators(const char* const* designators, int nchan, std::vector<char>& desig, std::vector<unsigned char>& dlen)
{
    desig.assign((size_t)nchan * NM_DESIG, 0);
    dlen.assign(nchan, 0);
    for (int c = 0; c < nchan; c++) {
        dlen[c] = (unsigned char)strlen(designators[c]);
        memcpy(desig.data() + (size_t)c * NM_DESIG, designators[c], dlen[c]);
    }
}

enum { NM_K_SCAN, NM_K_WRITE };

struct NmeaBufs {
    const char* desig;
    const unsigned char* dlen;
    HdlcRec* out;
    char* text;
    int* count; // [0] found, [1] records written, [2] bad-input flag, [3] the standard form's message-id counter
};

struct NmeaCall {
    NmeaScanParams s;
    NmeaWriteParams w;
};

struct NmeaPlan {
    int nchan, max_pdus, lmax, scan_t, write_t, write_groups;
    long long text_cap;
    std::vector<char> desig_host;         // what the handle's desig and dlen buffers hold
    std::vector<unsigned char> dlen_host;
    PlanBuf desig, dlen, out, text, count;

    // the argument check of aisx_nmea_batch_create but the designators' own (nm_bad_designator): nullptr when it passes
    static const char* check(const char* const* designators, int nchan, int max_pdus, int length_max, long text_cap)
    {
        static_assert(NM_MAX_OCTETS == 1024, "the bound in the text below");
        if (!designators || nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > NM_MAX_OCTETS || text_cap < 0)
            return "need designators, nchan >= 1, max_pdus >= 1, 2 <= length_max <= 1024, text_cap >= 0";
        return nullptr;
    }
    // scan_t, write_t: threads of the scan's one workgroup and of a write workgroup; max_groups: write workgroups at most
    NmeaPlan(const char* const* designators, int nchan_, int max_pdus_, int length_max, long text_cap_, int scan_t_ = NM_SCAN_T,
             int write_t_ = NM_W_T, int max_groups = NM_W_MAX_GROUPS)
        : nchan(nchan_), max_pdus(max_pdus_), lmax(length_max), scan_t(scan_t_), write_t(write_t_)
    {
        int max_dlen = 0;
        nm_bad_designator(designators, nchan, &max_dlen);
        // the worst case: every record as long as a payload can be, on the channel with the longest designator
        const long long worst = (long long)max_pdus * (nm_text_len(length_max - 1, max_dlen) + 1);
        text_cap = text_cap_ == 0 || text_cap_ > worst ? worst : text_cap_;
        const long long groups = ((long long)max_pdus + write_t / 64 - 1) / (write_t / 64);
        write_groups = (int)(groups < max_groups ? groups : max_groups);
        nm_pack_designators(designators, nchan, desig_host, dlen_host);
        desig = { desig_host.size(), false };
        dlen = { dlen_host.size(), false };
        out = { (size_t)max_pdus, false };
        text = { (size_t)text_cap, false };
        count = { 4, true };
    }

    // a call's kernel arguments (the standard form's plan, k_nmea_std.h, starts from them too)
    NmeaCall call(const NmeaBufs& b, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound) const
    {
        NmeaCall c;
        NmeaScanParams& s = c.s;
        s.in = pdus;
        s.npdus = npdus;
        s.nfound = nfound;
        s.dlen = b.dlen;
        s.nchan = nchan;
        s.max_pdus = max_pdus;
        s.max_len = lmax - 1;
        s.text_cap = text_cap;
        s.out = b.out;
        s.count = b.count;
        NmeaWriteParams& w = c.w;
        w.in = s.in;
        w.bytes = bytes;
        w.out = b.out;
        w.count = b.count;
        w.desig = b.desig;
        w.dlen = b.dlen;
        w.text = b.text;
        w.nwaves = write_groups * (write_t / 64);
        return c;
    }

    template <class Launch>
    bool process(const NmeaBufs& b, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound,
                 Launch&& launch) const
    {
        const NmeaCall c = call(b, pdus, bytes, npdus, nfound);
        return launch(PlanLaunch{ NM_K_SCAN, 1, 1, scan_t, (2 * (scan_t / 64) + 2) * 4 }, c) &&
               launch(PlanLaunch{ NM_K_WRITE, write_groups, 1, write_t, 0 }, c);
    }
};

} // namespace aisx
