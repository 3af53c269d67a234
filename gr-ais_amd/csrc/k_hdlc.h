// k_hdlc.h -- batched HDLC deframer (the device form of aisx_hdlc_work, aisx_framing.cpp, which is its
// specification): for every channel of a chain step, the PDUs whose CRC-16/X.25 checks, bit-exact with one host
// aisx_hdlc handle per channel fed the same bits in call order.
//
// One wave per channel, 4096 bits per pass, one 64-bit word of the bit stream per lane:
//   load     16 bytes per lane (aligned blocks, the row's misalignment removed afterwards), one bit per byte
//            (any nonzero byte is a 1), through LDS into the lane's word;
//   classify run5 = "the previous five bits are all ones" from the word and its predecessor (the last word of
//            the previous pass or call: the carried history), delim = bit & run5, data = ~run5 -- a zero behind
//            five ones is a stuffed bit and a one behind five ones closes a frame, whatever came before;
//   compact  the data bits into one LDS bit array behind the open frame's carried bits (prefix of the per-word
//            popcounts), so that every frame is a contiguous run of it;
//   frames   a delimiter at data position a whose segment (since the previous delimiter) holds d data bits
//            closes a frame of r = d mod P data bits, P = 8 (length_max + 1) + 1 (the length_max rule drops a
//            frame that has outgrown length_max at its next data bit and starts again behind it), i.e. of r / 8
//            whole octets starting at a - r; frames of at least length_min octets are CRC-checked bytewise
//            with a table in LDS, and the good ones written in bit order to the channel's staging area;
//   carry    the last 64 bits, the stream position and the open frame's bits since its last start (at most
//            8 (length_max + 1)) go to the next pass / call.
// Single-bit repair (hdlc_deframe_body<Ctx, true>, launched only for a handle with rules): a frame whose FCS fails and
// whose length has a rule looks its syndrome up in a 65536-entry table in global memory (one 2-byte load); a single
// error inside the frame whose message type the rule allows makes the frame a good one, its bit flipped in the byte on
// the way to staging (never in the LDS array: frames sharing a delimiter read it too) and its index kept beside the
// record.
// Error-event repair (hdlc_deframe_body<Ctx, true, true>, launched only for a handle whose event mask is not the
// single event alone): the table is the mask's (aisx_hdlc_event_table: event id and distance of its last flipped bit),
// the lookup gives id and the first flipped bit's index in the same 16 bits per good frame, the bytes on the way to
// staging take up to two flips, which may sit in two octets, and the mark beside the record is index | id << 16.
// hdlc_scan_body then places every channel's records behind those of the channels before it (one workgroup,
// a scan of the counts) and hdlc_gather_body copies them there: records ordered by channel and end bit, no
// atomic decides where one goes.
#pragma once
#include "aisx_common.h"

namespace aisx {

constexpr int HD_T = 64;                                            // one wave per channel
constexpr int HD_TILE = 64 * 64;                                    // bits per pass: a 64-bit word per lane
constexpr int HD_MAX_OCTETS = 1024;                                 // length_max bound
constexpr int HD_OPEN_BITS = 8 * (HD_MAX_OCTETS + 1);               // open frame carried between passes
constexpr int HD_ARR_WORDS = (HD_OPEN_BITS + HD_TILE) / 64 + 4;     // data-bit array (+ the words a read spills into)
constexpr int HD_LDS_SLOTS = 256 * 2;                               // behind the CRC table (256 x u16)
constexpr int HD_LDS_ARR = HD_LDS_SLOTS + 66 * 8;                   // 260 16-bit load slots (+ padding)
constexpr int HD_LDS_BYTES = HD_LDS_ARR + HD_ARR_WORDS * 8;
constexpr int HD_SCAN_T = 256;
constexpr int HD_MAX_RULES = 16;                                    // AISX_HDLC_MAX_RULES
constexpr int HD_LDS_BYTES_REPAIR = HD_LDS_BYTES + HD_MAX_RULES * 16; // the rules behind the array

struct HdlcState {
    unsigned long long hist; // the last 64 bits of the stream, the newest in bit 63
    unsigned long long pos;  // bits consumed since create / reset
    int open;                // data bits of the open frame since its last start (bits [0, open) of the carry row)
    int pad;
};

// aisx_pdu's layout (static_assert in aisx_hdlc.hip)
struct HdlcRec {
    unsigned long long end_bit;
    long long offset;
    int chan, len;
};

// aisx_hdlc_rule's layout (static_assert in aisx_hdlc.hip)
struct HdlcRule {
    int payload_octets, reserved;
    unsigned long long type_mask;
};

struct HdlcParams {
    const unsigned char* bits; long stride; // [nchan][stride] one bit per byte
    const int* nbits;                       // [nchan] bits of this call, read on the device
    int max_bits, lmin, lmax;
    HdlcState* st;                          // [nchan]
    unsigned long long* carry;              // [nchan][carry_words] open-frame bits
    int carry_words;
    HdlcRec* srec; int rec_cap;             // [nchan][rec_cap] staging: offsets relative to the channel's bytes
    unsigned char* sbytes; int byte_cap;    // [nchan][byte_cap]
    int* cnt; int* nbytes;                  // [nchan] records / payload bytes of this call
    int* flags;                             // [0] set when a channel's count was out of range
    // single-bit repair (read by hdlc_deframe_body<Ctx, true> alone)
    const HdlcRule* rules = nullptr; int nrules = 0;
    const unsigned short* syn_inv = nullptr; // [65536] syndrome -> distance from the frame's last bit + 1, 0 = none
                                             // (EVENTS: event id << 14 | distance of its last flipped bit + 1)
    int* sfix = nullptr;                     // [nchan][rec_cap] staging: the flipped bit's index in the frame, -1 = none
                                             // (EVENTS: the first flipped bit's index | event id << 16)
};

struct HdlcScanParams {
    const int* cnt; const int* nbytes;
    long long* rec_base; long long* byte_base; // [nchan] where each channel's records / bytes go
    int nchan, max_pdus;
    int* count;                                // [0] records found (all channels), [1] records kept
};

struct HdlcGatherParams {
    const HdlcRec* srec; int rec_cap;
    const unsigned char* sbytes; int byte_cap;
    const int* cnt; const int* nbytes;
    const long long* rec_base; const long long* byte_base;
    int max_pdus;
    HdlcRec* out; unsigned char* out_bytes;
    const int* sfix = nullptr; int* out_fix = nullptr; // the records' repair marks (both or neither)
};

struct alignas(16) HdB16 {
    unsigned long long a, b;
};

// bit j = (byte j of x != 0)
AISX_HD unsigned hd_nz8(unsigned long long x)
{
    const unsigned long long m7 = 0x7F7F7F7F7F7F7F7FULL;
    const unsigned long long t = ((((x & m7) + m7) | x) >> 7) & 0x0101010101010101ULL;
    return (unsigned)((t * 0x0102040810204080ULL) >> 56);
}
AISX_HD unsigned long long hd_below(int i) { return i >= 64 ? ~0ULL : ((1ULL << i) - 1ULL); }
AISX_HD int hd_popc(unsigned long long v) { return __builtin_popcountll(v); }
AISX_HD int hd_top(unsigned long long v) { return 63 - __builtin_clzll(v); } // v != 0
AISX_HD int hd_low(unsigned long long v) { return __builtin_ctzll(v); }      // v != 0
// 64 bits of a bit array from bit `pos` on (a[pos / 64 + 1] must be readable)
AISX_HD unsigned long long hd_read64(const unsigned long long* a, int pos)
{
    const int q = pos >> 6, s = pos & 63;
    return s ? (a[q] >> s) | (a[q + 1] << (64 - s)) : a[q];
}

// inclusive sum over the wave's lanes
template <class Ctx>
AISX_DI int hd_wave_sum(Ctx& cx, int v)
{
    const int l = cx.tid() & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int u = cx.shfl_i32(v, l >= d ? l - d : l);
        if (l >= d)
            v += u;
    }
    return v;
}

// the frame of `oct` octets at bit `fs` of the data-bit array: does its FCS (last two octets, low byte first)
// match CRC-16/X.25 of the octets before it?  Returns the syndrome, (computed FCS) xor (sent FCS): 0 = it matches.
AISX_HD unsigned hd_fcs_syndrome(const unsigned short* crc, const unsigned long long* arr, int fs, int oct)
{
    const int payload = oct - 2;
    unsigned reg = 0xFFFFu;
    for (int k = 0; k < payload; k += 8) {
        const unsigned long long v = hd_read64(arr, fs + 8 * k);
        const int m = payload - k < 8 ? payload - k : 8;
        for (int j = 0; j < m; j++)
            reg = (reg >> 8) ^ crc[(reg ^ (unsigned)(v >> (8 * j))) & 0xFFu];
    }
    const unsigned sent = (unsigned)(hd_read64(arr, fs + 8 * payload) & 0xFFFFu);
    return (~reg & 0xFFFFu) ^ sent;
}
AISX_HD bool hd_fcs_ok(const unsigned short* crc, const unsigned long long* arr, int fs, int oct)
{
    return hd_fcs_syndrome(crc, arr, fs, oct) == 0;
}

// the frame of `oct` octets at bit `fs` failed its FCS with `syn`: the index of the one bit to flip (0 = the frame's
// first bit), or -1 when the frame's length has no rule, no single error inside the frame gives the syndrome, or the
// message type after the flip is not one the rule allows
AISX_HD int hd_repair_bit(const HdlcRule* rules, int nrules, const unsigned short* syn_inv, const unsigned long long* arr, int fs,
                          int oct, unsigned syn)
{
    int k = 0;
    while (k < nrules && rules[k].payload_octets != oct - 2)
        k++;
    if (k == nrules)
        return -1;
    const int d1 = syn_inv[syn];
    if (d1 == 0 || d1 - 1 >= 8 * oct)
        return -1;
    const int i = 8 * oct - d1;
    const unsigned first = ((unsigned)hd_read64(arr, fs) & 0xFFu) ^ (i < 8 ? 1u << i : 0u);
    return ((rules[k].type_mask >> (first >> 2)) & 1ULL) ? i : -1;
}

// hd_repair_bit for the error events of a mask's table: event id << 14 | (index of the event's FIRST flipped bit + 1),
// or 0 under hd_repair_bit's conditions, all of the event's bits inside the frame (an event's span is its id) and the
// type read with every flip below bit 8 applied
AISX_HD unsigned hd_repair_event(const HdlcRule* rules, int nrules, const unsigned short* ev_tab, const unsigned long long* arr,
                                 int fs, int oct, unsigned syn)
{
    int k = 0;
    while (k < nrules && rules[k].payload_octets != oct - 2)
        k++;
    if (k == nrules)
        return 0u;
    const unsigned v = ev_tab[syn];
    const int id = (int)(v >> 14), d1 = (int)(v & 0x3FFFu);
    if (d1 == 0 || d1 - 1 + id >= 8 * oct)
        return 0u;
    const int last = 8 * oct - d1, i = last - id;
    const unsigned flips = ((i < 8 ? 1u << i : 0u) | (last < 8 ? 1u << last : 0u)) & 0xFFu;
    const unsigned first = ((unsigned)hd_read64(arr, fs) & 0xFFu) ^ flips;
    return ((rules[k].type_mask >> (first >> 2)) & 1ULL) ? ((unsigned)id << 14) | (unsigned)(i + 1) : 0u;
}

template <class Ctx, bool REPAIR = false, bool EVENTS = false>
AISX_DI void hdlc_deframe_body(Ctx& cx, const HdlcParams& p)
{
    static_assert(REPAIR || !EVENTS, "the error events are a form of the repair");
    const int l = cx.tid();
    const int c = cx.bx();
    char* lds = cx.lds();
    unsigned short* crc = (unsigned short*)lds;
    unsigned short* slots16 = (unsigned short*)(lds + HD_LDS_SLOTS);
    const unsigned long long* slots = (const unsigned long long*)(lds + HD_LDS_SLOTS);
    unsigned long long* arr = (unsigned long long*)(lds + HD_LDS_ARR);
    HdlcRule* rules = (HdlcRule*)(lds + HD_LDS_BYTES); // (REPAIR: HD_LDS_BYTES_REPAIR bytes of LDS)
    const int n = p.nbits[c];
    if (n < 0 || n > p.max_bits) { // not advanced; reported by the next read
        if (l == 0) {
            p.cnt[c] = 0;
            p.nbytes[c] = 0;
            p.flags[0] = 1;
        }
        return;
    }
    for (int k = 0; k < 4; k++) { // CRC-16/X.25 table: 0x1021 reflected
        unsigned r = (unsigned)(l + 64 * k);
        for (int j = 0; j < 8; j++)
            r = (r >> 1) ^ ((r & 1u) ? 0x8408u : 0u);
        crc[l + 64 * k] = (unsigned short)r;
    }
    if constexpr (REPAIR)
        if (l < p.nrules && l < HD_MAX_RULES)
            rules[l] = p.rules[l];
    const int nrules = p.nrules < HD_MAX_RULES ? p.nrules : HD_MAX_RULES;
    const HdlcState s0 = p.st[c];
    unsigned long long hist = s0.hist;
    int c0 = s0.open;
    unsigned long long* carry = p.carry + (long)c * p.carry_words;
    for (int j = l; j < HD_ARR_WORDS; j += 64) {
        unsigned long long v = 0;
        if (j * 64 < c0)
            v = carry[j] & hd_below(c0 - j * 64);
        arr[j] = v;
    }
    cx.sync();
    const unsigned char* row = p.bits + (long)c * p.stride;
    const int sh = (int)((unsigned long long)(size_t)row & 15u); // the row's offset in its first aligned block
    const unsigned char* ab = row - sh;
    HdlcRec* rec = p.srec + (long)c * p.rec_cap;
    unsigned char* outb = p.sbytes + (long)c * p.byte_cap;
    const int P = 8 * (p.lmax + 1) + 1;
    int nrec = 0, nbyt = 0;
    for (int t0 = 0; t0 < n; t0 += HD_TILE) {
        const int nb = n - t0 < HD_TILE ? n - t0 : HD_TILE;
        // blocks 0..256 of this pass (the 257th feeds the last word's top bits when the row is misaligned); only
        // aligned 16-byte blocks that hold at least one byte of the row's n are read
        for (int k = 0; k < 5; k++) {
            const int slot = 64 * k + l;
            if (k == 4 && l >= 4)
                break;
            const long J = (long)(t0 / 16) + slot;
            unsigned m = 0;
            if (k < 4 || l == 0)
                if (16 * J < (long)sh + n) {
                    const HdB16 v = *(const HdB16*)(ab + 16 * J);
                    m = hd_nz8(v.a) | (hd_nz8(v.b) << 8);
                }
            slots16[slot] = (unsigned short)m;
        }
        cx.sync();
        const int w = l;
        const int vb = nb - 64 * w <= 0 ? 0 : (nb - 64 * w >= 64 ? 64 : nb - 64 * w);
        const unsigned long long valid = hd_below(vb);
        const unsigned long long B = (sh ? (slots[w] >> sh) | (slots[w + 1] << (64 - sh)) : slots[w]) & valid;
        const unsigned long long pw = cx.shfl_u64(B, w > 0 ? w - 1 : 0);
        const unsigned long long prev = w > 0 ? pw : hist;
        unsigned long long run5 = ~0ULL;
        for (int k = 1; k <= 5; k++)
            run5 &= (B << k) | (prev >> (64 - k));
        const unsigned long long delim = B & run5;
        const unsigned long long data = ~run5 & valid;
        const int dc = hd_popc(data);
        const int dsum = hd_wave_sum(cx, dc);
        const int base = c0 + dsum - dc; // data position of this word's first data bit
        const int a_end = c0 + cx.shfl_i32(dsum, 63);
        // this word's data bits, stuffed zeros and delimiters taken out (highest first)
        unsigned long long x = B;
        for (unsigned long long rem = run5 & valid; rem;) {
            const int i = hd_top(rem);
            rem &= ~(1ULL << i);
            const unsigned long long lo = hd_below(i);
            x = (x & lo) | ((x >> 1) & ~lo);
        }
        if (dc) {
            const int q = base >> 6, s = base & 63;
            cx.atomic_or64(&arr[q], x << s);
            if (s && s + dc > 64)
                cx.atomic_or64(&arr[q + 1], x >> (64 - s));
        }
        // each lane publishes the data position of its word's LAST delimiter (encoded + 1, 0 = none); the exclusive
        // prefix max over the lanes before it is where the segment of this word's first delimiter starts (none in
        // this pass: 0, the open frame's start), the max over all lanes where the segment left open at the pass's
        // end starts
        const int enc = delim ? base + hd_popc(data & hd_below(hd_top(delim))) + 1 : 0;
        int all = 0;
        const int penc = cx.wave_excl_prefix_max_nn(enc);
        (void)cx.wave_excl_suffix_max_nn(enc, all);
        const int st0 = penc > 0 ? penc - 1 : 0;
        const int s_end = all > 0 ? all - 1 : 0;
        const int wl = (nb - 1) >> 6;
        const unsigned long long hn = vb == 64 ? B : (vb == 0 ? prev : (B << (64 - vb)) | (prev >> vb));
        hist = cx.shfl_u64(hn, wl);
        cx.sync();
        // frames closed in this word: length and CRC
        // (REPAIR: fixes holds, 16 bits per good frame of this word in order, the flipped bit's index + 1 or 0 -- a
        // good frame is at least 16 data bits and its delimiter, so a word closes four at most; EVENTS: the index is
        // the first flipped bit's, 14 bits of it, and the event's id sits in the two bits above)
        unsigned long long good = 0, fixes = 0;
        int ng = 0, gb = 0;
        {
            int st = st0;
            for (unsigned long long dm = delim; dm; dm &= dm - 1) {
                const int i = hd_low(dm);
                const int a = base + hd_popc(data & hd_below(i));
                const int r = (a - st) % P;
                const int oct = r >> 3;
                if (oct >= p.lmin) {
                    const unsigned syn = hd_fcs_syndrome(crc, arr, a - r, oct);
                    int fix = -1;
                    if constexpr (EVENTS) {
                        if (syn != 0)
                            fix = (int)hd_repair_event(rules, nrules, p.syn_inv, arr, a - r, oct, syn) - 1;
                    } else if constexpr (REPAIR) {
                        if (syn != 0)
                            fix = hd_repair_bit(rules, nrules, p.syn_inv, arr, a - r, oct, syn);
                    }
                    if (syn == 0 || fix >= 0) {
                        if constexpr (REPAIR)
                            fixes |= (unsigned long long)(fix + 1) << (16 * (ng & 3));
                        good |= 1ULL << i;
                        ng++;
                        gb += oct - 2;
                    }
                }
                st = a;
            }
        }
        const int gsum = hd_wave_sum(cx, ng), bsum = hd_wave_sum(cx, gb);
        {
            int ri = nrec + gsum - ng, bo = nbyt + bsum - gb;
            for (unsigned long long gm = good; gm; gm &= gm - 1) {
                const int i = hd_low(gm);
                const unsigned long long before = delim & hd_below(i);
                const int a = base + hd_popc(data & hd_below(i));
                const int st = before ? base + hd_popc(data & hd_below(hd_top(before))) : st0;
                const int r = (a - st) % P;
                const int len = (r >> 3) - 2;
                if (ri < p.rec_cap && bo + len <= p.byte_cap) { // (the staging is sized so that this always holds)
                    HdlcRec o;
                    o.end_bit = s0.pos + (unsigned long long)(t0 + 64 * w + i);
                    o.offset = bo;
                    o.chan = c;
                    o.len = len;
                    rec[ri] = o;
                    const int code = REPAIR ? (int)(fixes & 0xFFFFu) : 0;
                    // the first flipped bit and the event's other one (REPAIR alone: the one bit, twice)
                    const int fix = (EVENTS ? code & 0x3FFF : code) - 1;
                    const int id = EVENTS ? code >> 14 : 0, fix2 = fix + id;
                    for (int k = 0; k < len; k++) {
                        unsigned v = (unsigned)hd_read64(arr, a - r + 8 * k);
                        if constexpr (REPAIR)
                            if ((fix >> 3) == k) // (never for -1, nor for a wrong bit in the FCS, which is not delivered)
                                v ^= 1u << (fix & 7);
                        if constexpr (EVENTS)
                            if (id && (fix2 >> 3) == k)
                                v ^= 1u << (fix2 & 7);
                        outb[bo + k] = (unsigned char)v;
                    }
                    if constexpr (REPAIR)
                        p.sfix[(long)c * p.rec_cap + ri] = EVENTS && fix >= 0 ? fix | (id << 16) : fix;
                }
                if constexpr (REPAIR)
                    fixes >>= 16;
                ri++;
                bo += len;
            }
        }
        nrec += cx.shfl_i32(gsum, 63);
        nbyt += cx.shfl_i32(bsum, 63);
        // the open frame's bits since its last start move to the front of the array
        const int rn = (a_end - s_end) % P;
        const int src = a_end - rn, nw = (rn + 63) >> 6;
        unsigned long long mv[3];
        for (int k = 0; k < 3; k++) {
            const int j = l + 64 * k;
            mv[k] = j < nw ? hd_read64(arr, src + 64 * j) & hd_below(rn - 64 * j) : 0ULL;
        }
        cx.sync();
        for (int k = 0; k < 4; k++) {
            const int j = l + 64 * k;
            if (j < HD_ARR_WORDS)
                arr[j] = k < 3 ? mv[k] : 0ULL;
        }
        c0 = rn;
        cx.sync();
    }
    for (int j = l; j < p.carry_words; j += 64)
        carry[j] = arr[j];
    if (l == 0) {
        HdlcState s1;
        s1.hist = hist;
        s1.pos = s0.pos + (unsigned long long)n;
        s1.open = c0;
        s1.pad = 0;
        p.st[c] = s1;
        p.cnt[c] = nrec;
        p.nbytes[c] = nbyt;
    }
}

// one workgroup: channel c's records go to [rec_base[c], + cnt[c]), its bytes to [byte_base[c], + nbytes[c])
template <class Ctx>
AISX_DI void hdlc_scan_body(Ctx& cx, const HdlcScanParams& p)
{
    const int t = cx.tid(), T = cx.nthreads();
    long long* sr = (long long*)cx.lds();
    long long* sb = sr + T;
    const int per = (p.nchan + T - 1) / T;
    const int lo = t * per < p.nchan ? t * per : p.nchan, hi = lo + per < p.nchan ? lo + per : p.nchan;
    long long r = 0, b = 0;
    for (int c = lo; c < hi; c++) {
        r += p.cnt[c];
        b += p.nbytes[c];
    }
    sr[t] = r;
    sb[t] = b;
    cx.sync();
    for (int d = 1; d < T; d <<= 1) {
        const long long ur = t >= d ? sr[t - d] : 0, ub = t >= d ? sb[t - d] : 0;
        cx.sync();
        sr[t] += ur;
        sb[t] += ub;
        cx.sync();
    }
    long long rb = sr[t] - r, bb = sb[t] - b;
    for (int c = lo; c < hi; c++) {
        p.rec_base[c] = rb;
        p.byte_base[c] = bb;
        rb += p.cnt[c];
        bb += p.nbytes[c];
    }
    if (t == T - 1) {
        const long long tot = sr[T - 1];
        p.count[0] = tot > 0x7FFFFFFFLL ? 0x7FFFFFFF : (int)tot;
        p.count[1] = tot < (long long)p.max_pdus ? (int)tot : p.max_pdus;
    }
}

// one wave per channel: the records that fit (a prefix of the ordered list) and their bytes
template <class Ctx>
AISX_DI void hdlc_gather_body(Ctx& cx, const HdlcGatherParams& p)
{
    const int l = cx.tid(), c = cx.bx();
    const long long rb = p.rec_base[c], bb = p.byte_base[c];
    const int nr = p.cnt[c];
    const long long room = (long long)p.max_pdus - rb;
    const int nk = room <= 0 ? 0 : (room < nr ? (int)room : nr);
    const HdlcRec* in = p.srec + (long)c * p.rec_cap;
    for (int j = l; j < nk; j += 64) {
        HdlcRec o = in[j];
        o.offset += bb;
        p.out[rb + j] = o;
        if (p.out_fix)
            p.out_fix[rb + j] = p.sfix[(long)c * p.rec_cap + j];
    }
    const int kb = nk == nr ? p.nbytes[c] : (int)in[nk].offset;
    const unsigned char* sb = p.sbytes + (long)c * p.byte_cap;
    for (int k = l; k < kb; k += 64)
        p.out_bytes[bb + k] = sb[k];
}

// ------------------------------------------------------------------
// The launch plan of aisx_hdlc_batch_* (host only): the argument check, the derived sizes, the buffers and the
// per-call sequence.  aisx_hdlc.hip runs it on device memory, tests/emul_hdlc on host memory.
// ------------------------------------------------------------------
enum { HD_K_DEFRAME, HD_K_DEFRAME_REPAIR, HD_K_DEFRAME_EVENTS, HD_K_SCAN, HD_K_GATHER };

struct HdlcBufs { // a handle's buffers, sized by the HdlcPlan members of the same names
    HdlcState* st;
    unsigned long long* carry;
    HdlcRec* srec;
    unsigned char* sbytes;
    int* cnt;        // [nchan] records, [nchan] bytes
    long long* base; // [nchan] record bases, [nchan] byte bases
    int* count;      // [0] found, [1] kept, [2] bad-count flag
    HdlcRec* out;
    unsigned char* out_bytes;
    int* fix;        // [max_pdus] the records' repair marks
    const HdlcRule* rules; // a handle with rules: they, the staging of the marks and the syndrome table in use
    int* sfix;
    const unsigned short* syn;
};

struct HdlcCall {
    HdlcParams p;
    HdlcScanParams s;
    HdlcGatherParams g;
};

struct HdlcPlan {
    int lmin, lmax, nchan, max_bits, max_pdus, scan_t;
    int carry_words, rec_cap, byte_cap;
    long long out_bytes_cap;
    PlanBuf st, carry, srec, sbytes, cnt, base, count, out, out_bytes, fix, rules, sfix, syn;

    // the argument check of aisx_hdlc_batch_create: nullptr when it passes, else what is needed
    static const char* check(int length_min, int length_max, int nchan, int max_bits, int max_pdus)
    {
        static_assert(HD_MAX_OCTETS == 1024, "the bound in the text below");
        if (length_min < 2 || length_max < length_min || length_max > HD_MAX_OCTETS || nchan < 1 || max_bits < 1 ||
            max_bits > (1 << 28) || max_pdus < 1)
            return "need 2 <= length_min <= length_max <= 1024, nchan >= 1, 1 <= max_bits <= 2^28, max_pdus >= 1";
        return nullptr;
    }
    // scan_t: threads of the scan's one workgroup (the device runs HD_SCAN_T)
    HdlcPlan(int length_min, int length_max, int nchan_, int max_bits_, int max_pdus_, int scan_t_ = HD_SCAN_T)
        : lmin(length_min), lmax(length_max), nchan(nchan_), max_bits(max_bits_), max_pdus(max_pdus_), scan_t(scan_t_)
    {
        // a call's good frames per channel: disjoint runs of >= 8 length_min data bits, each closed by a bit of its
        // own, all but the first inside the call's bits; their payload comes from the open frame and the call's bits
        const long long span = 8LL * (lmax + 1) + max_bits;
        carry_words = (8 * (lmax + 1) + 63) / 64;
        rec_cap = (int)(span / (8LL * lmin + 1) + 2);
        byte_cap = (int)(span / 8 + 8);
        out_bytes_cap = (long long)max_pdus * (lmax - 1); // (a payload is at most length_max - 1 octets)
        const size_t nc = (size_t)nchan;
        st = { nc, true };
        carry = { nc * carry_words, true };
        srec = { nc * rec_cap, false };
        sbytes = { nc * byte_cap, false };
        cnt = { 2 * nc, true };
        base = { 2 * nc, true };
        count = { 4, true };
        out = { (size_t)max_pdus, true };
        out_bytes = { (size_t)out_bytes_cap, true };
        fix = { (size_t)max_pdus, false }; // (filled with -1 while the handle has no rules)
        rules = { HD_MAX_RULES, true };
        sfix = { nc * rec_cap, false };
        syn = { 65536, false };
    }

    // a call: nrules > 0 runs the repairing deframer, `events` the one of a mask that is not the single event alone
    template <class Launch>
    bool process(const HdlcBufs& b, const unsigned char* bits, long stride, const int* nbits, int nrules, bool events,
                 Launch&& launch) const
    {
        HdlcCall c;
        HdlcParams& p = c.p;
        p.bits = bits;
        p.stride = stride;
        p.nbits = nbits;
        p.max_bits = max_bits;
        p.lmin = lmin;
        p.lmax = lmax;
        p.st = b.st;
        p.carry = b.carry;
        p.carry_words = carry_words;
        p.srec = b.srec;
        p.rec_cap = rec_cap;
        p.sbytes = b.sbytes;
        p.byte_cap = byte_cap;
        p.cnt = b.cnt;
        p.nbytes = b.cnt + nchan;
        p.flags = b.count + 2;
        if (nrules > 0) {
            p.rules = b.rules;
            p.nrules = nrules;
            p.sfix = b.sfix;
            p.syn_inv = b.syn;
        }
        HdlcScanParams& s = c.s;
        s.cnt = p.cnt;
        s.nbytes = p.nbytes;
        s.rec_base = b.base;
        s.byte_base = b.base + nchan;
        s.nchan = nchan;
        s.max_pdus = max_pdus;
        s.count = b.count;
        HdlcGatherParams& g = c.g;
        g.srec = b.srec;
        g.rec_cap = rec_cap;
        g.sbytes = b.sbytes;
        g.byte_cap = byte_cap;
        g.cnt = p.cnt;
        g.nbytes = p.nbytes;
        g.rec_base = s.rec_base;
        g.byte_base = s.byte_base;
        g.max_pdus = max_pdus;
        g.out = b.out;
        g.out_bytes = b.out_bytes;
        if (nrules > 0) {
            g.sfix = b.sfix;
            g.out_fix = b.fix;
        }
        const PlanLaunch deframe = nrules <= 0 ? PlanLaunch{ HD_K_DEFRAME, nchan, 1, HD_T, HD_LDS_BYTES }
                                   : !events   ? PlanLaunch{ HD_K_DEFRAME_REPAIR, nchan, 1, HD_T, HD_LDS_BYTES_REPAIR }
                                               : PlanLaunch{ HD_K_DEFRAME_EVENTS, nchan, 1, HD_T, HD_LDS_BYTES_REPAIR };
        return launch(deframe, c) && launch(PlanLaunch{ HD_K_SCAN, 1, 1, scan_t, 2 * scan_t * 8 }, c) &&
               launch(PlanLaunch{ HD_K_GATHER, nchan, 1, HD_T, 0 }, c);
    }
};

} // namespace aisx
