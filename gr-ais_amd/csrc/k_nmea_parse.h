// k_nmea_parse.h -- batched NMEA parsing (the device form of aisx_nmea_parse_work, aisx_nmea_parse.cpp, which is its
// specification): a call's text, behind what the handle carried of the calls before, into PDU records, payload octets,
// times and counts, bit for bit what the host form gives call by call.
//
//   count   per tile of text (16 bytes per lane), the line ends in it;
//   scan    one workgroup: the tile counts' exclusive scan, the call's line count, the refusal of a bad call;
//   index   the same tiles again: every line end's position;
//   parse   one wave per line, 64 bytes per pass: ballots find the tag block's end, the commas and '*', an XOR over
//           the wave gives the checksum; a key per line (status, F, f, s, fill, chan, payload length) and the
//           payload's position and the time beside it;
//   group   six kernels over tiles of lines (count, scan, compact) and of sentences (messages, scan, place): the
//           accepted lines compacted by a scan behind the open group's carried sentences; every head checks its
//           followers in that list; message lengths come from the keys alone, a second scan places records and
//           bytes, the kept prefix and the counts; the two scans of tile sums run in one workgroup each;
//   write   one wave per record: lane j forms octet j (j + 64, ...) from the two characters it spans, found through
//           the message's at most nine fragment lengths;
//   carry   one wave: the partial line and the open group's payload characters into the handle's other carry
//           buffers, the state into its other copy.
// What is carried is never text that is parsed again: the partial line has no line end in it, and the open group is
// carried as keys plus payload characters, so nothing is counted twice.  Positions are virtual: p >= 0 is byte p of
// the call's text, -clen <= p < 0 the carried partial line, NP_GBASE + k byte k of the carried group's characters.
// No atomic decides where anything goes.
#pragma once
#include "aisx_common.h"
#include "k_nmea.h"

namespace aisx {

constexpr int NP_T = 256;          // count / index / parse / write kernels
constexpr int NP_SCAN_T = 1024;    // the scans of tile sums: one workgroup each
constexpr int NP_CHUNK = 16;       // bytes of text per lane and tile
constexpr int NP_MAX_GROUPS = 2048;
constexpr int NP_GMAX = 8;         // sentences of an open group at most (F <= 9)
constexpr int NP_LDS_BYTES = 2048;
constexpr long long NP_GBASE = -(1ll << 40);
constexpr int NP_NCNT = 12;

enum { NP_OK = 0, NP_FORMAT, NP_CHECKSUM, NP_CHANNEL, NP_ARMOUR, NP_EMPTY, NP_NSTATUS };
constexpr int NP_M_NLINES = 0, NP_M_BAD = 1, NP_M_CUR = 2, NP_M_NACC = 3, NP_M_STAT = 4, NP_M_N = NP_M_STAT + 8; // meta[]

struct NmpKey {
    unsigned k0;  // status | F << 8 | f << 12 | s << 16 | fill << 24
    int chan;
    int pay_len;  // payload characters
    int text_len; // bytes of the line (for the CARRIED count)
};
AISX_HD int npk_status(const NmpKey& k) { return (int)(k.k0 & 0xffu); }
AISX_HD int npk_F(const NmpKey& k) { return (int)((k.k0 >> 8) & 15u); }
AISX_HD int npk_f(const NmpKey& k) { return (int)((k.k0 >> 12) & 15u); }
AISX_HD int npk_s(const NmpKey& k) { return (int)((k.k0 >> 16) & 0xffu); }
AISX_HD int npk_fill(const NmpKey& k) { return (int)((k.k0 >> 24) & 7u); }

struct NmpState {
    int clen, skip, g, carried; // partial line bytes held; skipping to the next line end; open group's sentences
    long long line_base;        // index of the call's first line end
    NmpKey gkey[NP_GMAX];
    long long gpos[NP_GMAX], gline[NP_GMAX], gtime[NP_GMAX];
};

struct NmpNext { // what the group kernel decided for the carry kernel
    int open, head, plen, skip;
    long long tail_start;
};

struct NmpParams {
    const unsigned char* text;
    const long long* nbytes;
    long long max_bytes;
    int max_lines, max_pdus, max_len, max_line, flags, nchan; // max_len = length_max - 1 payload octets
    const char* desig;          // [nchan][NM_DESIG]
    const unsigned char* dlen;  // [nchan]
    NmpState* st;               // [2]
    unsigned char* lcarry;      // [2][max_line]
    unsigned char* gcarry;      // [2][NP_GMAX * max_line]
    int* tcount;                // [tiles] line ends per tile
    int* toff;                  // [tiles] ... before the tile
    int* meta;                  // [NP_M_N]
    long long* lend;            // [max_lines] position of every line end
    NmpKey* key;                // [max_lines]
    long long* pos;             // [max_lines] payload position
    long long* tm;              // [max_lines] time
    int* cidx;                  // [max_lines] accepted lines in order
    int* mlen;                  // [max_lines + NP_GMAX] octets of the message an entry of the compacted list heads, -1: none
    int* tl;                    // [line tiles] per tile of lines / entries: a count, then where its items go
    long long* tlb;             // [line tiles] ... of bytes
    int* bstat;                 // [NP_MAX_GROUPS][8] per workgroup: lines by status; [6] sentences in messages, [7] length rejects
    HdlcRec* rec;               // [max_pdus]
    int* aux;                   // [max_pdus] index of the message's head in the compacted list
    long long* times;           // [max_pdus]
    unsigned char* bytes;       // [max_pdus * max_len]
    int* count;                 // [NP_NCNT]
    NmpNext* next;
    int ngroups, nwaves;        // grid of the tile kernels; waves in the grid of the wave kernels
};

// the call's byte count, -1 when it lies outside [0, max_bytes]
AISX_HD long long nmp_nbytes(const NmpParams& p)
{
    const long long n = *p.nbytes;
    return n < 0 || n > p.max_bytes ? -1 : n;
}

struct NmpView {
    const unsigned char *text, *lc, *gc;
    int clen;
};
AISX_HD NmpView nmp_view(const NmpParams& p, int cur)
{
    NmpView v;
    v.text = p.text;
    v.lc = p.lcarry + (long)cur * p.max_line;
    v.gc = p.gcarry + (long)cur * NP_GMAX * p.max_line;
    v.clen = p.st[cur].clen;
    return v;
}
AISX_HD unsigned nmp_byte(const NmpView& v, long long pos)
{
    if (pos >= 0)
        return v.text[pos];
    if (pos >= -(long long)v.clen)
        return v.lc[v.clen + pos];
    return v.gc[pos - NP_GBASE];
}

struct alignas(16) NmpU4 {
    unsigned w[4];
};
// bit j: byte pos0 + j is a line end, of the 16 bytes from pos0 (a multiple of 16) that lie below n
AISX_HD unsigned nmp_chunk_mask(const unsigned char* text, long long pos0, long long n, bool aligned)
{
    unsigned m = 0;
    if (pos0 >= n)
        return 0;
    if (aligned && pos0 + NP_CHUNK <= n) {
        const NmpU4 v = *(const NmpU4*)(text + pos0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned x = v.w[q] ^ 0x0a0a0a0au;
            // bit 7 of every byte that is zero (exact: no borrow crosses a byte)
            const unsigned z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
            m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
        }
        return m;
    }
    for (int j = 0; j < NP_CHUNK; j++)
        if (pos0 + j < n && text[pos0 + j] == '\n')
            m |= 1u << j;
    return m;
}

AISX_HD int nmp_popc(unsigned m) { return __builtin_popcount(m); }

template <class Ctx>
AISX_DI long long nmp_wave_incl_sum_ll(Ctx& cx, long long v)
{
    const int l = cx.tid() & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = (long long)cx.shfl_u64((unsigned long long)v, l >= d ? l - d : l);
        if (l >= d)
            v += u;
    }
    return v;
}

// exclusive scan over the workgroup (two barriers); `total` is the workgroup's sum.  lds: one item per wave.
template <class Ctx>
AISX_DI int nmp_block_excl(Ctx& cx, int v, int* lds, int& total)
{
    const int t = cx.tid(), w = t >> 6, l = t & 63, nw = cx.nthreads() >> 6;
    const int incl = nm_wave_incl_sum(cx, v);
    if (l == 63)
        lds[w] = incl;
    cx.sync();
    int pre = 0, tot = 0;
    for (int u = 0; u < nw; u++) {
        const int x = lds[u];
        if (u < w)
            pre += x;
        tot += x;
    }
    cx.sync();
    total = tot;
    return pre + incl - v;
}
template <class Ctx>
AISX_DI long long nmp_block_excl_ll(Ctx& cx, long long v, long long* lds, long long& total)
{
    const int t = cx.tid(), w = t >> 6, l = t & 63, nw = cx.nthreads() >> 6;
    const long long incl = nmp_wave_incl_sum_ll(cx, v);
    if (l == 63)
        lds[w] = incl;
    cx.sync();
    long long pre = 0, tot = 0;
    for (int u = 0; u < nw; u++) {
        const long long x = lds[u];
        if (u < w)
            pre += x;
        tot += x;
    }
    cx.sync();
    total = tot;
    return pre + incl - v;
}

AISX_HD bool nmp_aligned(const NmpParams& p) { return ((unsigned long long)(size_t)p.text & 15ull) == 0; }

// line ends per tile of nthreads * NP_CHUNK bytes
template <class Ctx>
AISX_DI void nmp_count_body(Ctx& cx, const NmpParams& p)
{
    const int t = cx.tid(), T = cx.nthreads();
    long long n = nmp_nbytes(p);
    if (n < 0)
        n = 0;
    const long long tile = (long long)T * NP_CHUNK, ntiles = (n + tile - 1) / tile;
    const bool al = nmp_aligned(p);
    int* lds = (int*)cx.lds();
    for (long long i = cx.bx(); i < ntiles; i += p.ngroups) {
        const int c = nmp_popc(nmp_chunk_mask(p.text, i * tile + (long long)t * NP_CHUNK, n, al));
        int total;
        nmp_block_excl(cx, c, lds, total);
        if (t == 0)
            p.tcount[i] = total;
    }
}

// one workgroup: the tile counts' exclusive scan, the line count, whether the call is refused
template <class Ctx>
AISX_DI void nmp_scan_body(Ctx& cx, const NmpParams& p, int tile_threads)
{
    const int t = cx.tid(), T = cx.nthreads();
    const long long n0 = nmp_nbytes(p), n = n0 < 0 ? 0 : n0;
    const long long tile = (long long)tile_threads * NP_CHUNK, ntiles = (n + tile - 1) / tile;
    int* lds = (int*)cx.lds();
    long long base = 0;
    for (long long i0 = 0; i0 < ntiles; i0 += T) {
        const long long i = i0 + t;
        const int c = i < ntiles ? p.tcount[i] : 0;
        int total;
        const int ex = nmp_block_excl(cx, c, lds, total);
        if (i < ntiles)
            p.toff[i] = (int)(base + ex < 0x7fffffffll ? base + ex : 0x7fffffffll);
        base += total;
    }
    if (t == 0) {
        const bool bad = n0 < 0 || base > p.max_lines;
        p.meta[NP_M_NLINES] = bad ? 0 : (int)base;
        p.meta[NP_M_BAD] = bad ? 1 : 0;
    }
}

// the same tiles again: every line end's position
template <class Ctx>
AISX_DI void nmp_index_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads();
    const long long n = nmp_nbytes(p);
    const long long tile = (long long)T * NP_CHUNK, ntiles = (n + tile - 1) / tile;
    const bool al = nmp_aligned(p);
    int* lds = (int*)cx.lds();
    for (long long i = cx.bx(); i < ntiles; i += p.ngroups) {
        const long long pos0 = i * tile + (long long)t * NP_CHUNK;
        unsigned m = nmp_chunk_mask(p.text, pos0, n, al);
        int total;
        long long o = (long long)p.toff[i] + nmp_block_excl(cx, nmp_popc(m), lds, total);
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            if (o < p.max_lines)
                p.lend[o] = pos0 + j;
            o++;
        }
    }
}

AISX_HD int nmp_hexval(unsigned c)
{
    return c >= '0' && c <= '9' ? (int)c - '0' : c >= 'A' && c <= 'F' ? (int)c - 'A' + 10 : c >= 'a' && c <= 'f' ? (int)c - 'a' + 10 : -1;
}
AISX_HD bool nmp_isdigit(unsigned c) { return c >= '0' && c <= '9'; }

// the time of a tag block's content, m bytes from position ts (wave-uniform result)
template <class Ctx>
AISX_DI long long nmp_tag_time(Ctx& cx, const NmpView& v, long long ts, int m)
{
    const int l = cx.tid() & 63;
    int a = m; // what precedes the last '*'
    for (int base = 0; base < m; base += 64) {
        const int i = base + l;
        const unsigned long long mk = cx.ballot(i < m && nmp_byte(v, ts + i) == '*');
        if (mk)
            a = base + 63 - __builtin_clzll(mk);
    }
    // (the field behind a trailing ',' is empty: no lane need stand for it)
    for (int base = 0; base < a; base += 64) {
        const int i = base + l;
        bool ok = false;
        unsigned long long val = 0;
        if (i < a && (i == 0 || nmp_byte(v, ts + i - 1) == ',') && i + 2 < a && nmp_byte(v, ts + i) == 'c' &&
            nmp_byte(v, ts + i + 1) == ':') {
            int k = i + 2, nd = 0;
            ok = true;
            for (; k < a && nd <= 18; k++, nd++) {
                const unsigned c = nmp_byte(v, ts + k);
                if (c == ',')
                    break;
                ok = ok && nmp_isdigit(c);
                val = val * 10ull + (unsigned long long)(c - '0');
            }
            ok = ok && nd >= 1 && nd <= 18;
        }
        const unsigned long long mk = cx.ballot(ok);
        if (mk)
            return (long long)cx.shfl_u64(val, __builtin_ctzll(mk));
    }
    return -1;
}

// one wave per line
template <class Ctx>
AISX_DI void nmp_parse_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int l = cx.tid() & 63, cur = p.meta[NP_M_CUR], nlines = p.meta[NP_M_NLINES];
    const NmpView v = nmp_view(p, cur);
    const bool skip0 = p.st[cur].skip != 0;
    const bool ref_tail = (p.flags & 1) != 0;
    for (int k = cx.bx() * (cx.nthreads() >> 6) + cx.wave_id(); k < nlines; k += p.nwaves) {
        const long long start = k == 0 ? -(long long)v.clen : p.lend[k - 1] + 1, L = p.lend[k] - start;
        int status = NP_FORMAT, F = 0, f = 0, s = 0, fill = 0, chan = 0, pay_len = 0, Lc = 0;
        long long pay_pos = 0, time = -1;
        do {
            if (L > p.max_line || (k == 0 && skip0))
                break;
            Lc = (int)L;
            if (Lc > 0 && nmp_byte(v, start + Lc - 1) == '\r')
                Lc--;
            if (Lc == 0) {
                status = NP_EMPTY;
                break;
            }
            int b = 0;
            if (nmp_byte(v, start) == '\\') {
                int q = -1;
                for (int base = 1; base < Lc && q < 0; base += 64) {
                    const int i = base + l;
                    const unsigned long long mk = cx.ballot(i < Lc && nmp_byte(v, start + i) == '\\');
                    if (mk)
                        q = base + __builtin_ctzll(mk);
                }
                if (q < 0)
                    break;
                time = nmp_tag_time(cx, v, start + 1, q - 1);
                b = q + 1;
            }
            const long long B = start + b;
            const int n = Lc - b;
            if (n < 18)
                break;
            // the head: "!TTVDM,F,f," and the sequence id
            const unsigned h = l < 13 ? nmp_byte(v, B + l) : 0u;
            const unsigned h11 = (unsigned)cx.shfl_i32((int)h, 11);
            bool okh = true;
            if (l == 0)
                okh = h == '!';
            else if (l == 1 || l == 2)
                okh = (h >= 'A' && h <= 'Z') || nmp_isdigit(h);
            else if (l >= 3 && l <= 5)
                okh = h == (unsigned char)"VDM"[l - 3];
            else if (l == 6 || l == 8 || l == 10)
                okh = h == ',';
            else if (l == 7 || l == 9)
                okh = h >= '1' && h <= '9';
            else if (l == 11)
                okh = h == ',' || nmp_isdigit(h);
            else if (l == 12)
                okh = h11 == ',' || h == ',';
            const bool bad_head = cx.ballot(!okh) != 0;
            F = cx.shfl_i32((int)h, 7) - '0';
            f = cx.shfl_i32((int)h, 9) - '0';
            if (bad_head || f > F)
                break;
            s = h11 == ',' ? 0 : (int)h11;
            const int c0 = s ? 13 : 12;
            // the channel designator: up to 16 bytes before the next ','
            const int ic = c0 + l;
            const unsigned cc = l < 17 && ic < n ? nmp_byte(v, B + ic) : 0u;
            const unsigned long long mcomma = cx.ballot(l < 17 && ic < n && cc == ',');
            if (!mcomma)
                break;
            const int cl = __builtin_ctzll(mcomma);
            if (cx.ballot(l < cl && cc == '*'))
                break;
            const int p0 = c0 + cl + 1, p1 = n - 5;
            if (p1 < p0)
                break;
            // the tail: ",fill*HH"
            const unsigned tl = l < 5 ? nmp_byte(v, B + p1 + l) : 0u;
            bool okt = true;
            if (l == 0)
                okt = tl == ',';
            else if (l == 1)
                okt = tl >= '0' && tl <= '5';
            else if (l == 2)
                okt = tl == '*';
            else if (l == 3 || l == 4)
                okt = nmp_hexval(tl) >= 0;
            if (cx.ballot(!okt))
                break;
            fill = cx.shfl_i32((int)tl, 1) - '0';
            const int hh = nmp_hexval((unsigned)cx.shfl_i32((int)tl, 3)) * 16 + nmp_hexval((unsigned)cx.shfl_i32((int)tl, 4));
            pay_len = p1 - p0;
            pay_pos = B + p0;
            const bool tail_zero = ref_tail && f == F && fill > 0 && pay_len > 0;
            // the checksum over [1, n - 3), and the payload's bytes on the way
            unsigned x = 0;
            bool comma = false, unarm = false;
            for (int base = 1; base < n - 3; base += 64) {
                const int i = base + l;
                if (i < n - 3) {
                    const unsigned c = nmp_byte(v, B + i);
                    x ^= c;
                    if (i >= p0 && i < p1) {
                        comma = comma || c == ',';
                        if (!(tail_zero && i == p1 - 1))
                            unarm = unarm || !((c >= 48 && c <= 87) || (c >= 96 && c <= 119));
                    }
                }
            }
            for (int m = 32; m >= 1; m >>= 1)
                x ^= (unsigned)cx.shfl_xor_i32((int)x, m);
            const bool any_comma = cx.ballot(comma) != 0, any_unarm = cx.ballot(unarm) != 0;
            if (any_comma)
                break;
            if ((int)x != hh) {
                status = NP_CHECKSUM;
                break;
            }
            // the designator: the smallest matching index
            chan = -1;
            for (int base = 0; base < p.nchan && chan < 0; base += 64) {
                const int c = base + l;
                bool eq = c < p.nchan && p.dlen[c] == cl;
                if (eq)
                    for (int j = 0; j < cl; j++)
                        eq = eq && (unsigned char)p.desig[(long)c * NM_DESIG + j] == nmp_byte(v, B + c0 + j);
                const unsigned long long mk = cx.ballot(eq);
                if (mk)
                    chan = base + __builtin_ctzll(mk);
            }
            if (chan < 0) {
                status = NP_CHANNEL;
                break;
            }
            status = any_unarm ? NP_ARMOUR : NP_OK;
        } while (false);
        if (l == 0) {
            NmpKey key;
            key.k0 = (unsigned)status | (unsigned)F << 8 | (unsigned)f << 12 | (unsigned)s << 16 | (unsigned)fill << 24;
            key.chan = chan;
            key.pay_len = pay_len;
            key.text_len = Lc;
            p.key[k] = key;
            p.pos[k] = pay_pos;
            p.tm[k] = time;
        }
    }
}

// entry i of the compacted list: the g carried sentences of the open group, then the call's accepted lines
struct NmpEntries {
    const NmpState* s;
    const NmpParams* p;
    int g;
};
AISX_HD NmpKey nmp_ekey(const NmpEntries& e, int i) { return i < e.g ? e.s->gkey[i] : e.p->key[e.p->cidx[i - e.g]]; }
AISX_HD long long nmp_epos(const NmpEntries& e, int i) { return i < e.g ? e.s->gpos[i] : e.p->pos[e.p->cidx[i - e.g]]; }
AISX_HD long long nmp_etime(const NmpEntries& e, int i) { return i < e.g ? e.s->gtime[i] : e.p->tm[e.p->cidx[i - e.g]]; }
AISX_HD long long nmp_eline(const NmpEntries& e, int i)
{
    return i < e.g ? e.s->gline[i] : e.s->line_base + e.p->cidx[i - e.g];
}
AISX_HD bool nmp_follows(const NmpKey& h, const NmpKey& k, int j) // k is sentence j + 1 of the group h heads
{
    return npk_f(k) == j + 1 && npk_F(k) == npk_F(h) && npk_s(k) == npk_s(h) && k.chan == h.chan;
}

// ---- the group stage: six kernels over tiles of nthreads lines / sentences, one item per thread -------------------
// the workgroup's sum of v (two barriers)
template <class Ctx>
AISX_DI int nmp_block_sum(Ctx& cx, int v, int* lds)
{
    int total;
    nmp_block_excl(cx, v, lds, total);
    return total;
}

// gcount: accepted lines per tile; the lines of every status per workgroup
template <class Ctx>
AISX_DI void nmp_gcount_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads(), nlines = p.meta[NP_M_NLINES];
    const int ntiles = (nlines + T - 1) / T;
    int* lds = (int*)cx.lds();
    int cnt[NP_NSTATUS + 1];
    for (int q = 0; q <= NP_NSTATUS; q++)
        cnt[q] = 0;
    for (int i = cx.bx(); i < ntiles; i += p.ngroups) {
        const int k = i * T + t;
        const int st = k < nlines ? npk_status(p.key[k]) : NP_NSTATUS;
        cnt[st]++;
        const int total = nmp_block_sum(cx, st == NP_OK ? 1 : 0, lds);
        if (t == 0)
            p.tl[i] = total;
    }
    for (int q = 0; q < NP_NSTATUS; q++) {
        const int total = nmp_block_sum(cx, cnt[q], lds);
        if (t == 0)
            p.bstat[cx.bx() * 8 + q] = total;
    }
}

// gscan1, one workgroup: where every tile's accepted lines go; the call's accepted lines and status counts
template <class Ctx>
AISX_DI void nmp_gscan1_body(Ctx& cx, const NmpParams& p, int tile_threads)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads(), nlines = p.meta[NP_M_NLINES];
    const int ntiles = (nlines + tile_threads - 1) / tile_threads;
    int* lds = (int*)cx.lds();
    int base = 0;
    for (int i0 = 0; i0 < ntiles; i0 += T) {
        const int i = i0 + t;
        const int c = i < ntiles ? p.tl[i] : 0;
        int total;
        const int ex = nmp_block_excl(cx, c, lds, total);
        if (i < ntiles)
            p.tl[i] = base + ex;
        base += total;
    }
    const int nb = ntiles < p.ngroups ? ntiles : p.ngroups; // workgroups that had a tile
    for (int q = 0; q < NP_NSTATUS; q++) {
        int x = 0;
        for (int b = t; b < nb; b += T)
            x += p.bstat[b * 8 + q];
        const int total = nmp_block_sum(cx, x, lds);
        if (t == 0)
            p.meta[NP_M_STAT + q] = total;
    }
    if (t == 0)
        p.meta[NP_M_NACC] = base;
}

// gcompact: the accepted lines in order
template <class Ctx>
AISX_DI void nmp_gcompact_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads(), nlines = p.meta[NP_M_NLINES];
    const int ntiles = (nlines + T - 1) / T;
    int* lds = (int*)cx.lds();
    for (int i = cx.bx(); i < ntiles; i += p.ngroups) {
        const int k = i * T + t;
        const bool acc = k < nlines && npk_status(p.key[k]) == NP_OK;
        int total;
        const int ex = nmp_block_excl(cx, acc ? 1 : 0, lds, total);
        if (acc)
            p.cidx[p.tl[i] + ex] = k;
    }
}

// gmsg: every head checks its followers in the compacted list; a message's length from the keys alone
template <class Ctx>
AISX_DI void nmp_gmsg_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads();
    const NmpState& S = p.st[p.meta[NP_M_CUR]];
    const NmpEntries E{ &S, &p, S.g };
    const int n = S.g + p.meta[NP_M_NACC], ntiles = (n + T - 1) / T;
    int* lds = (int*)cx.lds();
    long long* ldsl = (long long*)(lds + 64);
    int nsent = 0, nrejlen = 0;
    for (int tile = cx.bx(); tile < ntiles; tile += p.ngroups) {
        const int i = tile * T + t;
        int len = -1; // (no record)
        if (i < n) {
            const NmpKey h = nmp_ekey(E, i);
            const int F = npk_F(h);
            if (npk_f(h) == 1 && i + F <= n) {
                bool ok = true;
                long P = h.pay_len;
                int fill = npk_fill(h);
                for (int q = 1; q < F && ok; q++) {
                    const NmpKey kq = nmp_ekey(E, i + q);
                    ok = nmp_follows(h, kq, q);
                    P += kq.pay_len;
                    fill = npk_fill(kq);
                }
                if (ok) {
                    nsent += F;
                    const long nbits = 6 * P - fill;
                    const int ln = (int)((nbits + 7) >> 3);
                    if (nbits > 0 && ln <= p.max_len)
                        len = ln;
                    else
                        nrejlen++;
                }
            }
            p.mlen[i] = len;
        }
        int tot;
        long long totl;
        nmp_block_excl(cx, len >= 0 ? 1 : 0, lds, tot);
        nmp_block_excl_ll(cx, len >= 0 ? (long long)len : 0ll, ldsl, totl);
        if (t == 0) {
            p.tl[tile] = tot;
            p.tlb[tile] = totl;
        }
    }
    const int a = nmp_block_sum(cx, nsent, lds), b = nmp_block_sum(cx, nrejlen, lds);
    if (t == 0) {
        p.bstat[cx.bx() * 8 + 6] = a;
        p.bstat[cx.bx() * 8 + 7] = b;
    }
}

// gscan2, one workgroup: where every tile's records and bytes go; the counts; what is carried
template <class Ctx>
AISX_DI void nmp_gscan2_body(Ctx& cx, const NmpParams& p, int tile_threads)
{
    const int t = cx.tid(), T = cx.nthreads();
    const int cur = p.meta[NP_M_CUR];
    const NmpState& S = p.st[cur];
    if (p.meta[NP_M_BAD]) {
        if (t == 0) {
            for (int k = 0; k < NP_NCNT; k++)
                p.count[k] = k == 2 ? 1 : k == NP_NCNT - 1 ? S.carried : 0;
            p.next->open = 0;
        }
        return;
    }
    const NmpEntries E{ &S, &p, S.g };
    const int nlines = p.meta[NP_M_NLINES], n = S.g + p.meta[NP_M_NACC], ntiles = (n + tile_threads - 1) / tile_threads;
    int* lds = (int*)cx.lds();
    long long* ldsl = (long long*)(lds + 64);
    int found = 0;
    long long nbyte = 0;
    for (int i0 = 0; i0 < ntiles; i0 += T) {
        const int i = i0 + t;
        int tot;
        long long totl;
        const int ex = nmp_block_excl(cx, i < ntiles ? p.tl[i] : 0, lds, tot);
        const long long exl = nmp_block_excl_ll(cx, i < ntiles ? p.tlb[i] : 0ll, ldsl, totl);
        if (i < ntiles) {
            p.tl[i] = found + ex;
            p.tlb[i] = nbyte + exl;
        }
        found += tot;
        nbyte += totl;
    }
    const int nb = ntiles < p.ngroups ? ntiles : p.ngroups;
    int x6 = 0, x7 = 0;
    for (int b = t; b < nb; b += T) {
        x6 += p.bstat[b * 8 + 6];
        x7 += p.bstat[b * 8 + 7];
    }
    const int nsent = nmp_block_sum(cx, x6, lds), nrejlen = nmp_block_sum(cx, x7, lds);
    if (t == 0) {
        // the group still open behind the last sentence
        int open = 0, head = 0;
        if (n > 0) {
            const NmpKey last = nmp_ekey(E, n - 1);
            const int fl = npk_f(last), h0 = n - fl;
            if (fl < npk_F(last) && h0 >= 0) {
                const NmpKey h = nmp_ekey(E, h0);
                bool ok = npk_f(h) == 1 && npk_F(h) == npk_F(last);
                for (int j = 1; j < fl && ok; j++)
                    ok = nmp_follows(h, nmp_ekey(E, h0 + j), j);
                if (ok) {
                    open = fl;
                    head = h0;
                }
            }
        }
        // the partial line behind the last line end
        const long long nbt = nmp_nbytes(p);
        const long long tail_start = nlines > 0 ? p.lend[nlines - 1] + 1 : -(long long)S.clen;
        long long plen = nbt - tail_start;
        int skip = nlines > 0 ? 0 : S.skip;
        if (skip || plen > p.max_line) {
            skip = 1;
            plen = 0;
        }
        int carried = (int)plen;
        for (int j = 0; j < open; j++)
            carried += nmp_ekey(E, head + j).text_len;
        NmpNext nx;
        nx.open = open;
        nx.head = head;
        nx.plen = (int)plen;
        nx.skip = skip;
        nx.tail_start = tail_start;
        *p.next = nx;
        p.count[0] = found;
        p.count[1] = found < p.max_pdus ? found : p.max_pdus;
        p.count[3] = nlines;
        p.count[4] = p.meta[NP_M_STAT + NP_OK];
        p.count[5] = p.meta[NP_M_STAT + NP_FORMAT];
        p.count[6] = p.meta[NP_M_STAT + NP_CHECKSUM];
        p.count[7] = p.meta[NP_M_STAT + NP_CHANNEL];
        p.count[8] = p.meta[NP_M_STAT + NP_ARMOUR];
        p.count[9] = n - nsent - open;
        p.count[10] = nrejlen;
        p.count[11] = carried;
    }
}

// gplace: the records of the messages, in order
template <class Ctx>
AISX_DI void nmp_gplace_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int t = cx.tid(), T = cx.nthreads();
    const NmpState& S = p.st[p.meta[NP_M_CUR]];
    const NmpEntries E{ &S, &p, S.g };
    const int n = S.g + p.meta[NP_M_NACC], ntiles = (n + T - 1) / T;
    int* lds = (int*)cx.lds();
    long long* ldsl = (long long*)(lds + 64);
    for (int tile = cx.bx(); tile < ntiles; tile += p.ngroups) {
        const int i = tile * T + t;
        const int len = i < n ? p.mlen[i] : -1;
        int tot;
        long long totl;
        const int idx = p.tl[tile] + nmp_block_excl(cx, len >= 0 ? 1 : 0, lds, tot);
        const long long off = p.tlb[tile] + nmp_block_excl_ll(cx, len >= 0 ? (long long)len : 0ll, ldsl, totl);
        if (len >= 0 && idx < p.max_pdus) {
            const NmpKey h = nmp_ekey(E, i);
            HdlcRec r;
            r.end_bit = (unsigned long long)nmp_eline(E, i + npk_F(h) - 1);
            r.offset = off;
            r.chan = h.chan;
            r.len = len;
            p.rec[idx] = r;
            p.aux[idx] = i;
            p.times[idx] = nmp_etime(E, i);
        }
    }
}

// one wave per record kept: lane j forms octets j, j + 64, ...
template <class Ctx>
AISX_DI void nmp_write_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int l = cx.tid() & 63, cur = p.meta[NP_M_CUR];
    const NmpState& S = p.st[cur];
    const NmpView v = nmp_view(p, cur);
    const NmpEntries E{ &S, &p, S.g };
    const int kept = p.count[1];
    const bool ref_tail = (p.flags & 1) != 0;
    for (int r = cx.bx() * (cx.nthreads() >> 6) + cx.wave_id(); r < kept; r += p.nwaves) {
        const HdlcRec rec = p.rec[r];
        const int i = p.aux[r];
        const int F = npk_F(nmp_ekey(E, i));
        int pl[9];
        long long pp[9];
        long P = 0;
        int fill = 0;
        bool tz = false;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            pl[q] = 0;
            pp[q] = 0;
            if (q < F) {
                const NmpKey k = nmp_ekey(E, i + q);
                pl[q] = k.pay_len;
                pp[q] = nmp_epos(E, i + q);
                P += k.pay_len;
                fill = npk_fill(k);
                tz = ref_tail && npk_f(k) == npk_F(k) && fill > 0 && k.pay_len > 0; // (of the last sentence)
            }
        }
        const long nbits = 6 * P - fill;
        auto val = [&](long ci) -> unsigned {
            if (ci >= P)
                return 0u;
            if (tz && ci == P - 1)
                return 0u;
            long c = ci;
            unsigned ch = 48;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                if (c >= 0 && c < pl[q])
                    ch = nmp_byte(v, pp[q] + c);
                c -= pl[q];
            }
            unsigned x = ch - 48u;
            if (x > 40u)
                x -= 8u;
            return x & 63u;
        };
        for (int j = l; j < rec.len; j += 64) {
            const long bit0 = 8l * j, ci = bit0 / 6;
            const int sh = (int)(bit0 % 6);
            const unsigned wv = val(ci) << 6 | val(ci + 1);
            unsigned o = (wv >> (4 - sh)) & 0xffu;
            const long held = nbits - bit0; // bits of this octet the message holds
            if (held < 8)
                o &= 0xffu << (8 - held);
            p.bytes[rec.offset + j] = (unsigned char)o;
        }
    }
}

// one wave: what the next call starts from, into the other copy of the state
template <class Ctx>
AISX_DI void nmp_carry_body(Ctx& cx, const NmpParams& p)
{
    if (p.meta[NP_M_BAD])
        return;
    const int l = cx.tid() & 63, cur = p.meta[NP_M_CUR], nc = cur ^ 1;
    const NmpState& S = p.st[cur];
    const NmpView v = nmp_view(p, cur);
    const NmpEntries E{ &S, &p, S.g };
    const NmpNext nx = *p.next;
    NmpState& D = p.st[nc];
    unsigned char* lc = p.lcarry + (long)nc * p.max_line;
    unsigned char* gc = p.gcarry + (long)nc * NP_GMAX * p.max_line;
    for (int i = l; i < nx.plen; i += 64)
        lc[i] = (unsigned char)nmp_byte(v, nx.tail_start + i);
    int off = 0;
    for (int q = 0; q < nx.open; q++) {
        const NmpKey k = nmp_ekey(E, nx.head + q);
        const long long src = nmp_epos(E, nx.head + q);
        for (int i = l; i < k.pay_len; i += 64)
            gc[off + i] = (unsigned char)nmp_byte(v, src + i);
        if (l == 0) {
            D.gkey[q] = k;
            D.gpos[q] = NP_GBASE + off;
            D.gline[q] = nmp_eline(E, nx.head + q);
            D.gtime[q] = nmp_etime(E, nx.head + q);
        }
        off += k.pay_len;
    }
    if (l == 0) {
        D.clen = nx.plen;
        D.skip = nx.skip;
        D.g = nx.open;
        D.carried = p.count[11];
        D.line_base = S.line_base + p.meta[NP_M_NLINES];
    }
    cx.wave_sync();
    if (l == 0)
        p.meta[NP_M_CUR] = nc;
}

// ------------------------------------------------------------------
// The launch plan of aisx_nmea_parse_batch_* (host only): the argument checks, the derived sizes, the buffers and the
// per-call sequence.  aisx_nmea_parse.hip runs it on device memory, tests/emul_nmea_parse on host memory.
// ------------------------------------------------------------------
enum {
    NP_K_COUNT, NP_K_SCAN, NP_K_INDEX, NP_K_PARSE, NP_K_GCOUNT, NP_K_GSCAN1, NP_K_GCOMPACT, NP_K_GMSG, NP_K_GSCAN2, NP_K_GPLACE,
    NP_K_WRITE, NP_K_CARRY, NP_NKERNELS
};

struct NmpBufs { // a handle's buffers, sized by the NmpPlan members of the same names (NmpParams says what they hold)
    const char* desig;
    const unsigned char* dlen;
    NmpState* st;
    unsigned char *lcarry, *gcarry;
    int *tcount, *toff, *meta;
    long long* lend;
    NmpKey* key;
    long long *pos, *tm;
    int *cidx, *mlen, *tl;
    long long* tlb;
    int* bstat;
    HdlcRec* rec;
    int* aux;
    long long* times;
    unsigned char* bytes;
    int* count;
    NmpNext* next;
};

struct NmpPlan {
    int nchan, lmax, max_line, flags, max_lines, max_pdus, threads, scan_t;
    long long max_bytes, ntiles, nlt; // tiles of text; tiles of lines / sentences
    int tile_groups, line_groups, pdu_groups, ltile_groups;
    std::vector<char> desig_host;         // what the handle's desig and dlen buffers hold
    std::vector<unsigned char> dlen_host;
    PlanBuf desig, dlen, st, lcarry, gcarry, tcount, toff, meta, lend, key, pos, tm, cidx, mlen, tl, tlb, bstat, rec, aux, times,
        bytes, count, next;

    // the argument check of aisx_nmea_parse_batch_create but the designators' own (nm_bad_designator): nullptr when it
    // passes (the one flag there is: AISX_NMEA_PARSE_REF_TAIL = 1)
    static const char* check(const char* const* designators, int nchan, int length_max, int max_line, int flags, long max_bytes,
                             int max_lines, int max_pdus)
    {
        static_assert(NM_MAX_OCTETS == 1024, "the bound in the text below");
        if (!designators || nchan < 1 || length_max < 2 || length_max > NM_MAX_OCTETS || max_line < 64 || max_line > 4096 ||
            (flags & ~1) || max_bytes < 1 || max_bytes > (1l << 30) || max_lines < 1 || max_lines > (1 << 26) || max_pdus < 1)
            return "need designators, nchan >= 1, 2 <= length_max <= 1024, 64 <= max_line <= 4096, flags 0 or 1, "
                   "1 <= max_bytes <= 2^30, 1 <= max_lines <= 2^26, max_pdus >= 1";
        return nullptr;
    }
    // threads_: of a tile / wave kernel's workgroup; scan_t_: of a scan's one workgroup; max_groups: workgroups at most
    NmpPlan(const char* const* designators, int nchan_, int length_max, int max_line_, int flags_, long max_bytes_, int max_lines_,
            int max_pdus_, int threads_ = NP_T, int scan_t_ = NP_SCAN_T, int max_groups = NP_MAX_GROUPS)
        : nchan(nchan_), lmax(length_max), max_line(max_line_), flags(flags_), max_lines(max_lines_), max_pdus(max_pdus_),
          threads(threads_), scan_t(scan_t_), max_bytes(max_bytes_)
    {
        auto groups = [max_groups](long long items, int per_group) {
            const long long g = (items + per_group - 1) / per_group;
            return (int)(g < 1 ? 1 : g < max_groups ? g : max_groups);
        };
        ntiles = (max_bytes + threads * NP_CHUNK - 1) / (threads * NP_CHUNK);
        tile_groups = groups(ntiles, 1);
        line_groups = groups(max_lines, threads / 64);
        pdu_groups = groups(max_pdus, threads / 64);
        nlt = ((long long)max_lines + NP_GMAX + threads - 1) / threads;
        ltile_groups = groups(nlt, 1);
        nm_pack_designators(designators, nchan, desig_host, dlen_host);
        const size_t nl = (size_t)max_lines, np = (size_t)max_pdus;
        desig = { desig_host.size(), false };
        dlen = { dlen_host.size(), false };
        st = { 2, true };
        lcarry = { 2 * (size_t)max_line, true };
        gcarry = { 2 * (size_t)NP_GMAX * max_line, true };
        tcount = toff = { (size_t)ntiles, false };
        meta = { NP_M_N, true };
        lend = key = pos = tm = cidx = { nl, false };
        mlen = { nl + NP_GMAX, false };
        tl = tlb = { (size_t)nlt, false };
        bstat = { (size_t)max_groups * 8, true };
        rec = aux = times = { np, false };
        bytes = { np * (size_t)(length_max - 1), false };
        count = { NP_NCNT, true };
        next = { 1, true };
    }

    // a call: twelve launches on four grids; the tile kernels read their grid from ngroups, the wave kernels theirs from
    // nwaves, and both are set for the launches that read them
    template <class Launch>
    bool process(const NmpBufs& b, const unsigned char* text, const long long* nbytes, Launch&& launch) const
    {
        NmpParams p;
        p.text = text;
        p.nbytes = nbytes;
        p.max_bytes = max_bytes;
        p.max_lines = max_lines;
        p.max_pdus = max_pdus;
        p.max_len = lmax - 1;
        p.max_line = max_line;
        p.flags = flags;
        p.nchan = nchan;
        p.desig = b.desig;
        p.dlen = b.dlen;
        p.st = b.st;
        p.lcarry = b.lcarry;
        p.gcarry = b.gcarry;
        p.tcount = b.tcount;
        p.toff = b.toff;
        p.meta = b.meta;
        p.lend = b.lend;
        p.key = b.key;
        p.pos = b.pos;
        p.tm = b.tm;
        p.cidx = b.cidx;
        p.mlen = b.mlen;
        p.tl = b.tl;
        p.tlb = b.tlb;
        p.bstat = b.bstat;
        p.rec = b.rec;
        p.aux = b.aux;
        p.times = b.times;
        p.bytes = b.bytes;
        p.count = b.count;
        p.next = b.next;
        auto on = [&](int kernel, int groups, int t) { return launch(PlanLaunch{ kernel, groups, 1, t, NP_LDS_BYTES }, p); };
        p.ngroups = tile_groups;
        p.nwaves = line_groups * (threads / 64);
        if (!on(NP_K_COUNT, tile_groups, threads) || !on(NP_K_SCAN, 1, scan_t) || !on(NP_K_INDEX, tile_groups, threads) ||
            !on(NP_K_PARSE, line_groups, threads))
            return false;
        p.ngroups = ltile_groups;
        if (!on(NP_K_GCOUNT, ltile_groups, threads) || !on(NP_K_GSCAN1, 1, scan_t) || !on(NP_K_GCOMPACT, ltile_groups, threads) ||
            !on(NP_K_GMSG, ltile_groups, threads) || !on(NP_K_GSCAN2, 1, scan_t) || !on(NP_K_GPLACE, ltile_groups, threads))
            return false;
        p.nwaves = pdu_groups * (threads / 64);
        return on(NP_K_WRITE, pdu_groups, threads) && on(NP_K_CARRY, 1, 64);
    }
};

} // namespace aisx
