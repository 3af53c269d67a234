// aisx_nmea_parse.cpp -- !AIVDM text back into PDUs on the host (include/aisx.h, aisx_nmea_parse_*): the specification
// of the batched device form (k_nmea_parse.h).  Plain C++, no device code and nothing that needs HIP: a byte stream
// cut into calls anywhere gives the same records, bytes, times and summed counts however it is cut.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/aisx.h"

namespace {

struct Sentence {
    int F, f, s, chan, fill;
    int64_t time, line;
    bool tail_zero;      // REF_TAIL: the last payload character counts as six zero bits
    int text_len;        // bytes of the line, for CARRIED
    std::string payload;
};

// the time of a tag block's content: everything from its last '*' on dropped, the first field "c:" + 1..18 digits
int64_t tag_time(const char* t, int m)
{
    int a = m;
    for (int i = m - 1; i >= 0; i--)
        if (t[i] == '*') {
            a = i;
            break;
        }
    for (int i = 0; i <= a;) {
        int e = i;
        while (e < a && t[e] != ',')
            e++;
        const int nd = e - i - 2;
        if (nd >= 1 && nd <= 18 && t[i] == 'c' && t[i + 1] == ':') {
            uint64_t v = 0; // (18 digits fit; unsigned, so that bytes that are no digits cannot overflow it)
            bool ok = true;
            for (int k = i + 2; k < e && ok; k++) {
                ok = t[k] >= '0' && t[k] <= '9';
                v = v * 10u + (uint64_t)(unsigned char)(t[k] - '0');
            }
            if (ok)
                return (int64_t)v;
        }
        i = e + 1;
    }
    return -1;
}

int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'A' && c <= 'F' ? c - 'A' + 10 : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

} // namespace

struct aisx_nmea_parse {
    std::vector<std::string> desig;
    int length_max = 0, max_line = 0, flags = 0;
    std::string partial; // the line that has not ended yet (at most max_line bytes)
    bool skipping = false; // ... which is already longer than max_line: its bytes are dropped up to the line end
    int64_t line = 0;    // index of the next line end
    std::vector<Sentence> group; // the open group's sentences so far

    // per call
    int* cnt = nullptr;
    aisx_pdu* pdus = nullptr;
    int pdu_cap = 0;
    uint8_t* bytes = nullptr;
    long bytes_cap = 0;
    int64_t* times = nullptr;
    int64_t next_offset = 0;
    bool full = false;

    void drop_group()
    {
        cnt[AISX_NMEAP_REJ_FRAGMENT] += (int)group.size();
        group.clear();
    }

    void message(const Sentence* s, int F)
    {
        long P = 0;
        for (int k = 0; k < F; k++)
            P += (long)s[k].payload.size();
        const long nbits = 6 * P - s[F - 1].fill, len = (nbits + 7) / 8;
        if (nbits <= 0 || len > length_max - 1) {
            cnt[AISX_NMEAP_REJ_LENGTH]++;
            return;
        }
        const int k = cnt[AISX_NMEAP_FOUND]++;
        const int64_t off = next_offset;
        next_offset += len;
        if (full || k >= pdu_cap || off + len > bytes_cap) {
            full = true; // (a prefix is kept)
            return;
        }
        cnt[AISX_NMEAP_KEPT]++;
        uint8_t* o = bytes + off;
        memset(o, 0, (size_t)len);
        long bit = 0;
        for (int q = 0; q < F; q++) {
            const std::string& pl = s[q].payload;
            for (size_t i = 0; i < pl.size(); i++, bit += 6) {
                int v = (unsigned char)pl[i] - 48;
                if (v > 40)
                    v -= 8;
                if (s[q].tail_zero && i + 1 == pl.size())
                    v = 0;
                for (int b = 0; b < 6; b++)
                    if (bit + b < nbits && ((v >> (5 - b)) & 1))
                        o[(bit + b) >> 3] |= (uint8_t)(0x80 >> ((bit + b) & 7));
            }
        }
        pdus[k].end_bit = (uint64_t)s[F - 1].line;
        pdus[k].offset = off;
        pdus[k].chan = s[0].chan;
        pdus[k].len = (int32_t)len;
        if (times)
            times[k] = s[0].time;
    }

    void accepted(Sentence&& x)
    {
        cnt[AISX_NMEAP_SENTENCES]++;
        if (!group.empty()) {
            const int F = group[0].F;
            if (x.f == (int)group.size() + 1 && x.F == F && x.s == group[0].s && x.chan == group[0].chan) {
                group.push_back(std::move(x));
                if ((int)group.size() == F) {
                    message(group.data(), F);
                    group.clear();
                }
                return;
            }
            drop_group();
        }
        if (x.F == 1)
            message(&x, 1);
        else if (x.f == 1)
            group.push_back(std::move(x));
        else
            cnt[AISX_NMEAP_REJ_FRAGMENT]++;
    }

    // one whole line of L bytes, the '\r' included and the '\n' not
    void line_end(const char* p, long L, bool overlong)
    {
        const int64_t idx = line++;
        cnt[AISX_NMEAP_LINES]++;
        if (overlong || L > max_line) {
            cnt[AISX_NMEAP_REJ_FORMAT]++;
            return;
        }
        int Lc = (int)L;
        if (Lc > 0 && p[Lc - 1] == '\r')
            Lc--;
        if (Lc == 0)
            return;
        int b = 0;
        int64_t time = -1;
        if (p[0] == '\\') {
            const char* q = (const char*)memchr(p + 1, '\\', (size_t)(Lc - 1));
            if (!q) {
                cnt[AISX_NMEAP_REJ_FORMAT]++;
                return;
            }
            time = tag_time(p + 1, (int)(q - p - 1));
            b = (int)(q - p) + 1;
        }
        const char* B = p + b;
        const int n = Lc - b;
        auto alnum = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9'); };
        auto dig19 = [](char c) { return c >= '1' && c <= '9'; };
        bool ok = n >= 18 && B[0] == '!' && alnum(B[1]) && alnum(B[2]) && B[3] == 'V' && B[4] == 'D' && B[5] == 'M' && B[6] == ',' &&
                  dig19(B[7]) && B[8] == ',' && dig19(B[9]) && B[9] <= B[7] && B[10] == ',';
        int s = 0, c0 = 12, c1 = -1;
        if (ok) {
            if (B[11] == ',')
                ;
            else if (B[11] >= '0' && B[11] <= '9' && B[12] == ',')
                s = B[11], c0 = 13;
            else
                ok = false;
        }
        if (ok) {
            for (int i = c0; i < n && i <= c0 + 16 && c1 < 0; i++) {
                if (B[i] == '*')
                    break;
                if (B[i] == ',')
                    c1 = i;
            }
            ok = c1 >= 0;
        }
        const int p0 = c1 + 1, p1 = n - 5;
        ok = ok && p1 >= p0 && B[p1] == ',' && !memchr(B + p0, ',', (size_t)(p1 - p0)) && B[n - 4] >= '0' && B[n - 4] <= '5' &&
             B[n - 3] == '*' && hexval(B[n - 2]) >= 0 && hexval(B[n - 1]) >= 0;
        if (!ok) {
            cnt[AISX_NMEAP_REJ_FORMAT]++;
            return;
        }
        int x = 0;
        for (int i = 1; i < n - 3; i++)
            x ^= (unsigned char)B[i];
        if (x != hexval(B[n - 2]) * 16 + hexval(B[n - 1])) {
            cnt[AISX_NMEAP_REJ_CHECKSUM]++;
            return;
        }
        int chan = -1;
        for (size_t c = 0; c < desig.size() && chan < 0; c++)
            if ((int)desig[c].size() == c1 - c0 && !memcmp(desig[c].data(), B + c0, (size_t)(c1 - c0)))
                chan = (int)c;
        if (chan < 0) {
            cnt[AISX_NMEAP_REJ_CHANNEL]++;
            return;
        }
        Sentence sn;
        sn.F = B[7] - '0';
        sn.f = B[9] - '0';
        sn.s = s;
        sn.chan = chan;
        sn.fill = B[n - 4] - '0';
        sn.time = time;
        sn.line = idx;
        sn.text_len = Lc;
        sn.tail_zero = (flags & AISX_NMEA_PARSE_REF_TAIL) && sn.f == sn.F && sn.fill > 0 && p1 > p0;
        for (int i = p0; i < p1 - (sn.tail_zero ? 1 : 0); i++) {
            const unsigned char c = (unsigned char)B[i];
            if (!((c >= 48 && c <= 87) || (c >= 96 && c <= 119))) {
                cnt[AISX_NMEAP_REJ_ARMOUR]++;
                return;
            }
        }
        sn.payload.assign(B + p0, (size_t)(p1 - p0));
        accepted(std::move(sn));
    }
};

extern "C" int aisx_nmea_parse_create(aisx_nmea_parse** out, const char* const* designators, int nchan, int length_max,
                                      int max_line, int flags)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (!designators || nchan < 1 || length_max < 2 || length_max > 1024 || max_line < 64 || max_line > 4096 ||
        (flags & ~AISX_NMEA_PARSE_REF_TAIL))
        return AISX_ERR_INVALID;
    for (int c = 0; c < nchan; c++)
        if (!designators[c] || strnlen(designators[c], 17) > 16)
            return AISX_ERR_INVALID;
    aisx_nmea_parse* h = new aisx_nmea_parse();
    for (int c = 0; c < nchan; c++)
        h->desig.emplace_back(designators[c]);
    h->length_max = length_max;
    h->max_line = max_line;
    h->flags = flags;
    *out = h;
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_destroy(aisx_nmea_parse* h)
{
    delete h;
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_reset(aisx_nmea_parse* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    h->partial.clear();
    h->skipping = false;
    h->line = 0;
    h->group.clear();
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_work(aisx_nmea_parse* h, const char* text, long nbytes, aisx_pdu* pdus, int pdu_cap,
                                    uint8_t* bytes, long bytes_cap, int64_t* times, int* counts)
{
    if (!h || !counts || nbytes < 0 || pdu_cap < 0 || bytes_cap < 0 || (nbytes > 0 && !text) || (pdu_cap > 0 && !pdus) ||
        (bytes_cap > 0 && !bytes))
        return AISX_ERR_INVALID;
    for (int k = 0; k < AISX_NMEAP_NCNT; k++)
        counts[k] = 0;
    h->cnt = counts;
    h->pdus = pdus;
    h->pdu_cap = pdu_cap;
    h->bytes = bytes;
    h->bytes_cap = bytes_cap;
    h->times = times;
    h->next_offset = 0;
    h->full = false;
    long i = 0;
    while (i < nbytes) {
        const char* nl = (const char*)memchr(text + i, '\n', (size_t)(nbytes - i));
        const long e = nl ? (long)(nl - text) : nbytes;
        if (h->skipping) {
            // (nothing is kept of a line that is already too long)
        } else if ((long)h->partial.size() + (e - i) > h->max_line) {
            h->skipping = true;
            h->partial.clear();
        } else if (!nl || !h->partial.empty()) {
            h->partial.append(text + i, (size_t)(e - i));
        }
        if (!nl)
            break;
        if (h->skipping)
            h->line_end(nullptr, 0, true);
        else if (!h->partial.empty())
            h->line_end(h->partial.data(), (long)h->partial.size(), false);
        else
            h->line_end(text + i, e - i, false);
        h->partial.clear();
        h->skipping = false;
        i = e + 1;
    }
    long carried = (long)h->partial.size();
    for (const Sentence& s : h->group)
        carried += s.text_len;
    counts[AISX_NMEAP_CARRIED] = (int)carried;
    return counts[AISX_NMEAP_KEPT] < counts[AISX_NMEAP_FOUND] ? AISX_ERR_OVERFLOW : AISX_OK;
}
