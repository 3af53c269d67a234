// aisx_framing.cpp -- host-side tail of the receive chain, plain C++:
//
//   aisx_hdlc_*      what digital.hdlc_deframer_bp(length_min, length_max) does for
//                    python/radio.py:64: HDLC bit de-stuffing, frames delimited by six
//                    consecutive ones, octets filled LSB first, CRC-16/X.25 over all but the
//                    last two octets, which carry the FCS low byte first;
//   aisx_pdu_to_nmea the sentence format of ais.pdu_to_nmea (observable behaviour of
//                    lib/pdu_to_nmea_impl.cc:63-131): ITU-R M.1371 / NMEA 0183 six-bit
//                    armouring, 56 payload characters per !AIVDM fragment, XOR checksum;
//   aisx_pdu_to_nmea_std  the same PDU as standard sentences (include/aisx.h states the form): the
//                    exact last character, the fill count on the last fragment only, a message id
//                    on multi-sentence messages, a tag block with the station and the time.
//
// Per-packet, bytes-per-second work: no GPU involved.  Written from the protocol rules; the
// reference's observable quirks that a consumer could depend on are kept and named below.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/aisx.h"
#include "aisx_repair.h"
#include "k_nmea_std.h"

namespace {

// CRC-16/X.25: polynomial 0x1021 reflected (0x8408), preset 0xFFFF, complemented result
class X25Fcs {
public:
    X25Fcs()
    {
        for (unsigned v = 0; v < 256; v++) {
            unsigned r = v;
            for (int k = 0; k < 8; k++)
                r = (r >> 1) ^ ((r & 1u) ? 0x8408u : 0u);
            table_[v] = (uint16_t)r;
        }
    }
    uint16_t operator()(const uint8_t* octets, size_t count) const
    {
        unsigned reg = 0xFFFFu;
        for (size_t k = 0; k < count; k++)
            reg = (reg >> 8) ^ table_[(reg ^ octets[k]) & 0xFFu];
        return (uint16_t)(~reg & 0xFFFFu);
    }

private:
    uint16_t table_[256];
};

const X25Fcs& fcs()
{
    static const X25Fcs f;
    return f;
}

// Single-error syndromes of the FCS check.  The CRC is linear, so one wrong bit at distance d from the frame's last
// bit (d = 0: the FCS's last bit) changes (computed FCS) xor (sent FCS) by a value that depends on d alone:
// 0x8000 for d = 0, one more step of the shift register for every bit further from the end.  The values repeat after
// 32767 steps; the first distance of each is kept.
class X25Syndromes {
public:
    X25Syndromes() : inv_(65536, 0)
    {
        unsigned s = 0x8000u;
        for (int d = 0; d < 32767; d++) {
            if (!inv_[s])
                inv_[s] = (uint16_t)(d + 1);
            s = (s >> 1) ^ ((s & 1u) ? 0x8408u : 0u);
        }
    }
    const uint16_t* inverse() const { return inv_.data(); } // [65536] distance + 1, 0 = no single error gives this

private:
    std::vector<uint16_t> inv_;
};

const X25Syndromes& syndromes()
{
    static const X25Syndromes s;
    return s;
}

// the event tables of aisx::hdlc_event_table, one per mask, built on first use
class X25EventTables {
public:
    const uint16_t* get(int events)
    {
        std::call_once(once_[events], [&] {
            tab_[events].resize(65536);
            aisx::hdlc_event_table(events, tab_[events].data());
        });
        return tab_[events].data();
    }

private:
    std::once_flag once_[AISX_HDLC_EV_ALL + 1];
    std::vector<uint16_t> tab_[AISX_HDLC_EV_ALL + 1];
};

} // namespace

// Receiver state: the run of ones seen so far (the de-stuffer), the octet being filled and the
// octets of the frame under way.
struct aisx_hdlc {
    int min_octets = 0, max_octets = 0;
    unsigned ones_run = 0;
    unsigned shift = 0;   // octet under construction, filled from the top and shifted down
    int nshift = 0;       // bits in it
    std::vector<uint8_t> frame;
    int nrules = 0;       // repair by CRC syndrome (aisx_hdlc_set_repair, _set_repair_events): off without rules
    aisx_hdlc_rule rules[AISX_HDLC_MAX_RULES] = {};
    int events = AISX_HDLC_EV_SINGLE;
    const uint16_t* event_tab = nullptr; // aisx::hdlc_event_table(events); not used for the single event alone

    void drop_frame()
    {
        frame.clear();
        shift = 0;
        nshift = 0;
    }
    void data_bit(unsigned bit)
    {
        // a frame that has outgrown length_max is abandoned as soon as one more data bit shows
        // up (the opening bits of the closing flag count: a frame of length_max + 1 octets never
        // survives, one of exactly length_max does)
        if ((int)frame.size() > max_octets) {
            drop_frame();
            return;
        }
        shift = (shift >> 1) | (bit ? 0x80u : 0u); // first bit received ends up as bit 0
        if (++nshift == 8) {
            frame.push_back((uint8_t)shift);
            shift = 0;
            nshift = 0;
        }
    }
    // six ones in a row: end of frame (or an abort / idle flags when nothing was collected).
    // Whole octets only; the flag's own leading bits sit in the partial octet and go with it.
    // the FCS of the frame does not match: one error event (one wrong bit, or with aisx_hdlc_set_repair_events one of
    // the enabled patterns) at the place the syndrome names, in a frame whose length has a rule and whose message type
    // after the flips the rule allows, is put right and the frame delivered with the mark first flipped bit's index
    // (bit 0 = the first bit received) | event id << 16; everything else is dropped
    template <class Sink>
    void repair(unsigned syndrome, Sink&& deliver)
    {
        const int got = (int)frame.size();
        const aisx_hdlc_rule* rule = nullptr;
        for (int k = 0; k < nrules && !rule; k++)
            if (rules[k].payload_octets == got - 2)
                rule = &rules[k];
        // (the single event alone keeps the table it always had, which reaches further than any frame can be long)
        const unsigned v = event_tab ? event_tab[syndrome] : syndromes().inverse()[syndrome];
        const int id = event_tab ? (int)(v >> 14) : 0, d1 = event_tab ? (int)(v & 0x3FFFu) : (int)v;
        if (!rule || !d1 || d1 - 1 + id >= 8 * got) // (an event's span is its id)
            return;
        const int last = 8 * got - d1, i = last - id;
        frame[(size_t)(last >> 3)] ^= (uint8_t)(1u << (last & 7)); // (in the FCS: the payload goes out as received)
        if (id)
            frame[(size_t)(i >> 3)] ^= (uint8_t)(1u << (i & 7));
        if ((rule->type_mask >> (frame[0] >> 2)) & 1u)
            deliver(frame.data(), got - 2, i | (id << 16));
    }
    template <class Sink>
    void delimiter(Sink&& deliver)
    {
        const int got = (int)frame.size();
        if (got >= min_octets) {
            const int payload = got - 2;
            const unsigned sent = (unsigned)frame[payload] | ((unsigned)frame[payload + 1] << 8);
            const unsigned syndrome = fcs()(frame.data(), (size_t)payload) ^ sent;
            if (syndrome == 0)
                deliver(frame.data(), payload, -1);
            else if (nrules)
                repair(syndrome, deliver);
        }
        drop_frame();
    }
};

extern "C" int aisx_hdlc_create(aisx_hdlc** h, int length_min, int length_max)
{
    // a frame is its payload plus the two FCS octets: anything shorter has no payload to check
    if (!h || length_min < 2 || length_max < length_min)
        return AISX_ERR_INVALID;
    aisx_hdlc* d = new aisx_hdlc();
    d->min_octets = length_min;
    d->max_octets = length_max;
    d->frame.reserve((size_t)length_max + 2);
    *h = d;
    return AISX_OK;
}

extern "C" int aisx_hdlc_destroy(aisx_hdlc* h)
{
    delete h;
    return AISX_OK;
}

// aisx_hdlc_work and aisx_hdlc_work_repair (fix_bits may be null)
static int hdlc_work(aisx_hdlc* h, const uint8_t* bits, int nbits, uint8_t* pdu_bytes, int pdu_cap, int* pdu_offsets,
                     int32_t* fix_bits, int max_pdus, int* npdus)
{
    if (!h || !bits || nbits < 0 || !npdus || (max_pdus > 0 && (!pdu_offsets || !pdu_bytes)))
        return AISX_ERR_INVALID;
    int found = 0, fill = 0, status = AISX_OK;
    if (max_pdus > 0)
        pdu_offsets[0] = 0;
    auto deliver = [&](const uint8_t* octets, int count, int fixed_bit) {
        if (found < max_pdus && fill + count <= pdu_cap) {
            memcpy(pdu_bytes + fill, octets, (size_t)count);
            fill += count;
            pdu_offsets[found + 1] = fill;
            if (fix_bits)
                fix_bits[found] = fixed_bit;
        } else {
            status = AISX_ERR_OVERFLOW;
        }
        found++;
    };
    for (const uint8_t *b = bits, *end = bits + nbits; b != end; ++b) {
        const unsigned bit = *b ? 1u : 0u;
        if (h->ones_run < 5)
            h->data_bit(bit);
        else if (bit)
            h->delimiter(deliver);
        // (else: the zero the transmitter stuffed behind five ones -- not data)
        h->ones_run = bit ? h->ones_run + 1 : 0;
    }
    *npdus = found;
    return status;
}

extern "C" int aisx_hdlc_work(aisx_hdlc* h, const uint8_t* bits, int nbits, uint8_t* pdu_bytes, int pdu_cap, int* pdu_offsets,
                              int max_pdus, int* npdus)
{
    return hdlc_work(h, bits, nbits, pdu_bytes, pdu_cap, pdu_offsets, nullptr, max_pdus, npdus);
}

extern "C" int aisx_hdlc_work_repair(aisx_hdlc* h, const uint8_t* bits, int nbits, uint8_t* pdu_bytes, int pdu_cap, int* pdu_offsets,
                                     int32_t* fix_bits, int max_pdus, int* npdus)
{
    if (max_pdus > 0 && !fix_bits)
        return AISX_ERR_INVALID;
    return hdlc_work(h, bits, nbits, pdu_bytes, pdu_cap, pdu_offsets, fix_bits, max_pdus, npdus);
}

int aisx::hdlc_rules_check(const aisx_hdlc_rule* rules, int nrules, int length_min, int length_max)
{
    if (nrules < 0 || nrules > AISX_HDLC_MAX_RULES || (nrules > 0 && !rules))
        return AISX_ERR_INVALID;
    for (int k = 0; k < nrules; k++) {
        if (rules[k].reserved != 0 || rules[k].payload_octets < length_min - 2 || rules[k].payload_octets > length_max - 2)
            return AISX_ERR_INVALID;
        for (int j = 0; j < k; j++)
            if (rules[j].payload_octets == rules[k].payload_octets)
                return AISX_ERR_INVALID;
    }
    return AISX_OK;
}

const uint16_t* aisx::hdlc_syndrome_table() { return syndromes().inverse(); }

void aisx::hdlc_event_table(int events, uint16_t* out)
{
    memset(out, 0, sizeof(uint16_t) * 65536);
    unsigned s[3] = { 0x8000u, 0, 0 }; // s(d), s(d + 1), s(d + 2)
    auto step = [](unsigned v) { return (v >> 1) ^ ((v & 1u) ? 0x8408u : 0u); };
    s[1] = step(s[0]);
    s[2] = step(s[1]);
    for (int d = 0; d < AISX_HDLC_EV_REACH; d++) { // ascending: the first event to claim a syndrome is the nearest
        for (int id = 0; id < 3; id++) {
            const unsigned syn = id ? s[0] ^ s[id] : s[0];
            if (((events >> id) & 1) && !out[syn])
                out[syn] = (uint16_t)((id << 14) | (d + 1));
        }
        s[0] = s[1];
        s[1] = s[2];
        s[2] = step(s[2]);
    }
}

const uint16_t* aisx::hdlc_event_table(int events)
{
    static X25EventTables tables;
    return tables.get(events & AISX_HDLC_EV_ALL);
}

extern "C" int aisx_hdlc_set_repair_events(aisx_hdlc* h, const aisx_hdlc_rule* rules, int nrules, int events)
{
    if (!h || !aisx::hdlc_events_ok(events) || aisx::hdlc_rules_check(rules, nrules, h->min_octets, h->max_octets) != AISX_OK)
        return AISX_ERR_INVALID;
    h->nrules = nrules;
    for (int k = 0; k < nrules; k++)
        h->rules[k] = rules[k];
    h->events = events;
    h->event_tab = events == AISX_HDLC_EV_SINGLE ? nullptr : aisx::hdlc_event_table(events);
    return AISX_OK;
}

extern "C" int aisx_hdlc_set_repair(aisx_hdlc* h, const aisx_hdlc_rule* rules, int nrules)
{
    return aisx_hdlc_set_repair_events(h, rules, nrules, AISX_HDLC_EV_SINGLE);
}

extern "C" int aisx_hdlc_event_table(int events, uint16_t* table)
{
    if (!table || !aisx::hdlc_events_ok(events))
        return AISX_ERR_INVALID;
    aisx::hdlc_event_table(events, table);
    return AISX_OK;
}

namespace {

// one payload character from a six-bit value: 0..39 -> '0'..'W', 40..63 -> '`'..'w'.
// Quirk kept from the reference (lib/pdu_to_nmea_impl.cc:81-88 compares a plain `char`): the
// padded last group can exceed 63, and a value of 128 or more counts as negative there.
inline char armour(unsigned group)
{
    const int as_char = (int)(int8_t)(uint8_t)group;
    return (char)(as_char + (as_char > 39 ? 56 : 48));
}

// bounded text sink that keeps the NMEA checksum (XOR of everything between '!' and '*')
class SentenceWriter {
public:
    SentenceWriter(char* dst, int cap) : dst_(dst), cap_(cap) {}
    void raw(char c)
    {
        if (used_ < cap_)
            dst_[used_] = c;
        used_++;
    }
    void put(char c)
    {
        sum_ ^= (uint8_t)c;
        raw(c);
    }
    void put(const char* s)
    {
        while (*s)
            put(*s++);
    }
    void put_number(int v)
    {
        char tmp[16];
        snprintf(tmp, sizeof tmp, "%d", v);
        put(tmp);
    }
    void open()
    {
        raw('!');
        sum_ = 0;
    }
    void close()
    {
        static const char hex[] = "0123456789ABCDEF";
        const uint8_t s = sum_;
        raw('*');
        raw(hex[s >> 4]);
        raw(hex[s & 15]);
    }
    int used() const { return used_; }

private:
    char* dst_;
    int cap_, used_ = 0;
    uint8_t sum_ = 0;
};

} // namespace

extern "C" int aisx_pdu_to_nmea(const char* designator, const uint8_t* pdu, int len, char* out, int cap)
{
    if (!designator || !pdu || len < 1 || !out || cap < 1)
        return AISX_ERR_INVALID;
    // payload: the PDU's bits, most significant first, in groups of six
    const int fill_bits = (6 - (len * 8) % 6) % 6;
    std::vector<char> payload;
    payload.reserve((size_t)(len * 8 + fill_bits) / 6);
    unsigned window = 0;
    int held = 0;
    for (int k = 0; k < len; k++) {
        window = ((window << 8) | pdu[k]) & 0xFFFFu;
        held += 8;
        while (held >= 6) {
            held -= 6;
            payload.push_back(armour((window >> held) & 63u));
        }
    }
    if (held > 0) {
        // Quirk kept from the reference (lib/pdu_to_nmea_impl.cc:70-78): the left-over bits are
        // placed at the top of their group and the group is then shifted up by the fill count
        // once more, in eight bits -- with 4 fill bits the group always comes out as 0
        const unsigned top_aligned = (window & ((1u << held) - 1u)) << (6 - held);
        payload.push_back(armour((top_aligned << fill_bits) & 0xFFu));
    }
    // fragments of at most 56 payload characters; every fragment reports the fill count (:113)
    const int per_fragment = 56;
    const int total = (int)payload.size();
    const int fragments = (total + per_fragment - 1) / per_fragment;
    SentenceWriter w(out, cap - 1);
    for (int f = 0; f < fragments; f++) {
        if (f)
            w.raw('\n');
        w.open();
        w.put("AIVDM,");
        w.put_number(fragments);
        w.put(',');
        w.put_number(f + 1);
        w.put(",,");
        w.put(designator);
        w.put(',');
        const int first = f * per_fragment, last = first + per_fragment < total ? first + per_fragment : total;
        for (int k = first; k < last; k++)
            w.put(payload[(size_t)k]);
        w.put(',');
        w.put_number(fill_bits);
        w.close();
    }
    if (w.used() > cap - 1)
        return AISX_ERR_OVERFLOW;
    out[w.used()] = '\0';
    return w.used();
}

extern "C" int aisx_nmea_std_text_len(int len, int dlen, int slen, int64_t time)
{
    if (len < 0 || len > aisx::NMS_MAX_OCTETS || dlen < 0 || slen < 0 || slen > aisx::NMS_STATION || !aisx::nms_time_ok(time))
        return AISX_ERR_INVALID;
    return aisx::nms_text_len(len, dlen, aisx::nms_tag_len(slen, aisx::nms_time_digits(time)));
}

extern "C" int aisx_pdu_to_nmea_std(const char* designator, const uint8_t* pdu, int len, int seq, const char* station, int64_t time,
                                    char* out, int cap)
{
    const char* sta = station ? station : "";
    if (!designator || !pdu || len < 1 || len > aisx::NMS_MAX_OCTETS || seq < 0 || seq > 9 || !aisx::nms_station_ok(sta) ||
        !aisx::nms_time_ok(time) || !out || cap < 1)
        return AISX_ERR_INVALID;
    // payload: the PDU's bits, most significant first, in groups of six, zeros behind the last bit
    const int total = (8 * len + 5) / 6, fill_bits = 6 * total - 8 * len;
    std::vector<char> payload((size_t)total);
    for (int k = 0; k < total; k++) {
        unsigned v = 0;
        for (int i = 6 * k; i < 6 * k + 6; i++)
            v = v << 1 | (i < 8 * len ? (pdu[i >> 3] >> (7 - (i & 7))) & 1u : 0u);
        payload[(size_t)k] = (char)(v < 40 ? v + 48 : v + 56);
    }
    // the tag block every fragment carries: \s:station,c:time*HH\ with HH over the fields
    char tag[64] = "";
    if (sta[0] || time >= 0) {
        char fields[48];
        int n = 0;
        if (sta[0])
            n += snprintf(fields + n, sizeof fields - (size_t)n, "s:%s", sta);
        if (time >= 0)
            n += snprintf(fields + n, sizeof fields - (size_t)n, "%sc:%lld", sta[0] ? "," : "", (long long)time);
        uint8_t sum = 0;
        for (int k = 0; k < n; k++)
            sum ^= (uint8_t)fields[k];
        snprintf(tag, sizeof tag, "\\%s*%02X\\", fields, sum);
    }
    const int per_fragment = 56;
    const int fragments = (total + per_fragment - 1) / per_fragment; // (at most nine: one digit)
    SentenceWriter w(out, cap - 1);
    for (int f = 0; f < fragments; f++) {
        if (f)
            w.raw('\n');
        for (const char* t = tag; *t; t++)
            w.raw(*t);
        w.open();
        w.put("AIVDM,");
        w.put_number(fragments);
        w.put(',');
        w.put_number(f + 1);
        w.put(',');
        if (fragments > 1)
            w.put_number(seq); // the sequential message id, on multi-sentence messages only
        w.put(',');
        w.put(designator);
        w.put(',');
        const int first = f * per_fragment, last = first + per_fragment < total ? first + per_fragment : total;
        for (int k = first; k < last; k++)
            w.put(payload[(size_t)k]);
        w.put(',');
        w.put_number(f + 1 == fragments ? fill_bits : 0); // the fill count belongs to the last fragment
        w.close();
    }
    if (w.used() > cap - 1)
        return AISX_ERR_OVERFLOW;
    out[w.used()] = '\0';
    return w.used();
}
