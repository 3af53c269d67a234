// aisx_msgtab.h -- the ITU-R M.1371 field layouts, written once: the host aisx_msg_decode (aisx_msg.cpp, the
// specification) and the batched kernel (k_msg.h) read the same table through the same extraction helpers, and the
// writers (aisx_msg_encode, aisx_msg_enc.cpp, and k_msg_enc.h) run it the other way through their inverses, below.
//
// Message bit i is bit 7 - i % 8 of payload octet i / 8.  Both readers hold a payload as MSG_ROW big-endian 32-bit
// words (octets 4k .. 4k + 3 in word k, zero beyond the payload, word MSG_ROW - 1 always zero), so message bit i is
// bit 31 - i % 32 of word i / 32 and a field of up to 30 bits is a shift of the 64-bit window of two neighbouring
// words.  No layout reaches beyond bit 424: MSG_OCTETS octets of a payload are all that is ever looked at.
#pragma once
#include "aisx_common.h"

namespace aisx {

constexpr int MSG_OCTETS = 53;       // octets of a payload the layouts can reach (type 5 ends at bit 424)
constexpr int MSG_ROW = 15;          // words per staged payload: 14 hold octets, the last stays zero
constexpr int MSG_STR = 48;          // bytes of strings per row (include/aisx.h: AISX_MSG_STR)
constexpr int MSG_STR_WORDS = MSG_STR / 4;
constexpr int32_t MSG_NA = INT32_MIN;
constexpr int MSG_FL_COMPLETE = 1, MSG_FL_NO_LAYOUT = 2, MSG_FL_BAD_RECORD = 4;

// columns, in the order of include/aisx.h's AISX_MSG_COL_* (aisx_msg.cpp asserts that they agree)
enum MsgCol {
    MC_TYPE, MC_REPEAT, MC_MMSI, MC_FLAGS, MC_NAV_STATUS, MC_ROT, MC_SOG, MC_ACCURACY, MC_LON, MC_LAT, MC_COG, MC_HEADING,
    MC_SECOND, MC_MANEUVER, MC_RAIM, MC_RADIO, MC_IMO, MC_AIS_VERSION, MC_SHIPTYPE, MC_TO_BOW, MC_TO_STERN, MC_TO_PORT,
    MC_TO_STARBOARD, MC_EPFD, MC_YEAR, MC_MONTH, MC_DAY, MC_HOUR, MC_MINUTE, MC_DRAUGHT, MC_DTE, MC_PART, MC_AID_TYPE,
    MC_OFF_POSITION, MC_VIRTUAL_AID, MC_ASSIGNED, MC_CS_FLAGS, MSG_NCOL
};
// behind a layout's columns: the first bit of its call sign, name and destination (0 = not carried; none starts at
// bit 0) and its minimum length in bits
enum { MT_CALLSIGN = MSG_NCOL, MT_NAME, MT_DESTINATION, MT_MIN_BITS, MSG_TAB_ROW };
enum MsgLayout {
    ML_NONE,      // the common header only
    ML_POS_A,     // 1, 2, 3
    ML_BASE,      // 4, 11
    ML_STATIC,    // 5
    ML_POS_B,     // 18
    ML_POS_B_EXT, // 19
    ML_ATON,      // 21
    ML_24A,       // 24, part 0
    ML_24B,       // 24, part 1
    ML_24X,       // 24, another part or none readable
    ML_LONG,      // 27
    MSG_NLAYOUT
};
constexpr int MSG_TAB_WORDS = (int)MSG_NLAYOUT * (int)MSG_TAB_ROW;

// a field: first bit (9 bits) | width << 9 (0 = the layout has no such column, at most 30) | signed << 14 | op << 15
enum { MSG_OP_NONE, MSG_OP_X1000, MSG_OP_SOG27, MSG_OP_COG27 }; // type 27 -> class-A units
constexpr uint32_t msg_f(int start, int width, bool sgn = false, int op = MSG_OP_NONE)
{
    return (uint32_t)start | (uint32_t)width << 9 | (sgn ? 1u << 14 : 0u) | (uint32_t)op << 15;
}

struct MsgTab {
    uint32_t f[MSG_NLAYOUT][MSG_TAB_ROW];
};

constexpr MsgTab msg_make_tab()
{
    MsgTab t{};
    for (int l = 0; l < MSG_NLAYOUT; l++) {
        t.f[l][MC_TYPE] = msg_f(0, 6);
        t.f[l][MC_REPEAT] = msg_f(6, 2);
        t.f[l][MC_MMSI] = msg_f(8, 30);
    }
    uint32_t* r = t.f[ML_NONE];
    r[MT_MIN_BITS] = 38;

    r = t.f[ML_POS_A];
    r[MT_MIN_BITS] = 168;
    r[MC_NAV_STATUS] = msg_f(38, 4);
    r[MC_ROT] = msg_f(42, 8, true);
    r[MC_SOG] = msg_f(50, 10);
    r[MC_ACCURACY] = msg_f(60, 1);
    r[MC_LON] = msg_f(61, 28, true);
    r[MC_LAT] = msg_f(89, 27, true);
    r[MC_COG] = msg_f(116, 12);
    r[MC_HEADING] = msg_f(128, 9);
    r[MC_SECOND] = msg_f(137, 6);
    r[MC_MANEUVER] = msg_f(143, 2);
    r[MC_RAIM] = msg_f(148, 1);
    r[MC_RADIO] = msg_f(149, 19);

    r = t.f[ML_BASE];
    r[MT_MIN_BITS] = 168;
    r[MC_YEAR] = msg_f(38, 14);
    r[MC_MONTH] = msg_f(52, 4);
    r[MC_DAY] = msg_f(56, 5);
    r[MC_HOUR] = msg_f(61, 5);
    r[MC_MINUTE] = msg_f(66, 6);
    r[MC_SECOND] = msg_f(72, 6);
    r[MC_ACCURACY] = msg_f(78, 1);
    r[MC_LON] = msg_f(79, 28, true);
    r[MC_LAT] = msg_f(107, 27, true);
    r[MC_EPFD] = msg_f(134, 4);
    r[MC_RAIM] = msg_f(148, 1);
    r[MC_RADIO] = msg_f(149, 19);

    r = t.f[ML_STATIC];
    r[MT_MIN_BITS] = 422; // (424 transmitted; whole octets make the two the same)
    r[MC_AIS_VERSION] = msg_f(38, 2);
    r[MC_IMO] = msg_f(40, 30);
    r[MT_CALLSIGN] = 70;
    r[MT_NAME] = 112;
    r[MC_SHIPTYPE] = msg_f(232, 8);
    r[MC_TO_BOW] = msg_f(240, 9);
    r[MC_TO_STERN] = msg_f(249, 9);
    r[MC_TO_PORT] = msg_f(258, 6);
    r[MC_TO_STARBOARD] = msg_f(264, 6);
    r[MC_EPFD] = msg_f(270, 4);
    r[MC_MONTH] = msg_f(274, 4);
    r[MC_DAY] = msg_f(278, 5);
    r[MC_HOUR] = msg_f(283, 5);
    r[MC_MINUTE] = msg_f(288, 6);
    r[MC_DRAUGHT] = msg_f(294, 8);
    r[MT_DESTINATION] = 302;
    r[MC_DTE] = msg_f(422, 1);

    r = t.f[ML_POS_B];
    r[MT_MIN_BITS] = 168;
    r[MC_SOG] = msg_f(46, 10);
    r[MC_ACCURACY] = msg_f(56, 1);
    r[MC_LON] = msg_f(57, 28, true);
    r[MC_LAT] = msg_f(85, 27, true);
    r[MC_COG] = msg_f(112, 12);
    r[MC_HEADING] = msg_f(124, 9);
    r[MC_SECOND] = msg_f(133, 6);
    r[MC_CS_FLAGS] = msg_f(141, 6);
    r[MC_RAIM] = msg_f(147, 1);
    r[MC_RADIO] = msg_f(148, 20);

    r = t.f[ML_POS_B_EXT];
    r[MT_MIN_BITS] = 312;
    r[MC_SOG] = msg_f(46, 10);
    r[MC_ACCURACY] = msg_f(56, 1);
    r[MC_LON] = msg_f(57, 28, true);
    r[MC_LAT] = msg_f(85, 27, true);
    r[MC_COG] = msg_f(112, 12);
    r[MC_HEADING] = msg_f(124, 9);
    r[MC_SECOND] = msg_f(133, 6);
    r[MT_NAME] = 143;
    r[MC_SHIPTYPE] = msg_f(263, 8);
    r[MC_TO_BOW] = msg_f(271, 9);
    r[MC_TO_STERN] = msg_f(280, 9);
    r[MC_TO_PORT] = msg_f(289, 6);
    r[MC_TO_STARBOARD] = msg_f(295, 6);
    r[MC_EPFD] = msg_f(301, 4);
    r[MC_RAIM] = msg_f(305, 1);
    r[MC_DTE] = msg_f(306, 1);
    r[MC_ASSIGNED] = msg_f(307, 1);

    r = t.f[ML_ATON];
    r[MT_MIN_BITS] = 272;
    r[MC_AID_TYPE] = msg_f(38, 5);
    r[MT_NAME] = 43;
    r[MC_ACCURACY] = msg_f(163, 1);
    r[MC_LON] = msg_f(164, 28, true);
    r[MC_LAT] = msg_f(192, 27, true);
    r[MC_TO_BOW] = msg_f(219, 9);
    r[MC_TO_STERN] = msg_f(228, 9);
    r[MC_TO_PORT] = msg_f(237, 6);
    r[MC_TO_STARBOARD] = msg_f(243, 6);
    r[MC_EPFD] = msg_f(249, 4);
    r[MC_SECOND] = msg_f(253, 6);
    r[MC_OFF_POSITION] = msg_f(259, 1);
    r[MC_RAIM] = msg_f(268, 1);
    r[MC_VIRTUAL_AID] = msg_f(269, 1);
    r[MC_ASSIGNED] = msg_f(270, 1);

    r = t.f[ML_24A];
    r[MT_MIN_BITS] = 160;
    r[MC_PART] = msg_f(38, 2);
    r[MT_NAME] = 40;

    r = t.f[ML_24B];
    r[MT_MIN_BITS] = 168;
    r[MC_PART] = msg_f(38, 2);
    r[MC_SHIPTYPE] = msg_f(40, 8);
    r[MT_CALLSIGN] = 90;
    r[MC_TO_BOW] = msg_f(132, 9);
    r[MC_TO_STERN] = msg_f(141, 9);
    r[MC_TO_PORT] = msg_f(150, 6);
    r[MC_TO_STARBOARD] = msg_f(156, 6);

    r = t.f[ML_24X];
    r[MT_MIN_BITS] = 160;
    r[MC_PART] = msg_f(38, 2);

    r = t.f[ML_LONG];
    r[MT_MIN_BITS] = 96;
    r[MC_ACCURACY] = msg_f(38, 1);
    r[MC_RAIM] = msg_f(39, 1);
    r[MC_NAV_STATUS] = msg_f(40, 4);
    r[MC_LON] = msg_f(44, 18, true, MSG_OP_X1000); // 1/10 minute -> 1/10000 minute
    r[MC_LAT] = msg_f(62, 17, true, MSG_OP_X1000);
    r[MC_SOG] = msg_f(79, 6, false, MSG_OP_SOG27); // knots -> 1/10 knot, 63 -> 1023 (not available)
    r[MC_COG] = msg_f(85, 9, false, MSG_OP_COG27); // degrees -> 1/10 degree, 511 -> 3600 (not available)
    return t;
}

// bits [s, s + n) of the staged payload, 1 <= n <= 30, most significant first
AISX_HD uint32_t msg_bits(const uint32_t* w, int s, int n)
{
    const int a = s >> 5;
    const uint64_t v = (uint64_t)w[a] << 32 | w[a + 1]; // (a + 1 <= MSG_ROW - 1: the zero word)
    return (uint32_t)(v >> (64 - (s & 31) - n)) & ((1u << n) - 1u);
}

// the column a table entry describes, from a payload of nbits bits
AISX_HD int32_t msg_field(const uint32_t* w, uint32_t d, int nbits)
{
    const int s = (int)(d & 511u), n = (int)(d >> 9 & 31u);
    if (n == 0 || s + n > nbits)
        return MSG_NA;
    const uint32_t x = msg_bits(w, s, n);
    const int32_t v = (d >> 14 & 1u) ? (int32_t)(x << (32 - n)) >> (32 - n) : (int32_t)x;
    switch (d >> 15) {
    case MSG_OP_X1000:
        return v * 1000;
    case MSG_OP_SOG27:
        return v == 63 ? 1023 : v * 10;
    case MSG_OP_COG27:
        return v == 511 ? 3600 : v * 10;
    }
    return v;
}

// type (MSG_NA when the payload does not hold it) and, for type 24, its part number (likewise) -> layout
AISX_HD int msg_layout(int32_t type, int32_t part)
{
    switch (type) {
    case 1:
    case 2:
    case 3:
        return ML_POS_A;
    case 4:
    case 11:
        return ML_BASE;
    case 5:
        return ML_STATIC;
    case 18:
        return ML_POS_B;
    case 19:
        return ML_POS_B_EXT;
    case 21:
        return ML_ATON;
    case 24:
        return part == 0 ? ML_24A : part == 1 ? ML_24B : ML_24X;
    case 27:
        return ML_LONG;
    }
    return ML_NONE;
}

// the layout of a staged payload of nbits bits (a row of the table is MSG_TAB_ROW words at layout * MSG_TAB_ROW)
AISX_HD int msg_layout_of(const uint32_t* w, int nbits)
{
    return msg_layout(msg_field(w, msg_f(0, 6), nbits), msg_field(w, msg_f(38, 2), nbits));
}

AISX_HD int32_t msg_flags(const uint32_t* lay, int layout, int nbits)
{
    return (nbits >= (int)lay[MT_MIN_BITS] ? MSG_FL_COMPLETE : 0) | (layout == ML_NONE ? MSG_FL_NO_LAYOUT : 0);
}

AISX_HD uint32_t msg_char(uint32_t v) { return v < 32u ? v + 64u : v; }

// word j (0 .. MSG_STR_WORDS - 1) of a row's strings, its first byte lowest: [0, 7) call sign, [7] NUL, [8, 28) name,
// [28, 48) destination; `lay` is the layout's row of the table
AISX_HD uint32_t msg_str_word(const uint32_t* w, const uint32_t* lay, int nbits, int j)
{
    const int slot = j < 2 ? 0 : j < 7 ? 1 : 2;
    const int k0 = 4 * (j - (slot == 0 ? 0 : slot == 1 ? 2 : 7)); // first of this word's characters in the string
    const int nch = slot == 0 ? 7 : 20, n = j == 1 ? 3 : 4;
    const int s0 = (int)lay[MT_CALLSIGN + slot];
    if (s0 == 0 || s0 + 6 * nch > nbits)
        return 0;
    const uint32_t x = msg_bits(w, s0 + 6 * k0, 6 * n);
    uint32_t out = 0;
    for (int c = 0; c < n; c++)
        out |= msg_char(x >> (6 * (n - 1 - c)) & 63u) << (8 * c);
    return out;
}

// ------------------------------------------------------------------
// The writer (aisx_msg_encode, aisx_msg_enc.cpp, and the batched kernel, k_msg_enc.h): the same table read the other
// way.  A row of columns becomes the payload of its layout, ceil(MT_MIN_BITS / 8) octets, every bit that no column or
// string covers zero.
// ------------------------------------------------------------------
constexpr int MSG_ENC_OCTETS = 56;             // the pitch of a record's payload in the device form's list
constexpr int MSG_ENC_WORDS = MSG_ENC_OCTETS / 4; // = MSG_ROW - 1: the words of a staged payload that hold octets
constexpr int MSG_ENC_NO_MMSI = 1, MSG_ENC_NO_LAYOUT = 2, MSG_ENC_RANGE = 4, MSG_ENC_BAD_CHAR = 8, MSG_ENC_BAD_ROW = 16;

// what a column that is MSG_NA is written as, in class-A units: the protocol's "not available" where it has one
struct MsgDefaults {
    int32_t v[MSG_NCOL];
};
constexpr MsgDefaults msg_make_defaults()
{
    MsgDefaults d{};
    d.v[MC_NAV_STATUS] = 15;
    d.v[MC_ROT] = -128;
    d.v[MC_SOG] = 1023;
    d.v[MC_LON] = 181 * 600000;
    d.v[MC_LAT] = 91 * 600000;
    d.v[MC_COG] = 3600;
    d.v[MC_HEADING] = 511;
    d.v[MC_SECOND] = 60;
    d.v[MC_HOUR] = 24;
    d.v[MC_MINUTE] = 60;
    d.v[MC_DTE] = 1;
    return d;
}
// the table and the defaults as the writers hold them: MSG_ENC_TAB_WORDS words, the defaults behind the layouts
constexpr int MSG_ENC_TAB_WORDS = MSG_TAB_WORDS + (int)MSG_NCOL;
struct MsgEncTab {
    MsgTab t;
    MsgDefaults d;
};
constexpr MsgEncTab msg_make_enc_tab() { return MsgEncTab{ msg_make_tab(), msg_make_defaults() }; }

// the inverse of msg_bits: ors the low n bits of x into bits [s, s + n) of the staged payload, 1 <= n <= 30
AISX_HD void msg_put_bits(uint32_t* w, int s, int n, uint32_t x)
{
    const int a = s >> 5;
    const uint64_t v = (uint64_t)(x & ((1u << n) - 1u)) << (64 - (s & 31) - n);
    w[a] |= (uint32_t)(v >> 32);
    w[a + 1] |= (uint32_t)v; // (a + 1 <= MSG_ROW - 1; no field reaches that word, so it stays zero)
}

// the inverse of msg_field for a column value v that is not MSG_NA: the field's bits in *x; false when the value does
// not fit the field (nothing is ever truncated).  Type 27's three ops are undone in integers first, and the range
// applies to the converted value.
AISX_HD bool msg_unfield(uint32_t d, int32_t v, uint32_t* x)
{
    const int n = (int)(d >> 9 & 31u);
    bool ok = true;
    switch (d >> 15) {
    case MSG_OP_X1000: // to nearest, halves away from zero
        v = v >= 0 ? (int32_t)(((int64_t)v + 500) / 1000) : -(int32_t)((500 - (int64_t)v) / 1000);
        break;
    case MSG_OP_SOG27:
        ok = v >= 0 && v <= 1023;
        v = !ok ? 0 : v == 1023 ? 63 : v >= 615 ? 62 : (v + 5) / 10;
        break;
    case MSG_OP_COG27:
        ok = v >= 0;
        v = !ok ? 0 : v >= 3600 ? 511 : ((v + 5) / 10) % 360;
        break;
    }
    const int32_t lim = (int32_t)1 << ((d >> 14 & 1u) ? n - 1 : n);
    ok = ok && v < lim && v >= ((d >> 14 & 1u) ? -lim : 0);
    *x = (uint32_t)v & ((1u << n) - 1u);
    return ok;
}

// byte b of a string slot -> its six bits; false for a byte that has none (lower case included)
AISX_HD bool msg_unchar(uint32_t b, uint32_t* six)
{
    *six = b & 63u;
    return b >= 32u && b < 96u;
}

// One row -> the staged payload w[MSG_ROW] (zeroed here) and its length in octets; returns the status, 0 or a sum of
// MSG_ENC_*.  v: the row's MSG_NCOL columns; str: its MSG_STR bytes as MSG_STR_WORDS words, the first byte lowest
// (nullptr: all NUL); tab: MSG_ENC_TAB_WORDS words.  A refused row leaves w zero and *len 0.
AISX_HD int msg_encode_row(const int32_t* v, const uint32_t* str, int as_type, int as_part, const uint32_t* tab, uint32_t* w, int* len)
{
    for (int k = 0; k < MSG_ROW; k++)
        w[k] = 0;
    *len = 0;
    const int32_t type = as_type >= 1 && as_type <= 63 ? as_type : v[MC_TYPE];
    int32_t part = as_part >= 0 ? as_part : v[MC_PART];
    const int layout = type >= 1 && type <= 63 ? msg_layout(type, part) : ML_NONE;
    if (layout == ML_24X && part == MSG_NA)
        part = 3;
    int st = layout == ML_NONE ? MSG_ENC_NO_LAYOUT : 0;
    if (v[MC_MMSI] == MSG_NA)
        st |= MSG_ENC_NO_MMSI;
    else if (v[MC_MMSI] < 0 || v[MC_MMSI] >= 1 << 30) // (out of range: no MMSI, and a column that does not fit)
        st |= MSG_ENC_NO_MMSI | MSG_ENC_RANGE;
    const uint32_t* lay = tab + layout * MSG_TAB_ROW;
    const int32_t* def = (const int32_t*)(tab + MSG_TAB_WORDS);
    if (layout != ML_NONE) {
#pragma unroll
        for (int c = 0; c < MSG_NCOL; c++) { // (unrolled: the kernel holds v in registers)
            const uint32_t d = lay[c];
            if ((d >> 9 & 31u) == 0 || c == MC_FLAGS || c == MC_MMSI)
                continue;
            int32_t val = c == MC_TYPE ? type : c == MC_PART ? part : v[c];
            if (val == MSG_NA)
                val = def[c];
            uint32_t x;
            if (!msg_unfield(d, val, &x))
                st |= MSG_ENC_RANGE;
            msg_put_bits(w, (int)(d & 511u), (int)(d >> 9 & 31u), x);
        }
        msg_put_bits(w, 8, 30, (uint32_t)v[MC_MMSI]);
        for (int slot = 0; slot < 3; slot++) {
            const int s0 = (int)lay[MT_CALLSIGN + slot];
            if (s0 == 0 || !str)
                continue;
            const int nch = slot == 0 ? 7 : 20, b0 = slot == 0 ? 0 : slot == 1 ? 8 : 28;
            for (int k = 0; k < nch; k++) {
                const uint32_t b = str[(b0 + k) >> 2] >> (8 * ((b0 + k) & 3)) & 255u;
                if (b == 0)
                    break; // (from the first NUL on, the slot is zeros)
                uint32_t six;
                if (!msg_unchar(b, &six))
                    st |= MSG_ENC_BAD_CHAR;
                msg_put_bits(w, s0 + 6 * k, 6, six);
            }
        }
    }
    if (st != 0) {
        for (int k = 0; k < MSG_ROW; k++)
            w[k] = 0;
        return st;
    }
    *len = ((int)lay[MT_MIN_BITS] + 7) >> 3;
    return 0;
}

} // namespace aisx
