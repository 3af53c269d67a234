// k_msg.h -- batched ITU-R M.1371 field decoder (the device form of aisx_msg_decode, aisx_msg.cpp, which is its
// specification): for every PDU record of a device list in the aisx_pdu layout, one row of a struct-of-arrays table,
// int32 cols[MSG_NCOL][max_pdus] and char strs[max_pdus][MSG_STR].
//
// One lane per record, 64 consecutive records per wave:
//   stage    the wave copies its records' first MSG_OCTETS octets into LDS together, as big-endian words: lane l of
//            pass k builds word 64 k + l of the wave's 64 x MSG_ROW, i.e. neighbouring lanes read neighbouring bytes
//            of one payload (a lane walking its own payload would read 64 scattered lines per load).  Only octets
//            below a record's len are read; the rest of its row is zero.
//   columns  each lane extracts its row's fields from its LDS row with the layout table (aisx_msgtab.h, copied to
//            LDS once per workgroup) and stores column c at cols[c][i0 + lane]: 64 consecutive ints per store.
//   strings  each lane writes its row's twelve words of characters to LDS, and the wave stores the 64 rows'
//            3072 contiguous bytes together, one 32-bit store of four characters per lane and pass.
// Rows stride MSG_ROW = 15 and MSG_SROW = 13 words in LDS: odd, so the lanes of a half wave fall on different banks.
// No atomic anywhere: a record's row is its index, and the bad-input flag is only ever set to 1.
#pragma once
#include "aisx_common.h"
#include "aisx_msgtab.h"
#include "k_hdlc.h"

namespace aisx {

constexpr int MSG_T = 256;            // four waves per workgroup
constexpr int MSG_MAX_GROUPS = 4096;
constexpr int MSG_MAX_OCTETS = 1024;  // length_max bound (the deframer's)
constexpr int MSG_SROW = MSG_STR_WORDS + 1;
constexpr int MSG_WAVE_WORDS = 64 * (MSG_ROW + MSG_SROW);
constexpr int msg_lds_bytes(int nthreads) { return 4 * (MSG_TAB_WORDS + (nthreads / 64) * MSG_WAVE_WORDS); }

struct MsgParams {
    const HdlcRec* in;
    const unsigned char* bytes;
    const int* npdus;     // one int on the device: records to decode
    const int* nfound;    // optional: PDUs the producer found
    const uint32_t* tab;  // [MSG_NLAYOUT][MSG_TAB_ROW] (MSG_TAB in device memory)
    int nchan, max_pdus, max_len; // max_len = length_max - 1 payload octets
    int nwaves;           // waves in the grid (records are taken in strides of 64 * nwaves)
    int32_t* cols;        // [MSG_NCOL][max_pdus]
    uint32_t* strs;       // [max_pdus][MSG_STR_WORDS]
    int* count;           // [0] found, [1] rows written, [2] set after bad input (cleared by the read)
};

// any multiple of 64 threads per workgroup, msg_lds_bytes(threads) of LDS
template <class Ctx>
AISX_DI void msg_body(Ctx& cx, const MsgParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, wv = cx.wave_id();
    uint32_t* tab = (uint32_t*)cx.lds();
    uint32_t* pay = tab + MSG_TAB_WORDS + wv * MSG_WAVE_WORDS; // [64][MSG_ROW]
    uint32_t* str = pay + 64 * MSG_ROW;                        // [64][MSG_SROW]
    for (int k = t; k < MSG_TAB_WORDS; k += T)
        tab[k] = p.tab[k];
    cx.sync();
    int n = *p.npdus;
    const bool bad_count = n < 0 || n > p.max_pdus;
    if (bad_count)
        n = 0;
    if (cx.bx() == 0 && t == 0) {
        p.count[0] = bad_count ? 0 : (p.nfound ? *p.nfound : n);
        p.count[1] = n;
        if (bad_count)
            p.count[2] = 1;
    }
    const int step = 64 * p.nwaves;
    for (int i0 = 64 * (cx.bx() * (T >> 6) + wv); i0 < n; i0 += step) { // (i0 + step <= max_pdus + 64 * MSG_MAX_GROUPS * 4: no overflow)
        const int i = i0 + l;
        const bool have = i < n;
        HdlcRec r;
        r.offset = 0;
        r.chan = 0;
        r.len = 0;
        if (have)
            r = p.in[i];
        const bool bad = r.chan < 0 || r.chan >= p.nchan || r.len < 0 || r.len > p.max_len;
        const int take = bad ? 0 : (r.len < MSG_OCTETS ? r.len : MSG_OCTETS);
        if (bad)
            p.count[2] = 1;
        // stage: word f of the wave's rows is word f % MSG_ROW of record f / MSG_ROW
#pragma unroll 5
        for (int k = 0; k < MSG_ROW; k++) {
            const int f = 64 * k + l, row = f / MSG_ROW, m = f - row * MSG_ROW;
            const int tk = cx.shfl_i32(take, row);
            const unsigned char* src = p.bytes + (long long)cx.shfl_u64((unsigned long long)r.offset, row) + 4 * m;
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (4 * m + b < tk)
                    w |= (uint32_t)src[b] << (24 - 8 * b);
            pay[f] = w;
        }
        cx.wave_lds_sync();
        const uint32_t* w = pay + l * MSG_ROW;
        const int nbits = 8 * take;
        const int layout = msg_layout_of(w, nbits);
        const uint32_t* lay = tab + layout * MSG_TAB_ROW;
        const int32_t flags = bad ? MSG_FL_BAD_RECORD : msg_flags(lay, layout, nbits);
        int32_t* col = p.cols + i;
#pragma unroll
        for (int c = 0; c < MSG_NCOL; c++) {
            const int32_t v = c == MC_FLAGS ? flags : msg_field(w, lay[c], nbits); // (a bad record has nbits = 0: all NA)
            if (have)
                col[(long long)c * p.max_pdus] = v;
        }
#pragma unroll
        for (int j = 0; j < MSG_STR_WORDS; j++)
            str[l * MSG_SROW + j] = msg_str_word(w, lay, nbits, j);
        cx.wave_lds_sync();
        uint32_t* dst = p.strs + (long long)i0 * MSG_STR_WORDS;
#pragma unroll
        for (int k = 0; k < MSG_STR_WORDS; k++) {
            const int d = 64 * k + l, row = d / MSG_STR_WORDS, j = d - row * MSG_STR_WORDS;
            if (i0 + row < n)
                dst[d] = str[row * MSG_SROW + j];
        }
        cx.wave_lds_sync(); // (the next pass writes the rows these reads came from)
    }
}

// ------------------------------------------------------------------
// The launch plan of aisx_msg_batch_* (host only): the argument check, the derived sizes, the buffers and the
// per-call sequence.  aisx_msg.hip runs it on device memory, tests/emul_msg on host memory.
// ------------------------------------------------------------------
struct MsgBufs {
    const uint32_t* tab; // MSG_TAB
    int32_t* cols;       // [MSG_NCOL][max_pdus]
    uint32_t* strs;      // [max_pdus][MSG_STR_WORDS]
    int* count;          // [0] found, [1] rows written, [2] bad-input flag
};

struct MsgPlan {
    int nchan, max_pdus, lmax, threads, groups;
    PlanBuf tab, cols, strs, count;

    // the argument check of aisx_msg_batch_create: nullptr when it passes, else what is needed
    static const char* check(int nchan, int max_pdus, int length_max)
    {
        static_assert(MSG_MAX_OCTETS == 1024, "the bound in the text below");
        if (nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > MSG_MAX_OCTETS)
            return "need nchan >= 1, max_pdus >= 1, 2 <= length_max <= 1024";
        return nullptr;
    }
    // threads_: of a workgroup, a multiple of 64; max_groups: workgroups at most
    MsgPlan(int nchan_, int max_pdus_, int length_max, int threads_ = MSG_T, int max_groups = MSG_MAX_GROUPS)
        : nchan(nchan_), max_pdus(max_pdus_), lmax(length_max), threads(threads_)
    {
        const long long g = ((long long)max_pdus + threads - 1) / threads;
        groups = (int)(g < max_groups ? g : max_groups);
        tab = { (size_t)MSG_TAB_WORDS, false };
        cols = { (size_t)MSG_NCOL * max_pdus, false };
        strs = { (size_t)MSG_STR_WORDS * max_pdus, false };
        count = { 4, true };
    }

    template <class Launch>
    bool process(const MsgBufs& b, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound,
                 Launch&& launch) const
    {
        MsgParams p;
        p.in = pdus;
        p.bytes = bytes;
        p.npdus = npdus;
        p.nfound = nfound;
        p.tab = b.tab;
        p.nchan = nchan;
        p.max_pdus = max_pdus;
        p.max_len = lmax - 1;
        p.nwaves = groups * (threads / 64);
        p.cols = b.cols;
        p.strs = b.strs;
        p.count = b.count;
        return launch(PlanLaunch{ 0, groups, 1, threads, msg_lds_bytes(threads) }, p);
    }
};

} // namespace aisx
