// k_msg_enc.h -- batched ITU-R M.1371 field encoder (the device form of aisx_msg_encode, aisx_msg_enc.cpp, which is
// its specification): the mirror of k_msg.h.  For every record of a call, one row of a struct-of-arrays table -- int32
// cols[MSG_NCOL][col_stride] and char strs[rows][MSG_STR], the decoder's or the vessel table's -- becomes one PDU of a
// device list in the aisx_pdu layout: record i at the fixed pitch of MSG_ENC_OCTETS bytes, so that nothing has to be
// scanned or counted to place it.
//
// One lane per record, 64 consecutive records per wave:
//   rows     lane l's row is its record's index, or idx[i]: without an index list column c is one load of 64
//            consecutive ints per wave, with one it is a gather.
//   strings  the wave copies its rows' 64 x MSG_STR bytes into LDS together, one 32-bit load per lane and pass: word
//            64 k + l of the wave's 64 x MSG_STR_WORDS, i.e. neighbouring lanes read neighbouring words of one row
//            (without an index list the 3072 bytes are one contiguous block).
//   encode   each lane runs the rule (aisx_msgtab.h: msg_encode_row) with the table in LDS and builds its payload's
//            MSG_ENC_WORDS big-endian words in its own LDS row.
//   store    the wave stores the 64 rows' 3584 contiguous payload bytes together, one byte-swapped 32-bit store per
//            lane and pass; a refused row's words are zero.  Records and status are written by their own lane.
// Rows stride MSG_ROW = 15 and MSG_SROW = 13 words in LDS: odd, so the lanes of a half wave fall on different banks.
// The two counts (rows encoded, rows refused) take one ballot per wave and one atomic add each by its first lane, on
// counters the per-call sequence clears in front of the kernel.
#pragma once
#include "aisx_common.h"
#include "aisx_msgtab.h"
#include "k_hdlc.h"

namespace aisx {

constexpr int MENC_T = 256;           // four waves per workgroup
constexpr int MENC_MAX_GROUPS = 4096;
constexpr int MENC_MAX_ROWS = 1 << 28; // (row counts and 64-bit byte offsets far from any overflow)
constexpr int MENC_SROW = MSG_STR_WORDS + 1;
constexpr int MENC_WAVE_WORDS = 64 * (MSG_ROW + MENC_SROW);
constexpr int MENC_NCNT = 5;          // count: [0] = [1] records, [2] bad-count flag, [3] encoded, [4] refused
constexpr int menc_lds_bytes(int nthreads) { return 4 * (MSG_ENC_TAB_WORDS + (nthreads / 64) * MENC_WAVE_WORDS); }

struct MsgEncParams {
    const int32_t* cols;  // [MSG_NCOL][col_stride]
    long long col_stride;
    const uint32_t* strs; // [table_rows][MSG_STR_WORDS], or nullptr: all NUL
    const int32_t* idx;   // optional: record i is made from row idx[i]
    const int* nrows;     // one int on the device: records to make
    const int32_t* chan;  // optional: the channel of record i, at [i] without idx and at [idx[i]] with it
    const uint32_t* tab;  // [MSG_ENC_TAB_WORDS] (MSG_ENC_TAB in device memory)
    int as_type, as_part;
    int nchan, max_rows, table_rows;
    int nwaves;           // waves in the grid (records are taken in strides of 64 * nwaves)
    HdlcRec* out;         // [max_rows]
    uint32_t* bytes;      // [max_rows][MSG_ENC_WORDS]
    int32_t* status;      // [max_rows]
    int* count;           // [MENC_NCNT]; [3] and [4] are zero on entry
};

// any multiple of 64 threads per workgroup, menc_lds_bytes(threads) of LDS
template <class Ctx>
AISX_DI void msg_enc_body(Ctx& cx, const MsgEncParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, wv = cx.wave_id();
    uint32_t* tab = (uint32_t*)cx.lds();
    uint32_t* pay = tab + MSG_ENC_TAB_WORDS + wv * MENC_WAVE_WORDS; // [64][MSG_ROW]
    uint32_t* str = pay + 64 * MSG_ROW;                             // [64][MENC_SROW]
    for (int k = t; k < MSG_ENC_TAB_WORDS; k += T)
        tab[k] = p.tab[k];
    cx.sync();
    int n = *p.nrows;
    const bool bad_count = n < 0 || n > p.max_rows;
    if (bad_count)
        n = 0;
    if (cx.bx() == 0 && t == 0) {
        p.count[0] = n;
        p.count[1] = n;
        if (bad_count)
            p.count[2] = 1;
    }
    const int step = 64 * p.nwaves;
    for (int i0 = 64 * (cx.bx() * (T >> 6) + wv); i0 < n; i0 += step) { // (i0 + step <= MENC_MAX_ROWS + 64 * MENC_MAX_GROUPS * 4: no overflow)
        const int i = i0 + l;
        const bool have = i < n;
        int row = have ? (p.idx ? p.idx[i] : i) : -1;
        bool ok = have && row >= 0 && row < p.table_rows;
        int ch = 0;
        if (ok && p.chan) {
            ch = p.chan[p.idx ? row : i];
            if (ch < 0 || ch >= p.nchan) {
                ok = false;
                ch = 0;
            }
        }
        if (!ok)
            row = -1;
        // strings: word d of the wave's rows is word d % MSG_STR_WORDS of the row of lane d / MSG_STR_WORDS
#pragma unroll
        for (int k = 0; k < MSG_STR_WORDS; k++) {
            const int d = 64 * k + l, rl = d / MSG_STR_WORDS, j = d - rl * MSG_STR_WORDS;
            const int r = cx.shfl_i32(row, rl);
            str[rl * MENC_SROW + j] = r >= 0 && p.strs ? p.strs[(long long)r * MSG_STR_WORDS + j] : 0u;
        }
        int32_t v[MSG_NCOL];
#pragma unroll
        for (int c = 0; c < MSG_NCOL; c++)
            v[c] = ok ? p.cols[(long long)c * p.col_stride + row] : MSG_NA;
        cx.wave_lds_sync();
        uint32_t* w = pay + l * MSG_ROW;
        int len = 0, st = MSG_ENC_BAD_ROW;
        if (ok)
            st = msg_encode_row(v, str + l * MENC_SROW, p.as_type, p.as_part, tab, w, &len);
        else
            for (int k = 0; k < MSG_ROW; k++)
                w[k] = 0;
        if (have) {
            HdlcRec r;
            r.end_bit = (unsigned long long)i;
            r.offset = (long long)MSG_ENC_OCTETS * i;
            r.chan = ch;
            r.len = len;
            p.out[i] = r;
            p.status[i] = st;
        }
        const unsigned long long good = cx.ballot(have && st == 0), all = cx.ballot(have);
        if (l == 0) {
            const int ng = aisx_popc64(good), na = aisx_popc64(all);
            if (ng)
                cx.atomic_add_i32(p.count + 3, ng);
            if (na - ng)
                cx.atomic_add_i32(p.count + 4, na - ng);
        }
        cx.wave_lds_sync();
        uint32_t* dst = p.bytes + (long long)i0 * MSG_ENC_WORDS;
#pragma unroll
        for (int k = 0; k < MSG_ENC_WORDS; k++) {
            const int d = 64 * k + l, rl = d / MSG_ENC_WORDS, m = d - rl * MSG_ENC_WORDS;
            if (i0 + rl < n)
                dst[d] = __builtin_bswap32(pay[rl * MSG_ROW + m]); // (octet 4 m first in memory)
        }
        cx.wave_lds_sync(); // (the next pass writes the rows these reads came from)
    }
}

// ------------------------------------------------------------------
// The launch plan of aisx_msg_enc_batch_* (host only): the argument check, the derived sizes, the buffers and the
// per-call sequence.  aisx_msg_enc.hip runs it on device memory, tests/emul_msg_enc on host memory.
// ------------------------------------------------------------------
struct MsgEncBufs {
    const uint32_t* tab; // MSG_ENC_TAB
    HdlcRec* pdus;       // [max_rows]
    uint32_t* bytes;     // [max_rows][MSG_ENC_WORDS]
    int32_t* status;     // [max_rows]
    int* count;          // [MENC_NCNT]
};

struct MsgEncPlan {
    int nchan, max_rows, table_rows, threads, groups;
    PlanBuf tab, pdus, bytes, status, count;

    // the argument check of aisx_msg_enc_batch_create: nullptr when it passes, else what is needed
    static const char* check(int nchan, int max_rows, int table_rows)
    {
        static_assert(MENC_MAX_ROWS == 1 << 28, "the bound in the text below");
        if (nchan < 1 || max_rows < 1 || table_rows < 1 || max_rows > MENC_MAX_ROWS)
            return "need nchan >= 1, 1 <= max_rows <= 2^28, table_rows >= 1";
        return nullptr;
    }
    // the argument check of aisx_msg_enc_batch_process, behind the pointers that must be there
    const char* check_call(long long col_stride, const void* strs) const
    {
        if (col_stride < table_rows || ((size_t)strs & 3u) != 0)
            return "need col_stride >= table_rows and strings aligned to 4 bytes";
        return nullptr;
    }
    // threads_: of a workgroup, a multiple of 64; max_groups: workgroups at most
    MsgEncPlan(int nchan_, int max_rows_, int table_rows_, int threads_ = MENC_T, int max_groups = MENC_MAX_GROUPS)
        : nchan(nchan_), max_rows(max_rows_), table_rows(table_rows_), threads(threads_)
    {
        const long long g = ((long long)max_rows + threads - 1) / threads;
        groups = (int)(g < max_groups ? g : max_groups);
        tab = { (size_t)MSG_ENC_TAB_WORDS, false };
        pdus = { (size_t)max_rows, false };
        bytes = { (size_t)MSG_ENC_WORDS * max_rows, false };
        status = { (size_t)max_rows, false };
        count = { (size_t)MENC_NCNT, true };
    }

    // clear(int* first, int n): n ints zeroed in front of the launch, in its queue
    template <class Clear, class Launch>
    bool process(const MsgEncBufs& b, const int32_t* cols, long long col_stride, const uint32_t* strs, const int32_t* idx,
                 const int* nrows, const int32_t* chan, int as_type, int as_part, Clear&& clear, Launch&& launch) const
    {
        MsgEncParams p;
        p.cols = cols;
        p.col_stride = col_stride;
        p.strs = strs;
        p.idx = idx;
        p.nrows = nrows;
        p.chan = chan;
        p.tab = b.tab;
        p.as_type = as_type;
        p.as_part = as_part;
        p.nchan = nchan;
        p.max_rows = max_rows;
        p.table_rows = table_rows;
        p.nwaves = groups * (threads / 64);
        p.out = b.pdus;
        p.bytes = b.bytes;
        p.status = b.status;
        p.count = b.count;
        if (!clear(b.count + 3, 2))
            return false;
        return launch(PlanLaunch{ 0, groups, 1, threads, menc_lds_bytes(threads) }, p);
    }
};

} // namespace aisx
