// k_track.h -- the vessel table in device memory (the device form of aisx_track_update / aisx_track_expire,
// aisx_track.cpp, which is its specification): int32 tab[TRK_NCOL][capacity] and char strs[capacity][MSG_STR], vessel v
// the v-th distinct MMSI ever accepted, merged from the rows of a decoded table (k_msg.h's layout).
//
// The specification takes the rows one after the other; here one lane takes one row, and everything that depends on
// the order is computed from row indices, so that the result does not depend on the order the lanes ran in:
//
//   clear    the batch hash (MMSI -> the first row carrying it), 2 * max_rows slots or more, and the call's counters
//   find     every valid row claims or finds its MMSI's slot in the batch hash (compare-and-swap on the key) and
//            lowers the slot's first row to its own (atomic min; a lane whose lower neighbour carries the same MMSI
//            leaves that to the neighbour, so a batch of one MMSI issues one atomic per wave)
//   classify the first row of every MMSI looks it up in the table's hash (read only: known vessel or new); every
//            workgroup counts its first rows and its new ones
//   assign   a prefix sum of those counts over the rows: a new MMSI's rank among the batch's new MMSIs, ordered by first
//            row, gives its vessel nvessels_before + rank -- or, where that does not fit the capacity, drops it; the same
//            sum, less the dropped, is the MMSI's position j in the changed list.  The first row initialises a new
//            vessel's row of the table, enters the MMSI into the table's hash (accepted keys only: nothing provisional
//            ever gets there) and clears the changed vessel's winner cells.
//   winner   per changed vessel and column, the largest row index carrying a value (atomic max on win[c][j]; NA values
//            issue nothing, and a lane whose upper neighbour carries a value for the same vessel leaves it to that one)
//   apply    the row that won a cell stores its value at tab[c][v]; the vessel's last merged row stores COUNT, STAMP,
//            POS_STAMP and CHAN
//
// and expire is keep / compact: a prefix sum over the vessels' keep flags, a copy of the kept rows into the other table
// buffer at their new indices, and the table's hash cleared and filled again from the kept MMSIs.
// Workspace is indexed by row, by batch-hash slot or by changed-list position: nothing is cleared per capacity.
#pragma once
#include "aisx_common.h"
#include "aisx_msgtab.h"
#include "k_hdlc.h"

namespace aisx {

constexpr int TRK_T = 256;
constexpr int TRK_MAX = 1 << 24; // capacity and max_rows bound
enum { TC_COUNT = MSG_NCOL, TC_STAMP, TC_POS_STAMP, TC_CHAN, TRK_NCOL };
// the counts (include/aisx.h: AISX_TRK_CNT_*), and behind them what only the kernels use
enum { TN_VESSELS, TN_MERGED, TN_SKIPPED, TN_DROPPED, TN_CHANGED, TN_REMOVED, TN_FULL, TN_BAD, TRK_NCNT,
       TN_PREV = TRK_NCNT, // vessels before the running call
       TRK_COUNT_WORDS = 12 };
// winner cells of a changed vessel: the message columns, the three string slots, "a row had a position", rows merged
enum { TW_STR = MSG_NCOL, TW_POS = MSG_NCOL + 3, TW_COUNT, TRK_NWIN };
constexpr int32_t TRK_EMPTY = MSG_NA; // key of a free hash slot (a row whose MMSI is NA is never looked up)
constexpr int TRK_NEW = -1, TRK_DROPPED = -2;
constexpr int TRK_LDS_BYTES = 4 * 2 * (TRK_T / 64);

AISX_HD int trk_slot_word(int s) { return s == 0 ? 0 : s == 1 ? 2 : 7; }  // first word of string slot s
AISX_HD int trk_slot_words(int s) { return s == 0 ? 2 : 5; }
AISX_HD bool trk_always(int c) { return c == MC_TYPE || c == MC_REPEAT || c == MC_MMSI || c == MC_FLAGS; }
AISX_HD unsigned trk_hash(int32_t key, int bits) { return ((uint32_t)key * 2654435761u) >> (32 - bits); }
// slots of a hash that holds at most n keys: a power of two, at least 2 n
inline int trk_hash_bits(long long n)
{
    int b = 6;
    while ((1ll << b) < 2 * n)
        b++;
    return b;
}

struct TrkParams {
    const int32_t* in_cols; long long in_stride; // [MSG_NCOL][in_stride]
    const uint32_t* in_strs;                      // [rows][MSG_STR_WORDS]
    const HdlcRec* in_recs;                       // [rows] or nullptr
    const int* nrows;                             // one int on the device
    int32_t stamp;
    int capacity, max_rows, grid;                 // grid: workgroups of the launch
    int32_t* tab; uint32_t* strs;                 // the table: [TRK_NCOL][capacity], [capacity][MSG_STR_WORDS]
    int32_t* tab2; uint32_t* strs2;               // expire: the buffer the survivors go to; gather: the compact block
    int32_t* hkey; int* hval; int hbits;          // the table's hash: MMSI -> vessel
    int32_t* bkey; int* bfirst; int* bval; int* bj; int bbits; // the batch hash: MMSI -> first row, vessel, list position
    int* rslot;                                   // [max_rows] a row's batch-hash slot, -1 = skipped
    int* bsum; int nbmax;                         // [2][nbmax] per-workgroup counts
    int* win;                                     // [TRK_NWIN][max_rows]
    int* changed;                                 // [max_rows]
    int* count;                                   // [TRK_COUNT_WORDS]
};

AISX_DI int trk_nrows(const TrkParams& p)
{
    const int n = *p.nrows;
    return n < 0 || n > p.max_rows ? 0 : n;
}

// flags of this workgroup's lanes: in* = those set in the lanes below this one, blk* = in the whole workgroup
template <class Ctx>
AISX_DI void trk_block_scan(Ctx& cx, bool fa, bool fb, int& ina, int& inb, int& blka, int& blkb)
{
    const int l = cx.tid() & 63, wv = cx.wave_id(), nw = cx.nthreads() >> 6;
    int* lds = (int*)cx.lds();
    const unsigned long long ma = cx.ballot(fa), mb = cx.ballot(fb);
    if (l == 0) {
        lds[wv] = hd_popc(ma);
        lds[nw + wv] = hd_popc(mb);
    }
    cx.sync();
    ina = hd_popc(ma & hd_below(l));
    inb = hd_popc(mb & hd_below(l));
    blka = blkb = 0;
    for (int w = 0; w < nw; w++) {
        const int a = lds[w], b = lds[nw + w];
        if (w < wv) {
            ina += a;
            inb += b;
        }
        blka += a;
        blkb += b;
    }
    cx.sync();
}

// the sums of bsum[0][k] and bsum[1][k] over the workgroups k below this one
template <class Ctx>
AISX_DI void trk_block_base(Ctx& cx, const TrkParams& p, int& basea, int& baseb)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, wv = cx.wave_id(), nw = T >> 6;
    int* lds = (int*)cx.lds();
    int a = 0, b = 0;
    for (int k = t; k < cx.bx(); k += T) {
        a += p.bsum[k];
        b += p.bsum[p.nbmax + k];
    }
    for (int d = 1; d < 64; d <<= 1) {
        a += cx.shfl_xor_i32(a, d);
        b += cx.shfl_xor_i32(b, d);
    }
    if (l == 0) {
        lds[wv] = a;
        lds[nw + wv] = b;
    }
    cx.sync();
    basea = baseb = 0;
    for (int w = 0; w < nw; w++) {
        basea += lds[w];
        baseb += lds[nw + w];
    }
    cx.sync();
}

// MMSI -> vessel into the table's hash (the key is not in it; at most `capacity` keys in 2 * capacity slots or more)
template <class Ctx>
AISX_DI void trk_hash_put(Ctx& cx, const TrkParams& p, int32_t mmsi, int v)
{
    const unsigned mask = (1u << p.hbits) - 1u;
    unsigned s = trk_hash(mmsi, p.hbits);
    while (cx.atomic_cas_i32(&p.hkey[s], TRK_EMPTY, mmsi) != TRK_EMPTY)
        s = (s + 1) & mask;
    p.hval[s] = v;
}

template <class Ctx>
AISX_DI void trk_clear_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads();
    const long long nb = 1ll << p.bbits;
    for (long long k = (long long)cx.bx() * T + t; k < nb; k += (long long)p.grid * T) {
        p.bkey[k] = TRK_EMPTY;
        p.bfirst[k] = INT32_MAX;
    }
    if (cx.bx() == 0 && t == 0) {
        const int n = *p.nrows;
        p.count[TN_MERGED] = p.count[TN_SKIPPED] = p.count[TN_DROPPED] = p.count[TN_CHANGED] = p.count[TN_FULL] = 0;
        p.count[TN_PREV] = p.count[TN_VESSELS];
        if (n < 0 || n > p.max_rows)
            p.count[TN_BAD] = 1;
    }
}

template <class Ctx>
AISX_DI void trk_find_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, n = trk_nrows(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const bool have = i < n;
    const int32_t mmsi = have ? p.in_cols[MC_MMSI * p.in_stride + i] : MSG_NA;
    const int32_t flags = have ? p.in_cols[MC_FLAGS * p.in_stride + i] : 0;
    const bool valid = have && !(flags & MSG_FL_BAD_RECORD) && mmsi != MSG_NA;
    int slot = -1;
    if (valid) {
        const unsigned mask = (1u << p.bbits) - 1u;
        unsigned s = trk_hash(mmsi, p.bbits);
        for (;;) {
            int32_t k = *(const volatile int32_t*)&p.bkey[s]; // (a stale EMPTY is put right by the swap's answer)
            if (k == TRK_EMPTY)
                k = cx.atomic_cas_i32(&p.bkey[s], TRK_EMPTY, mmsi);
            if (k == TRK_EMPTY || k == mmsi)
                break;
            s = (s + 1) & mask;
        }
        slot = (int)s;
    }
    // the lane below carries the same MMSI: its row index is lower, and it (or one below it) issues the minimum
    const int below = cx.shfl_i32(valid ? mmsi : MSG_NA, l > 0 ? l - 1 : 0);
    if (valid && !(l > 0 && below == mmsi))
        cx.atomic_min_i32(&p.bfirst[slot], (int)i);
    if (have)
        p.rslot[i] = slot;
    const unsigned long long skipped = cx.ballot(have && !valid);
    if (l == 0 && skipped)
        cx.atomic_add_i32(&p.count[TN_SKIPPED], hd_popc(skipped));
}

template <class Ctx>
AISX_DI void trk_classify_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), n = trk_nrows(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const int slot = i < n ? p.rslot[i] : -1;
    const bool first = slot >= 0 && p.bfirst[slot] == (int)i;
    int v = TRK_NEW;
    if (first) {
        const int32_t mmsi = p.bkey[slot];
        const unsigned mask = (1u << p.hbits) - 1u;
        for (unsigned s = trk_hash(mmsi, p.hbits);; s = (s + 1) & mask) {
            const int32_t k = p.hkey[s];
            if (k == mmsi)
                v = p.hval[s];
            if (k == mmsi || k == TRK_EMPTY)
                break;
        }
        p.bval[slot] = v;
    }
    int ina, inb, blka, blkb;
    trk_block_scan(cx, first, first && v == TRK_NEW, ina, inb, blka, blkb);
    if (t == 0) {
        p.bsum[cx.bx()] = blka;
        p.bsum[p.nbmax + cx.bx()] = blkb;
    }
}

template <class Ctx>
AISX_DI void trk_assign_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), n = trk_nrows(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const int slot = i < n ? p.rslot[i] : -1;
    const bool first = slot >= 0 && p.bfirst[slot] == (int)i;
    int v = first ? p.bval[slot] : 0;
    const bool fresh = first && v == TRK_NEW;
    int baset, basen, int_, inn, blkt, blkn;
    trk_block_base(cx, p, baset, basen);
    trk_block_scan(cx, first, fresh, int_, inn, blkt, blkn);
    const int nv0 = p.count[TN_PREV], room = p.capacity - nv0;
    const int ext = baset + int_, exn = basen + inn; // first rows, and new MMSIs, below this row
    if (first) {
        if (fresh) {
            if (exn < room) {
                v = nv0 + exn;
                trk_hash_put(cx, p, p.bkey[slot], v);
                for (int c = 0; c < TRK_NCOL; c++)
                    p.tab[(long long)c * p.capacity + v] = c == TC_COUNT ? 0 : MSG_NA;
                for (int k = 0; k < MSG_STR_WORDS; k++)
                    p.strs[(long long)v * MSG_STR_WORDS + k] = 0u;
            } else
                v = TRK_DROPPED;
            p.bval[slot] = v;
        }
        if (v >= 0) {
            const int j = ext - (exn > room ? exn - room : 0);
            p.changed[j] = v;
            p.bj[slot] = j;
            for (int w = 0; w < TRK_NWIN; w++)
                p.win[(long long)w * p.max_rows + j] = w == TW_COUNT ? 0 : -1;
        }
    }
    if (t == 0 && (long long)(cx.bx() + 1) * T >= n) { // the last workgroup with rows: the totals
        const int tott = baset + blkt, totn = basen + blkn;
        p.count[TN_VESSELS] = nv0 + (totn < room ? totn : room);
        p.count[TN_CHANGED] = tott - (totn > room ? totn - room : 0);
    }
}

// a row's vessel and list position (-1: the row was skipped or dropped)
AISX_DI void trk_row_target(const TrkParams& p, long long i, int n, int& v, int& j)
{
    const int slot = i < n ? p.rslot[i] : -1;
    v = slot >= 0 ? p.bval[slot] : TRK_NEW;
    j = v >= 0 ? p.bj[slot] : -1;
}

template <class Ctx>
AISX_DI void trk_winner_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, n = trk_nrows(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    int v, j;
    trk_row_target(p, i, n, v, j);
    const bool merged = j >= 0;
    const int jup = cx.shfl_i32(j, l < 63 ? l + 1 : l), jdn = cx.shfl_i32(j, l > 0 ? l - 1 : l);
    const bool same_up = merged && l < 63 && jup == j; // the lane above merges into the same vessel, with a higher row
    const bool same_dn = merged && l > 0 && jdn == j;
    // a cell this row carries: the highest such row wins; a lane whose upper neighbour carries it too stays silent
    auto offer = [&](int w, bool carries) {
        const unsigned long long m = cx.ballot(carries);
        if (carries && !(same_up && ((m >> (l + 1)) & 1ull)))
            cx.atomic_max_i32(&p.win[(long long)w * p.max_rows + j], (int)i);
    };
    int32_t lon = MSG_NA, lat = MSG_NA;
#pragma unroll
    for (int c = 0; c < MSG_NCOL; c++) {
        const int32_t x = merged ? p.in_cols[c * p.in_stride + i] : MSG_NA;
        if (c == MC_LON)
            lon = x;
        if (c == MC_LAT)
            lat = x;
        offer(c, merged && (trk_always(c) || x != MSG_NA));
    }
#pragma unroll
    for (int s = 0; s < 3; s++)
        offer(TW_STR + s, merged && (p.in_strs[i * MSG_STR_WORDS + trk_slot_word(s)] & 255u) != 0u);
    offer(TW_POS, merged && lon != MSG_NA && lat != MSG_NA);
    // rows merged per vessel: the head of a run of lanes with one vessel adds the run's length
    const unsigned long long ends = cx.ballot(!same_up); // (lane 63 always ends a run)
    if (merged && !same_dn)
        cx.atomic_add_i32(&p.win[(long long)TW_COUNT * p.max_rows + j], hd_low(ends >> l) + 1);
    const unsigned long long mm = cx.ballot(merged), md = cx.ballot(v == TRK_DROPPED);
    if (l == 0 && mm)
        cx.atomic_add_i32(&p.count[TN_MERGED], hd_popc(mm));
    if (l == 0 && md)
        cx.atomic_add_i32(&p.count[TN_DROPPED], hd_popc(md));
}

template <class Ctx>
AISX_DI void trk_apply_body(Ctx& cx, const TrkParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), n = trk_nrows(p);
    const long long i = (long long)cx.bx() * T + t;
    if (cx.bx() == 0 && t == 0)
        p.count[TN_FULL] = p.count[TN_DROPPED] > 0 ? 1 : 0;
    if ((long long)cx.bx() * T >= n)
        return;
    int v, j;
    trk_row_target(p, i, n, v, j);
    if (j < 0)
        return;
    const int* win = p.win + j;
#pragma unroll
    for (int c = 0; c < MSG_NCOL; c++)
        if (win[(long long)c * p.max_rows] == (int)i)
            p.tab[(long long)c * p.capacity + v] = p.in_cols[c * p.in_stride + i];
#pragma unroll
    for (int s = 0; s < 3; s++)
        if (win[(long long)(TW_STR + s) * p.max_rows] == (int)i)
            for (int k = trk_slot_word(s); k < trk_slot_word(s) + trk_slot_words(s); k++)
                p.strs[(long long)v * MSG_STR_WORDS + k] = p.in_strs[i * MSG_STR_WORDS + k];
    if (win[(long long)MC_TYPE * p.max_rows] == (int)i) { // the vessel's last merged row (TYPE always overwrites)
        int32_t* col = p.tab + v;
        const long long sum = (long long)col[(long long)TC_COUNT * p.capacity] + win[(long long)TW_COUNT * p.max_rows];
        col[(long long)TC_COUNT * p.capacity] = sum > INT32_MAX ? INT32_MAX : (int32_t)sum;
        col[(long long)TC_STAMP * p.capacity] = p.stamp;
        if (win[(long long)TW_POS * p.max_rows] >= 0)
            col[(long long)TC_POS_STAMP * p.capacity] = p.stamp;
        col[(long long)TC_CHAN * p.capacity] = p.in_recs ? p.in_recs[i].chan : MSG_NA;
    }
}

// ---- expire: keep flags and the hash cleared; then the survivors compacted into tab2 / strs2 and entered again ----
template <class Ctx>
AISX_DI void trk_keep_body(Ctx& cx, const TrkParams& p, int32_t min_stamp)
{
    const int t = cx.tid(), T = cx.nthreads(), nv = p.count[TN_VESSELS];
    const long long nh = 1ll << p.hbits;
    for (long long k = (long long)cx.bx() * T + t; k < nh; k += (long long)p.grid * T)
        p.hkey[k] = TRK_EMPTY;
    if (cx.bx() == 0 && t == 0) {
        p.count[TN_PREV] = nv;
        p.count[TN_REMOVED] = p.count[TN_CHANGED] = 0;
    }
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= nv)
        return;
    const bool keep = i < nv && p.tab[(long long)TC_STAMP * p.capacity + i] >= min_stamp;
    int ina, inb, blka, blkb;
    trk_block_scan(cx, keep, false, ina, inb, blka, blkb);
    if (t == 0) {
        p.bsum[cx.bx()] = blka;
        p.bsum[p.nbmax + cx.bx()] = 0;
    }
}

template <class Ctx>
AISX_DI void trk_compact_body(Ctx& cx, const TrkParams& p, int32_t min_stamp)
{
    const int t = cx.tid(), T = cx.nthreads(), nv = p.count[TN_PREV];
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= nv)
        return;
    const bool keep = i < nv && p.tab[(long long)TC_STAMP * p.capacity + i] >= min_stamp;
    int base, baseb, in, inb, blk, blkb;
    trk_block_base(cx, p, base, baseb);
    trk_block_scan(cx, keep, false, in, inb, blk, blkb);
    if (keep) {
        const int d = base + in;
        for (int c = 0; c < TRK_NCOL; c++)
            p.tab2[(long long)c * p.capacity + d] = p.tab[(long long)c * p.capacity + i];
        for (int k = 0; k < MSG_STR_WORDS; k++)
            p.strs2[(long long)d * MSG_STR_WORDS + k] = p.strs[i * MSG_STR_WORDS + k];
        trk_hash_put(cx, p, p.tab[(long long)MC_MMSI * p.capacity + i], d);
    }
    if (t == 0 && (long long)(cx.bx() + 1) * T >= nv) {
        p.count[TN_VESSELS] = base + blk;
        p.count[TN_REMOVED] = nv - (base + blk);
    }
}

// the changed vessels' rows into the compact block tab2 [TRK_NCOL][max_rows], strs2 [max_rows][MSG_STR_WORDS]
template <class Ctx>
AISX_DI void trk_gather_body(Ctx& cx, const TrkParams& p)
{
    const long long j = (long long)cx.bx() * cx.nthreads() + cx.tid();
    int nc = p.count[TN_CHANGED];
    nc = nc < 0 ? 0 : nc > p.max_rows ? p.max_rows : nc;
    if (j >= nc)
        return;
    const int v = p.changed[j];
    for (int c = 0; c < TRK_NCOL; c++)
        p.tab2[(long long)c * p.max_rows + j] = p.tab[(long long)c * p.capacity + v];
    for (int k = 0; k < MSG_STR_WORDS; k++)
        p.strs2[j * MSG_STR_WORDS + k] = p.strs[(long long)v * MSG_STR_WORDS + k];
}

// ------------------------------------------------------------------
// The launch plan of aisx_track_batch_* (host only): the argument check, the derived sizes, the buffers and the
// per-call sequences.  aisx_track.hip runs it on device memory, tests/emul_track on host memory.
// ------------------------------------------------------------------
enum { TRK_K_CLEAR, TRK_K_FIND, TRK_K_CLASSIFY, TRK_K_ASSIGN, TRK_K_WINNER, TRK_K_APPLY, TRK_K_KEEP, TRK_K_COMPACT, TRK_K_GATHER };

struct TrkBufs {
    int32_t* tab[2];   // [TRK_NCOL][capacity]
    uint32_t* strs[2]; // [capacity][MSG_STR_WORDS]
    int32_t* hkey;     // [1 << hbits], TRK_EMPTY in an empty table
    int* hval;
    int32_t* bkey;     // [1 << bbits]
    int *bfirst, *bval, *bj;
    int* rslot;        // [max_rows]
    int* bsum;         // [2][max(row_groups, cap_groups)]
    int* win;          // [TRK_NWIN][max_rows]
    int* changed;      // [max_rows]
    int32_t* gcols;    // [TRK_NCOL][max_rows]   the changed vessels' rows, gathered
    uint32_t* gstrs;   // [max_rows][MSG_STR_WORDS]
    int* count;        // [TRK_COUNT_WORDS]
};

struct TrkCall {
    TrkParams p;
    int32_t min_stamp; // TRK_K_KEEP and TRK_K_COMPACT
};

struct TrkPlan {
    int capacity, max_rows, hbits, bbits, row_groups, cap_groups, clear_groups, nbmax;
    int cur = 0; // which table buffer the calls issued so far leave the table in
    PlanBuf tab, strs, hkey, hval, bkey, bfirst, bval, bj, rslot, bsum, win, changed, gcols, gstrs, count;

    // the argument check of aisx_track_batch_create: nullptr when it passes, else what is needed
    static const char* check(int capacity, int max_rows)
    {
        static_assert(TRK_MAX == 16777216, "the bound in the text below");
        if (capacity < 1 || capacity > TRK_MAX || max_rows < 1 || max_rows > TRK_MAX)
            return "need 1 <= capacity <= 16777216 and 1 <= max_rows <= 16777216";
        return nullptr;
    }
    TrkPlan(int capacity_, int max_rows_) : capacity(capacity_), max_rows(max_rows_)
    {
        hbits = trk_hash_bits(capacity);
        bbits = trk_hash_bits(max_rows);
        row_groups = (max_rows + TRK_T - 1) / TRK_T;
        cap_groups = (capacity + TRK_T - 1) / TRK_T;
        clear_groups = row_groups < 1024 ? row_groups : 1024;
        nbmax = row_groups > cap_groups ? row_groups : cap_groups;
        const size_t H = (size_t)1 << hbits, B = (size_t)1 << bbits, R = (size_t)max_rows, C = (size_t)capacity;
        tab = { TRK_NCOL * C, false };
        strs = { MSG_STR_WORDS * C, false };
        hkey = { H, false }; // (filled with TRK_EMPTY)
        hval = { H, false };
        bkey = bfirst = bval = bj = { B, false };
        rslot = { R, false };
        bsum = { 2 * (size_t)nbmax, false };
        win = { TRK_NWIN * R, false };
        changed = { R, false };
        gcols = { TRK_NCOL * R, false };
        gstrs = { MSG_STR_WORDS * R, false };
        count = { TRK_COUNT_WORDS, true };
    }
    void reset() { cur = 0; }

    TrkParams params(const TrkBufs& b) const
    {
        TrkParams p = {};
        p.capacity = capacity;
        p.max_rows = max_rows;
        p.tab = b.tab[cur];
        p.strs = b.strs[cur];
        p.hkey = b.hkey;
        p.hval = b.hval;
        p.hbits = hbits;
        p.bkey = b.bkey;
        p.bfirst = b.bfirst;
        p.bval = b.bval;
        p.bj = b.bj;
        p.bbits = bbits;
        p.rslot = b.rslot;
        p.bsum = b.bsum;
        p.nbmax = nbmax;
        p.win = b.win;
        p.changed = b.changed;
        p.count = b.count;
        return p;
    }
    static PlanLaunch on(int kernel, int groups) { return PlanLaunch{ kernel, groups, 1, TRK_T, TRK_LDS_BYTES }; }

    // aisx_track_batch_process: six kernels
    template <class Launch>
    bool process(const TrkBufs& b, const int32_t* cols, long col_stride, const uint32_t* strs_in, const HdlcRec* recs,
                 const int* nrows, int32_t stamp, Launch&& launch) const
    {
        TrkCall c = { params(b), 0 };
        TrkParams& p = c.p;
        p.in_cols = cols;
        p.in_stride = col_stride;
        p.in_strs = strs_in;
        p.in_recs = recs;
        p.nrows = nrows;
        p.stamp = stamp;
        p.grid = clear_groups;
        if (!launch(on(TRK_K_CLEAR, clear_groups), c))
            return false;
        p.grid = row_groups;
        for (int k = TRK_K_FIND; k <= TRK_K_APPLY; k++)
            if (!launch(on(k, row_groups), c))
                return false;
        return true;
    }
    // aisx_track_batch_expire: two kernels, after which the table is in the other buffer
    template <class Launch>
    bool expire(const TrkBufs& b, int32_t min_stamp, Launch&& launch)
    {
        TrkCall c = { params(b), min_stamp };
        c.p.tab2 = b.tab[cur ^ 1];
        c.p.strs2 = b.strs[cur ^ 1];
        c.p.grid = cap_groups;
        if (!launch(on(TRK_K_KEEP, cap_groups), c) || !launch(on(TRK_K_COMPACT, cap_groups), c))
            return false;
        cur ^= 1;
        return true;
    }
    // the gather of aisx_track_batch_read_changed: one kernel
    template <class Launch>
    bool gather(const TrkBufs& b, Launch&& launch) const
    {
        TrkCall c = { params(b), 0 };
        c.p.tab2 = b.gcols;
        c.p.strs2 = b.gstrs;
        c.p.grid = row_groups;
        return launch(on(TRK_K_GATHER, row_groups), c);
    }
};

} // namespace aisx
