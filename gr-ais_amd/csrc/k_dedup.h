// k_dedup.h -- PDUs heard by several receivers, suppressed in device memory (the device form of aisx_dedup_update,
// aisx_dedup.cpp, which is its specification): of the records of a PDU list that carry one payload, the first is kept and
// counts the others, and a payload kept within the last `window` calls is suppressed altogether.
//
// The specification takes the records one after the other; here one lane takes one record, and everything that depends
// on the order is computed from record indices, so that the result does not depend on the order the lanes ran in:
//
//   clear    the call hash (key -> the first record carrying it, and how many do), 2 * max_pdus slots or more, the set of
//            the ring that this call's kept keys will enter, and the call's counters
//   find     every record with a good length computes its key (dd_key: one lane, eight octets a step, read byte by byte
//            because a payload starts at any address and nothing outside it may be touched), claims or finds the key's
//            slot in the call hash (compare-and-swap on the key), lowers the slot's first record to its own (atomic min)
//            and adds itself to the slot's copies (atomic add; the head of a run of lanes with one key does both for the
//            run, and skips the minimum where the cell is already lower, so a list of one payload issues at most two atomics
//            per wave)
//   classify the first record of every key looks the key up in the ring's sets whose stamp lies inside the window (read
//            only; at most one holds it); every workgroup counts the records it keeps: the bad ones and the first
//            records of keys that are not remembered
//   assign   a prefix sum of those counts over the records gives a kept record its output index j; it copies its record and
//            mark there, writes copies[j], and enters its key into this call's set (kept keys only)
//   fill     first[i] of every keyed record from its key's slot, and the two counts of suppressed records
//
// Every probe loop is bounded by the slot count.  Workspace is indexed by record or by slot; what is cleared per call is
// the call hash and ONE set of the ring, both in proportion to max_pdus.
#pragma once
#include "aisx_common.h"
#include "k_hdlc.h"
#include "k_track.h"

namespace aisx {

typedef unsigned long long dd_u64;

constexpr int DD_T = TRK_T;
constexpr int DD_MAX = 1 << 24;  // max_pdus bound
constexpr int DD_MAX_WINDOW = 15;
constexpr int DD_LDS_BYTES = TRK_LDS_BYTES; // (trk_block_scan's)
// the counts (include/aisx.h: AISX_DEDUP_CNT_*), and the device form's count words: found, written, flag, then those
enum { DN_IN, DN_KEPT, DN_DUP_CALL, DN_DUP_WINDOW, DN_BAD_LEN, DD_NCNT };
enum { DC_FOUND, DC_WRITTEN, DC_BAD };
constexpr int DC_CNT = 3, DD_COUNT_WORDS = DC_CNT + DD_NCNT;
constexpr dd_u64 DD_EMPTY = 0ull; // key of a free slot: dd_key never returns it
constexpr int DD_UNKEYED = -2;    // rslot of a record whose len is bad (-1: no record)

// ---- the key (include/aisx.h states it) ----
AISX_HD dd_u64 dd_key_begin(int len) { return 0x9E3779B97F4A7C15ull ^ ((dd_u64)(long long)len * 0xFF51AFD7ED558CCDull); }
AISX_HD dd_u64 dd_key_step(dd_u64 h, dd_u64 w)
{
    h = (h ^ w) * 0x9FB21C651E98DF25ull;
    return h ^ (h >> 32);
}
AISX_HD dd_u64 dd_key_end(dd_u64 h)
{
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h == DD_EMPTY ? 1ull : h;
}
// len >= 0; reads pdu[0 .. len) and nothing else
AISX_HD dd_u64 dd_key(const unsigned char* pdu, int len)
{
    dd_u64 h = dd_key_begin(len);
    for (int k = 0; k < len; k += 8) {
        dd_u64 w = 0;
#pragma unroll
        for (int b = 0; b < 8; b++)
            if (k + b < len)
                w |= (dd_u64)pdu[k + b] << (8 * b);
        h = dd_key_step(h, w);
    }
    return dd_key_end(h);
}
// a key's home slot in a hash of 1 << bits slots; a probe chain goes on at (s + 1) & mask
AISX_HD unsigned dd_home(dd_u64 key, int bits) { return (unsigned)(key >> (64 - bits)); }

struct DdParams {
    const HdlcRec* in;           // the producer's records
    const unsigned char* bytes;  // and their payload bytes
    const int* npdus;            // one int on the device: records handed over
    const int* nfound;           // one int on the device or nullptr: PDUs the producer found
    const int32_t* marks;        // [records] or nullptr
    int max_pdus, max_len, grid, bits; // max_len: length_max - 1; grid: workgroups of the launch
    dd_u64* ckey; int* cfirst; int* ccount; int* cval; // the call hash [1 << bits]: key -> first record, records, first[] of the others
    dd_u64* ring;                // [window + 1][1 << bits] the remembered keys, one set per stamp
    int cur;                     // the set this call's kept keys enter (cleared by this call)
    int nsets;                   // the other sets whose stamp lies inside the window,
    unsigned char set[DD_MAX_WINDOW], age[DD_MAX_WINDOW]; // and stamp - their stamp, 1 .. window
    int* rslot;                  // [max_pdus] a record's slot in the call hash, or DD_UNKEYED
    int* bsum;                   // [workgroups] kept records per workgroup
    HdlcRec* out; int32_t* first; int32_t* copies; int32_t* omarks; // [max_pdus] each
    int* count;                  // [DD_COUNT_WORDS]
};

AISX_DI int dd_nrecs(const DdParams& p)
{
    const int n = *p.npdus;
    return n < 0 || n > p.max_pdus ? 0 : n;
}

// the slot of `key` in the set `tab`, or -1 when the chain from its home slot ends without it
AISX_DI int dd_lookup(const dd_u64* tab, int bits, dd_u64 key)
{
    const unsigned mask = (1u << bits) - 1u;
    unsigned s = dd_home(key, bits);
    for (unsigned probes = 0; probes <= mask; probes++, s = (s + 1) & mask) {
        const dd_u64 k = tab[s];
        if (k == key)
            return (int)s;
        if (k == DD_EMPTY)
            return -1;
    }
    return -1;
}

// the sum of bsum[k] over the workgroups k below this one
template <class Ctx>
AISX_DI int dd_block_base(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, wv = cx.wave_id(), nw = T >> 6;
    int* lds = (int*)cx.lds();
    int a = 0;
    for (int k = t; k < cx.bx(); k += T)
        a += p.bsum[k];
    for (int d = 1; d < 64; d <<= 1)
        a += cx.shfl_xor_i32(a, d);
    if (l == 0)
        lds[wv] = a;
    cx.sync();
    int base = 0;
    for (int w = 0; w < nw; w++)
        base += lds[w];
    cx.sync();
    return base;
}

template <class Ctx>
AISX_DI void dd_clear_body(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads();
    const long long nb = 1ll << p.bits;
    dd_u64* mine = p.ring + (long long)p.cur * nb;
    for (long long k = (long long)cx.bx() * T + t; k < nb; k += (long long)p.grid * T) {
        p.ckey[k] = DD_EMPTY;
        p.cfirst[k] = INT32_MAX;
        p.ccount[k] = 0;
        mine[k] = DD_EMPTY;
    }
    if (cx.bx() == 0 && t == 0) {
        const int n = *p.npdus;
        const bool bad = n < 0 || n > p.max_pdus;
        const int found = p.nfound ? *p.nfound : n;
        p.count[DC_FOUND] = !bad && found > n ? found - n : 0; // (assign adds the kept records)
        p.count[DC_WRITTEN] = 0;
        if (bad)
            p.count[DC_BAD] = 1;
        for (int c = 0; c < DD_NCNT; c++)
            p.count[DC_CNT + c] = 0;
        p.count[DC_CNT + DN_IN] = bad ? 0 : n;
    }
}

template <class Ctx>
AISX_DI void dd_find_body(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, n = dd_nrecs(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const bool have = i < n;
    long long off = 0;
    int len = -1;
    if (have) {
        off = p.in[i].offset;
        len = p.in[i].len;
    }
    const bool good = have && len >= 0 && len <= p.max_len;
    dd_u64 key = DD_EMPTY;
    int slot = -1;
    if (good) {
        const dd_u64 mykey = dd_key(p.bytes + off, len);
        const unsigned mask = (1u << p.bits) - 1u;
        unsigned s = dd_home(mykey, p.bits);
        // (at most max_pdus keys in 2 * max_pdus slots or more: the chain ends; the bound is for what cannot happen)
        for (unsigned probes = 0; probes <= mask; probes++, s = (s + 1) & mask) {
            dd_u64 k = *(const volatile dd_u64*)&p.ckey[s]; // (a stale EMPTY is put right by the swap's answer)
            if (k == DD_EMPTY)
                k = cx.atomic_cas_u64(&p.ckey[s], DD_EMPTY, mykey);
            if (k == DD_EMPTY || k == mykey) {
                slot = (int)s;
                key = mykey;
                break;
            }
        }
    }
    const bool keyed = slot >= 0;
    // lanes below and above with the same key: the head of such a run has the lowest record index and acts for all of it
    const dd_u64 kdn = cx.shfl_u64(key, l > 0 ? l - 1 : 0), kup = cx.shfl_u64(key, l < 63 ? l + 1 : l);
    const bool same_dn = keyed && l > 0 && kdn == key, same_up = keyed && l < 63 && kup == key;
    const unsigned long long ends = cx.ballot(!same_up); // (lane 63 always ends a run)
    if (keyed && !same_dn) {
        // (the cell only ever falls: a value already at or below i, however stale, makes the minimum a no-op)
        if (*(const volatile int*)&p.cfirst[slot] > (int)i)
            cx.atomic_min_i32(&p.cfirst[slot], (int)i);
        cx.atomic_add_i32(&p.ccount[slot], hd_low(ends >> l) + 1);
    }
    if (have)
        p.rslot[i] = keyed ? slot : DD_UNKEYED;
    const unsigned long long badm = cx.ballot(have && !good);
    if (l == 0 && badm)
        cx.atomic_add_i32(&p.count[DC_CNT + DN_BAD_LEN], hd_popc(badm));
}

template <class Ctx>
AISX_DI void dd_classify_body(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), n = dd_nrecs(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const int slot = i < n ? p.rslot[i] : -1;
    const bool head = slot >= 0 && p.cfirst[slot] == (int)i;
    int v = 0;
    if (head) {
        const dd_u64 key = p.ckey[slot];
        const long long nb = 1ll << p.bits;
        for (int q = 0; q < p.nsets; q++)
            if (dd_lookup(p.ring + (long long)p.set[q] * nb, p.bits, key) >= 0) {
                v = -1 - (int)p.age[q];
                break;
            }
        p.cval[slot] = v; // first[] of the key's records when it is remembered; else assign puts j here
    }
    const bool keep = slot == DD_UNKEYED || (head && v == 0);
    int ina, inb, blka, blkb;
    trk_block_scan(cx, keep, false, ina, inb, blka, blkb);
    if (t == 0)
        p.bsum[cx.bx()] = blka;
}

template <class Ctx>
AISX_DI void dd_assign_body(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), n = dd_nrecs(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const int slot = i < n ? p.rslot[i] : -1;
    const bool head = slot >= 0 && p.cfirst[slot] == (int)i;
    // (a slot's cval is read here by the key's first record alone, before that same lane overwrites it)
    const bool keep = slot == DD_UNKEYED || (head && p.cval[slot] == 0);
    const int base = dd_block_base(cx, p);
    int in, inb, blk, blkb;
    trk_block_scan(cx, keep, false, in, inb, blk, blkb);
    if (keep) {
        const int j = base + in;
        p.out[j] = p.in[i];
        if (p.marks)
            p.omarks[j] = p.marks[i];
        p.first[i] = j;
        p.copies[j] = slot >= 0 ? p.ccount[slot] : 1;
        if (slot >= 0) {
            p.cval[slot] = j;
            // the key into this call's set (it is not in it; at most max_pdus keys in 2 * max_pdus slots or more)
            const dd_u64 key = p.ckey[slot];
            dd_u64* mine = p.ring + ((long long)p.cur << p.bits);
            const unsigned mask = (1u << p.bits) - 1u;
            unsigned s = dd_home(key, p.bits);
            for (unsigned probes = 0; probes <= mask; probes++, s = (s + 1) & mask)
                if (cx.atomic_cas_u64(&mine[s], DD_EMPTY, key) == DD_EMPTY)
                    break;
        }
    }
    if (t == 0 && (long long)(cx.bx() + 1) * T >= n) { // the last workgroup with records: the totals
        const int kept = base + blk;
        p.count[DC_FOUND] += kept;
        p.count[DC_WRITTEN] = kept;
        p.count[DC_CNT + DN_KEPT] = kept;
    }
}

template <class Ctx>
AISX_DI void dd_fill_body(Ctx& cx, const DdParams& p)
{
    const int t = cx.tid(), T = cx.nthreads(), l = t & 63, n = dd_nrecs(p);
    const long long i = (long long)cx.bx() * T + t;
    if ((long long)cx.bx() * T >= n)
        return;
    const int slot = i < n ? p.rslot[i] : -1;
    const bool keyed = slot >= 0;
    const int v = keyed ? p.cval[slot] : 0;
    if (keyed)
        p.first[i] = v;
    const unsigned long long dw = cx.ballot(keyed && v < 0), dc = cx.ballot(keyed && v >= 0 && p.cfirst[slot] != (int)i);
    if (l == 0 && dw)
        cx.atomic_add_i32(&p.count[DC_CNT + DN_DUP_WINDOW], hd_popc(dw));
    if (l == 0 && dc)
        cx.atomic_add_i32(&p.count[DC_CNT + DN_DUP_CALL], hd_popc(dc));
}

// ------------------------------------------------------------------
// The launch plan of aisx_dedup_batch_* (host only): the argument check, the derived sizes, the buffers, the ring's
// stamps and the per-call sequence.  aisx_dedup.hip runs it on device memory, tests/emul_dedup on host memory.
// ------------------------------------------------------------------
enum { DD_K_CLEAR, DD_K_FIND, DD_K_CLASSIFY, DD_K_ASSIGN, DD_K_FILL, DD_NKERNELS };

struct DdBufs {
    dd_u64* ckey;  // [1 << bits]
    int *cfirst, *ccount, *cval;
    dd_u64* ring;  // [window + 1][1 << bits]
    int* rslot;    // [max_pdus]
    int* bsum;     // [groups]
    HdlcRec* out;  // [max_pdus]
    int32_t *first, *copies, *omarks;
    int* count;    // [DD_COUNT_WORDS]
};

struct DdPlan {
    int window, max_pdus, length_max, bits, groups, clear_groups;
    PlanBuf ckey, cfirst, ccount, cval, ring, rslot, bsum, out, first, copies, omarks, count;
    // the ring: which set the last call filled, the stamp each set was filled at, and the last call's stamp
    int cur = 0;
    bool used[DD_MAX_WINDOW + 1] = {};
    long long label[DD_MAX_WINDOW + 1] = {};
    bool have_prev = false;
    long long prev = 0;

    // the argument check of aisx_dedup_batch_create: nullptr when it passes, else what is needed
    static const char* check(int window, int max_pdus, int length_max)
    {
        static_assert(DD_MAX == 16777216 && DD_MAX_WINDOW == 15, "the bounds in the text below");
        if (window < 0 || window > DD_MAX_WINDOW || max_pdus < 1 || max_pdus > DD_MAX || length_max < 2 || length_max > 1024)
            return "need 0 <= window <= 15, 1 <= max_pdus <= 16777216 and 2 <= length_max <= 1024";
        return nullptr;
    }
    DdPlan(int window_, int max_pdus_, int length_max_) : window(window_), max_pdus(max_pdus_), length_max(length_max_)
    {
        bits = trk_hash_bits(max_pdus);
        groups = (max_pdus + DD_T - 1) / DD_T;
        clear_groups = groups < 1024 ? groups : 1024;
        const size_t B = (size_t)1 << bits, R = (size_t)max_pdus;
        ckey = cfirst = ccount = cval = { B, false };
        ring = { B * (size_t)(window + 1), false }; // (a set is cleared by the call that fills it)
        rslot = out = first = copies = omarks = { R, false };
        bsum = { (size_t)groups, false };
        count = { DD_COUNT_WORDS, true };
    }
    void reset()
    {
        cur = 0;
        have_prev = false;
        for (bool& u : used)
            u = false;
    }
    // the stamp rule: strictly above the previous call's
    bool stamp_ok(int32_t stamp) const { return !have_prev || (long long)stamp > prev; }
    static PlanLaunch on(int kernel, int groups) { return PlanLaunch{ kernel, groups, 1, DD_T, DD_LDS_BYTES }; }

    // aisx_dedup_batch_process: five kernels (the caller has checked stamp_ok)
    template <class Launch>
    bool process(const DdBufs& b, const HdlcRec* in, const unsigned char* bytes, const int* npdus, const int* nfound,
                 const int32_t* marks, int32_t stamp, Launch&& launch)
    {
        cur = (cur + 1) % (window + 1);
        used[cur] = true;
        label[cur] = stamp;
        have_prev = true;
        prev = stamp;
        DdParams p = {};
        p.in = in;
        p.bytes = bytes;
        p.npdus = npdus;
        p.nfound = nfound;
        p.marks = marks;
        p.max_pdus = max_pdus;
        p.max_len = length_max - 1;
        p.bits = bits;
        p.ckey = b.ckey;
        p.cfirst = b.cfirst;
        p.ccount = b.ccount;
        p.cval = b.cval;
        p.ring = b.ring;
        p.cur = cur;
        for (int q = 0; q <= window; q++) {
            const long long age = (long long)stamp - label[q];
            if (q != cur && used[q] && age >= 1 && age <= window) {
                p.set[p.nsets] = (unsigned char)q;
                p.age[p.nsets++] = (unsigned char)age;
            }
        }
        p.rslot = b.rslot;
        p.bsum = b.bsum;
        p.out = b.out;
        p.first = b.first;
        p.copies = b.copies;
        p.omarks = b.omarks;
        p.count = b.count;
        p.grid = clear_groups;
        if (!launch(on(DD_K_CLEAR, clear_groups), p))
            return false;
        p.grid = groups;
        for (int k = DD_K_FIND; k <= DD_K_FILL; k++)
            if (!launch(on(k, groups), p))
                return false;
        return true;
    }
};

} // namespace aisx
