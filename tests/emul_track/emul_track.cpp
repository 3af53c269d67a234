// emul_track.cpp -- CPU model of the vessel table in device memory (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the
// kernel bodies of gr-ais_amd/csrc/k_track.h run one OS thread per lane, driven the way aisx_track.hip drives them on the
// device (host memory in place of device memory).  The lanes of a workgroup are free-running threads, so the races on a
// hash slot, a first row and a winner cell are real here.
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_track.h"

namespace {

// EmuCtx plus the atomics k_track.h needs (aisx_devctx.h has the device's)
struct TrkCtx : EmuCtx {
    explicit TrkCtx(const EmuCtx& c) : EmuCtx(c) {}
    int atomic_cas_i32(int* p, int expect, int desired) const
    {
        __atomic_compare_exchange_n(p, &expect, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expect; // (the value found, as atomicCAS)
    }
    int atomic_min_i32(int* p, int v) const
    {
        int old = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
            ;
        return old;
    }
    int atomic_max_i32(int* p, int v) const
    {
        int old = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
            ;
        return old;
    }
};

struct EmuTrk {
    int capacity, max_rows, hbits, bbits, row_groups, cap_groups, cur = 0;
    std::vector<int32_t> tab[2], hkey, bkey, gcols;
    std::vector<uint32_t> strs[2], gstrs;
    std::vector<int> hval, bfirst, bval, bj, rslot, bsum, win, changed;
    int count[TRK_COUNT_WORDS] = {};
};

TrkParams params(EmuTrk* h)
{
    TrkParams p = {};
    p.capacity = h->capacity;
    p.max_rows = h->max_rows;
    p.tab = h->tab[h->cur].data();
    p.strs = h->strs[h->cur].data();
    p.hkey = h->hkey.data();
    p.hval = h->hval.data();
    p.hbits = h->hbits;
    p.bkey = h->bkey.data();
    p.bfirst = h->bfirst.data();
    p.bval = h->bval.data();
    p.bj = h->bj.data();
    p.bbits = h->bbits;
    p.rslot = h->rslot.data();
    p.bsum = h->bsum.data();
    p.nbmax = std::max(h->row_groups, h->cap_groups);
    p.win = h->win.data();
    p.changed = h->changed.data();
    p.count = h->count;
    return p;
}

template <class Body>
void run(int groups, Body body)
{
    run_grid(groups, 1, TRK_T, TRK_LDS_BYTES, [&](EmuCtx& cx) {
        TrkCtx tc(cx);
        body(tc);
    });
}

} // namespace

extern "C" {

// the argument checks are the product's (aisx_track_batch_create); returns nullptr where it returns AISX_ERR_INVALID
void* emu_trk_create(int capacity, int max_rows)
{
    if (capacity < 1 || capacity > TRK_MAX || max_rows < 1 || max_rows > TRK_MAX)
        return nullptr;
    EmuTrk* h = new EmuTrk();
    h->capacity = capacity;
    h->max_rows = max_rows;
    h->hbits = trk_hash_bits(capacity);
    h->bbits = trk_hash_bits(max_rows);
    h->row_groups = (max_rows + TRK_T - 1) / TRK_T;
    h->cap_groups = (capacity + TRK_T - 1) / TRK_T;
    const size_t H = (size_t)1 << h->hbits, B = (size_t)1 << h->bbits, R = (size_t)max_rows, C = (size_t)capacity;
    const int junk = 0x5a5a5a5a; // (what is not written shows)
    for (int k = 0; k < 2; k++) {
        h->tab[k].assign(TRK_NCOL * C, junk);
        h->strs[k].assign(MSG_STR_WORDS * C, 0x5a5a5a5au);
    }
    h->hkey.assign(H, TRK_EMPTY);
    h->hval.assign(H, junk);
    h->bkey.assign(B, junk);
    h->bfirst.assign(B, junk);
    h->bval.assign(B, junk);
    h->bj.assign(B, junk);
    h->rslot.assign(R, junk);
    h->bsum.assign(2 * (size_t)std::max(h->row_groups, h->cap_groups), junk);
    h->win.assign(TRK_NWIN * R, junk);
    h->changed.assign(R, junk);
    h->gcols.assign(TRK_NCOL * R, junk);
    h->gstrs.assign(MSG_STR_WORDS * R, 0x5a5a5a5au);
    return h;
}

void emu_trk_destroy(void* hv) { delete (EmuTrk*)hv; }

void emu_trk_process(void* hv, const int32_t* cols, long col_stride, const uint32_t* strs, const HdlcRec* recs, const int* nrows,
                     int32_t stamp)
{
    EmuTrk* h = (EmuTrk*)hv;
    TrkParams p = params(h);
    p.in_cols = cols;
    p.in_stride = col_stride;
    p.in_strs = strs;
    p.in_recs = recs;
    p.nrows = nrows;
    p.stamp = stamp;
    p.grid = h->row_groups;
    run(h->row_groups, [&](TrkCtx& cx) { trk_clear_body(cx, p); });
    run(h->row_groups, [&](TrkCtx& cx) { trk_find_body(cx, p); });
    run(h->row_groups, [&](TrkCtx& cx) { trk_classify_body(cx, p); });
    run(h->row_groups, [&](TrkCtx& cx) { trk_assign_body(cx, p); });
    run(h->row_groups, [&](TrkCtx& cx) { trk_winner_body(cx, p); });
    run(h->row_groups, [&](TrkCtx& cx) { trk_apply_body(cx, p); });
}

void emu_trk_expire(void* hv, int32_t min_stamp)
{
    EmuTrk* h = (EmuTrk*)hv;
    TrkParams p = params(h);
    p.tab2 = h->tab[h->cur ^ 1].data();
    p.strs2 = h->strs[h->cur ^ 1].data();
    p.grid = h->cap_groups;
    run(h->cap_groups, [&](TrkCtx& cx) { trk_keep_body(cx, p, min_stamp); });
    run(h->cap_groups, [&](TrkCtx& cx) { trk_compact_body(cx, p, min_stamp); });
    h->cur ^= 1;
}

// count [TRK_NCNT] (the bad-input flag cleared here); the whole table, written or not: cols [TRK_NCOL][capacity],
// strs [capacity][MSG_STR]; changed [max_rows]
void emu_trk_read(void* hv, int32_t* cols, char* strs, int* changed, int* count)
{
    EmuTrk* h = (EmuTrk*)hv;
    memcpy(count, h->count, sizeof(int) * TRK_NCNT);
    h->count[TN_BAD] = 0;
    memcpy(cols, h->tab[h->cur].data(), sizeof(int32_t) * h->tab[h->cur].size());
    memcpy(strs, h->strs[h->cur].data(), sizeof(uint32_t) * h->strs[h->cur].size());
    memcpy(changed, h->changed.data(), sizeof(int) * h->changed.size());
}

// one cell of the table set from outside (a count just short of saturation cannot be reached by feeding rows)
void emu_trk_poke(void* hv, int col, int vessel, int32_t value)
{
    EmuTrk* h = (EmuTrk*)hv;
    h->tab[h->cur][(size_t)col * h->capacity + vessel] = value;
}

// the gather of aisx_track_batch_read_changed: cols [TRK_NCOL][max_rows], strs [max_rows][MSG_STR]
void emu_trk_gather(void* hv, int32_t* cols, char* strs)
{
    EmuTrk* h = (EmuTrk*)hv;
    TrkParams p = params(h);
    p.tab2 = h->gcols.data();
    p.strs2 = h->gstrs.data();
    p.grid = h->row_groups;
    run(h->row_groups, [&](TrkCtx& cx) { trk_gather_body(cx, p); });
    memcpy(cols, h->gcols.data(), sizeof(int32_t) * h->gcols.size());
    memcpy(strs, h->gstrs.data(), sizeof(uint32_t) * h->gstrs.size());
}

}
