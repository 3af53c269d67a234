// emul_track.cpp -- CPU model of the vessel table in device memory (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the
// kernel bodies of gr-ais_amd/csrc/k_track.h run one OS thread per lane, driven by the launch plan that drives them on the
// device (TrkPlan, k_track.h) with host memory in place of device memory.  The lanes of a workgroup are free-running
// threads, so the races on a hash slot, a first row and a winner cell are real here.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
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
    explicit EmuTrk(const TrkPlan& plan) : pl(plan) {}
    TrkPlan pl;
    std::vector<int32_t> tab[2], hkey, bkey, gcols;
    std::vector<uint32_t> strs[2], gstrs;
    std::vector<int> hval, bfirst, bval, bj, rslot, bsum, win, changed, count;
};

TrkBufs bufs(EmuTrk* h)
{
    return TrkBufs{ { h->tab[0].data(), h->tab[1].data() }, { h->strs[0].data(), h->strs[1].data() }, h->hkey.data(), h->hval.data(),
                    h->bkey.data(), h->bfirst.data(), h->bval.data(), h->bj.data(), h->rslot.data(), h->bsum.data(), h->win.data(),
                    h->changed.data(), h->gcols.data(), h->gstrs.data(), h->count.data() };
}

// a launch of the plan's: the body of its id
bool run(const PlanLaunch& l, const TrkCall& c)
{
    run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& ec) {
        TrkCtx cx(ec);
        switch (l.kernel) {
        case TRK_K_CLEAR: trk_clear_body(cx, c.p); break;
        case TRK_K_FIND: trk_find_body(cx, c.p); break;
        case TRK_K_CLASSIFY: trk_classify_body(cx, c.p); break;
        case TRK_K_ASSIGN: trk_assign_body(cx, c.p); break;
        case TRK_K_WINNER: trk_winner_body(cx, c.p); break;
        case TRK_K_APPLY: trk_apply_body(cx, c.p); break;
        case TRK_K_KEEP: trk_keep_body(cx, c.p, c.min_stamp); break;
        case TRK_K_COMPACT: trk_compact_body(cx, c.p, c.min_stamp); break;
        case TRK_K_GATHER: trk_gather_body(cx, c.p); break;
        }
    });
    return true;
}

} // namespace

extern "C" {

// returns nullptr where aisx_track_batch_create returns AISX_ERR_INVALID
void* emu_trk_create(int capacity, int max_rows)
{
    if (TrkPlan::check(capacity, max_rows))
        return nullptr;
    EmuTrk* h = new EmuTrk(TrkPlan(capacity, max_rows));
    const TrkPlan& pl = h->pl;
    for (int k = 0; k < 2; k++) {
        emu_alloc(h->tab[k], pl.tab);
        emu_alloc(h->strs[k], pl.strs);
    }
    h->hkey.assign(pl.hkey.n, TRK_EMPTY);
    emu_alloc(h->hval, pl.hval);
    emu_alloc(h->bkey, pl.bkey);
    emu_alloc(h->bfirst, pl.bfirst);
    emu_alloc(h->bval, pl.bval);
    emu_alloc(h->bj, pl.bj);
    emu_alloc(h->rslot, pl.rslot);
    emu_alloc(h->bsum, pl.bsum);
    emu_alloc(h->win, pl.win);
    emu_alloc(h->changed, pl.changed);
    emu_alloc(h->gcols, pl.gcols);
    emu_alloc(h->gstrs, pl.gstrs);
    emu_alloc(h->count, pl.count);
    return h;
}

void emu_trk_destroy(void* hv) { delete (EmuTrk*)hv; }

void emu_trk_process(void* hv, const int32_t* cols, long col_stride, const uint32_t* strs, const HdlcRec* recs, const int* nrows,
                     int32_t stamp)
{
    EmuTrk* h = (EmuTrk*)hv;
    h->pl.process(bufs(h), cols, col_stride, strs, recs, nrows, stamp, run);
}

void emu_trk_expire(void* hv, int32_t min_stamp)
{
    EmuTrk* h = (EmuTrk*)hv;
    h->pl.expire(bufs(h), min_stamp, run);
}

// count [TRK_NCNT] (the bad-input flag cleared here); the whole table, written or not: cols [TRK_NCOL][capacity],
// strs [capacity][MSG_STR]; changed [max_rows]
void emu_trk_read(void* hv, int32_t* cols, char* strs, int* changed, int* count)
{
    EmuTrk* h = (EmuTrk*)hv;
    memcpy(count, h->count.data(), sizeof(int) * TRK_NCNT);
    h->count[TN_BAD] = 0;
    memcpy(cols, h->tab[h->pl.cur].data(), sizeof(int32_t) * h->pl.tab.n);
    memcpy(strs, h->strs[h->pl.cur].data(), sizeof(uint32_t) * h->pl.strs.n);
    memcpy(changed, h->changed.data(), sizeof(int) * h->pl.changed.n);
}

// one cell of the table set from outside (a count just short of saturation cannot be reached by feeding rows)
void emu_trk_poke(void* hv, int col, int vessel, int32_t value)
{
    EmuTrk* h = (EmuTrk*)hv;
    h->tab[h->pl.cur][(size_t)col * h->pl.capacity + vessel] = value;
}

// the gather of aisx_track_batch_read_changed: cols [TRK_NCOL][max_rows], strs [max_rows][MSG_STR]
void emu_trk_gather(void* hv, int32_t* cols, char* strs)
{
    EmuTrk* h = (EmuTrk*)hv;
    h->pl.gather(bufs(h), run);
    memcpy(cols, h->gcols.data(), sizeof(int32_t) * h->pl.gcols.n);
    memcpy(strs, h->gstrs.data(), sizeof(uint32_t) * h->pl.gstrs.n);
}

// the plan: out[7] = hbits, bbits, row_groups, cap_groups, clear_groups, the length of bsum, nbmax; 0 where it refuses
int emu_trk_plan(int capacity, int max_rows, long long* out)
{
    if (TrkPlan::check(capacity, max_rows))
        return 0;
    const TrkPlan pl(capacity, max_rows);
    const long long v[7] = { pl.hbits, pl.bbits, pl.row_groups, pl.cap_groups, pl.clear_groups, (long long)pl.bsum.n, pl.nbmax };
    memcpy(out, v, sizeof v);
    return 1;
}

}
