// emul_dedup.cpp -- CPU model of the duplicate suppression in device memory (TEST INFRASTRUCTURE, see ../emul/emul.cpp):
// the kernel bodies of gr-ais_amd/csrc/k_dedup.h run one OS thread per lane, driven by the launch plan that drives them on
// the device (DdPlan, k_dedup.h) with host memory in place of device memory.  The lanes of a workgroup are free-running
// threads, so the races on a hash slot, a first record and a copies cell are real here.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_dedup.h"

namespace {

// EmuCtx plus the atomics k_dedup.h needs (aisx_devctx.h has the device's)
struct DdCtx : EmuCtx {
    explicit DdCtx(const EmuCtx& c) : EmuCtx(c) {}
    dd_u64 atomic_cas_u64(dd_u64* p, dd_u64 expect, dd_u64 desired) const
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
};

struct EmuDd {
    explicit EmuDd(const DdPlan& plan) : pl(plan) {}
    DdPlan pl;
    std::vector<dd_u64> ckey, ring;
    std::vector<int> cfirst, ccount, cval, rslot, bsum, count;
    std::vector<HdlcRec> out;
    std::vector<int32_t> first, copies, omarks;
};

bool run(const PlanLaunch& l, const DdParams& p)
{
    run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& ec) {
        DdCtx cx(ec);
        switch (l.kernel) {
        case DD_K_CLEAR: dd_clear_body(cx, p); break;
        case DD_K_FIND: dd_find_body(cx, p); break;
        case DD_K_CLASSIFY: dd_classify_body(cx, p); break;
        case DD_K_ASSIGN: dd_assign_body(cx, p); break;
        case DD_K_FILL: dd_fill_body(cx, p); break;
        }
    });
    return true;
}

} // namespace

extern "C" {

// returns nullptr where aisx_dedup_batch_create returns AISX_ERR_INVALID
void* emu_dd_create(int window, int max_pdus, int length_max)
{
    if (DdPlan::check(window, max_pdus, length_max))
        return nullptr;
    EmuDd* h = new EmuDd(DdPlan(window, max_pdus, length_max));
    const DdPlan& pl = h->pl;
    emu_alloc(h->ckey, pl.ckey);
    emu_alloc(h->ring, pl.ring);
    emu_alloc(h->cfirst, pl.cfirst);
    emu_alloc(h->ccount, pl.ccount);
    emu_alloc(h->cval, pl.cval);
    emu_alloc(h->rslot, pl.rslot);
    emu_alloc(h->bsum, pl.bsum);
    emu_alloc(h->count, pl.count);
    emu_alloc(h->out, pl.out);
    emu_alloc(h->first, pl.first);
    emu_alloc(h->copies, pl.copies);
    emu_alloc(h->omarks, pl.omarks);
    return h;
}

void emu_dd_destroy(void* hv) { delete (EmuDd*)hv; }

void emu_dd_reset(void* hv)
{
    EmuDd* h = (EmuDd*)hv;
    std::fill(h->count.begin(), h->count.end(), 0);
    h->pl.reset();
}

// 0, or -2 where aisx_dedup_batch_process returns AISX_ERR_OUT_OF_RANGE (nothing runs)
int emu_dd_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound,
                   const int32_t* marks, int32_t stamp)
{
    EmuDd* h = (EmuDd*)hv;
    if (!h->pl.stamp_ok(stamp))
        return -2;
    const DdBufs b = { h->ckey.data(),  h->cfirst.data(), h->ccount.data(), h->cval.data(),   h->ring.data(),   h->rslot.data(),
                       h->bsum.data(),  h->out.data(),    h->first.data(),  h->copies.data(), h->omarks.data(), h->count.data() };
    h->pl.process(b, pdus, bytes, npdus, nfound, marks, stamp, run);
    return 0;
}

// the whole of every result buffer, written or not: pdus / first / copies / marks [max_pdus], count [DD_COUNT_WORDS]
// (the bad-input flag cleared here)
void emu_dd_read(void* hv, HdlcRec* pdus, int32_t* first, int32_t* copies, int32_t* marks, int* count)
{
    EmuDd* h = (EmuDd*)hv;
    memcpy(count, h->count.data(), sizeof(int) * DD_COUNT_WORDS);
    h->count[DC_BAD] = 0;
    memcpy(pdus, h->out.data(), sizeof(HdlcRec) * h->pl.out.n);
    memcpy(first, h->first.data(), sizeof(int32_t) * h->pl.first.n);
    memcpy(copies, h->copies.data(), sizeof(int32_t) * h->pl.copies.n);
    memcpy(marks, h->omarks.data(), sizeof(int32_t) * h->pl.omarks.n);
}

// the plan: out[4] = bits, groups, clear_groups, the ring's sets; 0 where it refuses
int emu_dd_plan(int window, int max_pdus, int length_max, long long* out)
{
    if (DdPlan::check(window, max_pdus, length_max))
        return 0;
    const DdPlan pl(window, max_pdus, length_max);
    const long long v[4] = { pl.bits, pl.groups, pl.clear_groups, (long long)(pl.ring.n >> pl.bits) };
    memcpy(out, v, sizeof v);
    return 1;
}

// a key's home slot in a hash of 1 << bits slots (k_dedup.h, dd_home)
unsigned emu_dd_home(unsigned long long key, int bits) { return dd_home(key, bits); }
}
