// emul_nmea_parse.cpp -- CPU model of the batched NMEA parser (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// bodies of gr-ais_amd/csrc/k_nmea_parse.h run one OS thread per lane under the same EmuCtx, driven by the launch plan that
// drives them on the device (NmpPlan, k_nmea_parse.h: its four grids, ngroups and nwaves as it sets them between the
// launches) with host memory in place of device memory.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_nmea_parse.h"

namespace {

constexpr int EMU_T = 128;      // (the device runs NP_T threads: two waves keep the cross-wave scans in play)
constexpr int EMU_SCAN_T = 128; // (the device runs NP_SCAN_T)
constexpr int EMU_GROUPS = 3;   // (the device takes up to NP_MAX_GROUPS: a few make every strided loop turn)

struct EmuNmp {
    explicit EmuNmp(NmpPlan&& plan) : pl(std::move(plan)) {}
    const NmpPlan pl;
    std::vector<unsigned char> lcarry, gcarry, bytes;
    std::vector<NmpState> st;
    std::vector<int> tcount, toff, meta, cidx, aux, count, mlen, tl, bstat;
    std::vector<long long> lend, pos, tm, times, tlb;
    std::vector<NmpKey> key;
    std::vector<HdlcRec> rec;
    std::vector<NmpNext> next;
};

void emu_nmp_clear(EmuNmp* h)
{
    emu_alloc(h->st, h->pl.st);
    emu_alloc(h->meta, h->pl.meta);
    emu_alloc(h->count, h->pl.count);
}

} // namespace

extern "C" {

// returns nullptr where aisx_nmea_parse_batch_create returns AISX_ERR_INVALID
void* emu_nmp_create(const char* const* designators, int nchan, int length_max, int max_line, int flags, long max_bytes,
                     int max_lines, int max_pdus)
{
    if (NmpPlan::check(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus) ||
        nm_bad_designator(designators, nchan) >= 0)
        return nullptr;
    EmuNmp* h = new EmuNmp(NmpPlan(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus, EMU_T, EMU_SCAN_T,
                                   EMU_GROUPS));
    const NmpPlan& pl = h->pl;
    emu_alloc(h->lcarry, pl.lcarry);
    emu_alloc(h->gcarry, pl.gcarry);
    emu_alloc(h->bytes, pl.bytes);
    emu_alloc(h->tcount, pl.tcount);
    emu_alloc(h->toff, pl.toff);
    emu_alloc(h->cidx, pl.cidx);
    emu_alloc(h->mlen, pl.mlen);
    emu_alloc(h->tl, pl.tl);
    emu_alloc(h->tlb, pl.tlb);
    emu_alloc(h->bstat, pl.bstat);
    emu_alloc(h->aux, pl.aux);
    emu_alloc(h->lend, pl.lend);
    emu_alloc(h->pos, pl.pos);
    emu_alloc(h->tm, pl.tm);
    emu_alloc(h->times, pl.times);
    emu_alloc(h->key, pl.key);
    emu_alloc(h->rec, pl.rec);
    emu_alloc(h->next, pl.next);
    emu_nmp_clear(h);
    return h;
}

void emu_nmp_destroy(void* hv) { delete (EmuNmp*)hv; }
void emu_nmp_reset(void* hv) { emu_nmp_clear((EmuNmp*)hv); }

// `text` must hold *nbytes bytes when that count is in range; nothing else of it is read
void emu_nmp_process(void* hv, const unsigned char* text, const long long* nbytes)
{
    EmuNmp* h = (EmuNmp*)hv;
    const NmpBufs b = { h->pl.desig_host.data(), h->pl.dlen_host.data(), h->st.data(), h->lcarry.data(), h->gcarry.data(),
                        h->tcount.data(), h->toff.data(), h->meta.data(), h->lend.data(), h->key.data(), h->pos.data(), h->tm.data(),
                        h->cidx.data(), h->mlen.data(), h->tl.data(), h->tlb.data(), h->bstat.data(), h->rec.data(), h->aux.data(),
                        h->times.data(), h->bytes.data(), h->count.data(), h->next.data() };
    const int T = h->pl.threads; // (the scans are told the threads of the kernels whose tile sums they scan)
    h->pl.process(b, text, nbytes, [&](const PlanLaunch& l, const NmpParams& p) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) {
            switch (l.kernel) {
            case NP_K_COUNT: nmp_count_body(cx, p); break;
            case NP_K_SCAN: nmp_scan_body(cx, p, T); break;
            case NP_K_INDEX: nmp_index_body(cx, p); break;
            case NP_K_PARSE: nmp_parse_body(cx, p); break;
            case NP_K_GCOUNT: nmp_gcount_body(cx, p); break;
            case NP_K_GSCAN1: nmp_gscan1_body(cx, p, T); break;
            case NP_K_GCOMPACT: nmp_gcompact_body(cx, p); break;
            case NP_K_GMSG: nmp_gmsg_body(cx, p); break;
            case NP_K_GSCAN2: nmp_gscan2_body(cx, p, T); break;
            case NP_K_GPLACE: nmp_gplace_body(cx, p); break;
            case NP_K_WRITE: nmp_write_body(cx, p); break;
            case NP_K_CARRY: nmp_carry_body(cx, p); break;
            }
        });
        return true;
    });
}

// counts [NP_NCNT] (the bad-input flag is cleared here), the records kept, their bytes and times
void emu_nmp_read(void* hv, HdlcRec* recs, unsigned char* bytes, long long* times, int* counts)
{
    EmuNmp* h = (EmuNmp*)hv;
    for (int k = 0; k < NP_NCNT; k++)
        counts[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(recs, h->rec.data(), sizeof(HdlcRec) * kept);
    memcpy(times, h->times.data(), sizeof(long long) * kept);
    const long long nb = kept ? h->rec[kept - 1].offset + h->rec[kept - 1].len : 0;
    memcpy(bytes, h->bytes.data(), (size_t)nb);
}

// the plan at the device's constants: out[6] = ntiles, nlt, tile_groups, line_groups, ltile_groups, pdu_groups, then
// (grid, ngroups, nwaves) of each of the call's launches in order, out[6 + 3 * NP_NKERNELS] in all; 0 where it refuses
int emu_nmp_plan(const char* const* designators, int nchan, int length_max, int max_line, int flags, long max_bytes, int max_lines,
                 int max_pdus, long long* out)
{
    if (NmpPlan::check(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus) ||
        nm_bad_designator(designators, nchan) >= 0)
        return 0;
    const NmpPlan pl(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus);
    const long long v[6] = { pl.ntiles, pl.nlt, pl.tile_groups, pl.line_groups, pl.ltile_groups, pl.pdu_groups };
    memcpy(out, v, sizeof v);
    int k = 0;
    pl.process(NmpBufs{}, nullptr, nullptr, [&](const PlanLaunch& l, const NmpParams& p) {
        if (l.kernel != k) // (the kernels in their order)
            return false;
        long long* o = out + 6 + 3 * k++;
        o[0] = l.gx;
        o[1] = p.ngroups;
        o[2] = p.nwaves;
        return true;
    });
    return k == NP_NKERNELS;
}

}
