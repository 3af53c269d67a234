// emul_hdlc.cpp -- CPU model of the batched HDLC deframer, with and without the repair by CRC syndrome (TEST
// INFRASTRUCTURE, see ../emul/emul.cpp): the kernel bodies of gr-ais_amd/csrc/k_hdlc.h run one OS thread per lane under
// the same EmuCtx, driven by the launch plan that drives them on the device (HdlcPlan, k_hdlc.h) with host memory in
// place of device memory.  The tables are the host form's (aisx_framing.cpp, built into this library), as on the device.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/aisx_repair.h"
#include "../../gr-ais_amd/csrc/k_hdlc.h"

namespace {

constexpr int EMU_SCAN_T = 64; // (the device runs HD_SCAN_T threads)

struct EmuHdlc {
    explicit EmuHdlc(const HdlcPlan& plan) : pl(plan) {}
    const HdlcPlan pl;
    std::vector<HdlcState> st;
    std::vector<unsigned long long> carry;
    std::vector<HdlcRec> srec, out;
    std::vector<unsigned char> sbytes, out_bytes;
    std::vector<int> cnt, count, sfix, fix;
    std::vector<long long> base;
    std::vector<HdlcRule> rules;
    std::vector<unsigned short> ev_tab;
    int nrules = 0, events = AISX_HDLC_EV_SINGLE;
};

} // namespace

extern "C" {

// returns nullptr where aisx_hdlc_batch_create returns AISX_ERR_INVALID
void* emu_hdlc_create(int lmin, int lmax, int nchan, int max_bits, int max_pdus)
{
    if (HdlcPlan::check(lmin, lmax, nchan, max_bits, max_pdus))
        return nullptr;
    EmuHdlc* h = new EmuHdlc(HdlcPlan(lmin, lmax, nchan, max_bits, max_pdus, EMU_SCAN_T));
    const HdlcPlan& pl = h->pl;
    emu_alloc(h->st, pl.st);
    emu_alloc(h->carry, pl.carry);
    emu_alloc(h->srec, pl.srec);
    emu_alloc(h->sbytes, pl.sbytes);
    emu_alloc(h->cnt, pl.cnt);
    emu_alloc(h->base, pl.base);
    emu_alloc(h->count, pl.count);
    emu_alloc(h->out, pl.out);
    emu_alloc(h->out_bytes, pl.out_bytes);
    emu_alloc(h->rules, pl.rules);
    emu_alloc(h->sfix, pl.sfix);
    h->fix.assign(pl.fix.n, -1);
    return h;
}

void emu_hdlc_destroy(void* hv) { delete (EmuHdlc*)hv; }

// the rules and the mask as aisx_hdlc_batch_set_repair_events takes them, already checked by the caller; nrules == 0: off
void emu_hdlc_set_repair(void* hv, const HdlcRule* rules, int nrules, int events)
{
    EmuHdlc* h = (EmuHdlc*)hv;
    if (nrules == 0 && h->nrules > 0)
        h->fix.assign(h->fix.size(), -1);
    std::copy(rules, rules + nrules, h->rules.begin());
    h->nrules = nrules;
    h->events = events;
    if (events != AISX_HDLC_EV_SINGLE) {
        h->ev_tab.resize(h->pl.syn.n);
        aisx::hdlc_event_table(events, h->ev_tab.data());
    }
}

void emu_hdlc_process(void* hv, const unsigned char* bits, long stride, const int* nbits)
{
    EmuHdlc* h = (EmuHdlc*)hv;
    const bool single = h->events == AISX_HDLC_EV_SINGLE;
    const HdlcBufs b = { h->st.data(),  h->carry.data(),     h->srec.data(), h->sbytes.data(), h->cnt.data(),
                         h->base.data(), h->count.data(),     h->out.data(),  h->out_bytes.data(), h->fix.data(),
                         h->rules.data(), h->sfix.data(),     single ? aisx::hdlc_syndrome_table() : h->ev_tab.data() };
    h->pl.process(b, bits, stride, nbits, h->nrules, !single, [&](const PlanLaunch& l, const HdlcCall& c) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) {
            switch (l.kernel) {
            case HD_K_DEFRAME: hdlc_deframe_body(cx, c.p); break;
            case HD_K_DEFRAME_REPAIR: hdlc_deframe_body<EmuCtx, true>(cx, c.p); break;
            case HD_K_DEFRAME_EVENTS: hdlc_deframe_body<EmuCtx, true, true>(cx, c.p); break;
            case HD_K_SCAN: hdlc_scan_body(cx, c.s); break;
            case HD_K_GATHER: hdlc_gather_body(cx, c.g); break;
            }
        });
        return true;
    });
}

// count[0] found, [1] kept, [2] bad-count flag (cleared here); records, bytes and (fix != nullptr) marks of the kept ones
void emu_hdlc_read(void* hv, HdlcRec* pdus, unsigned char* bytes, int* fix, int* count)
{
    EmuHdlc* h = (EmuHdlc*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(pdus, h->out.data(), sizeof(HdlcRec) * kept);
    if (fix)
        memcpy(fix, h->fix.data(), sizeof(int) * kept);
    const long long nb = kept ? h->out[kept - 1].offset + h->out[kept - 1].len : 0;
    memcpy(bytes, h->out_bytes.data(), (size_t)nb);
}

// the host form's single-error table (not part of the C ABI), for the tests that compare tables with it
void emu_hdlc_syndrome_table(unsigned short* out) { memcpy(out, aisx::hdlc_syndrome_table(), sizeof(unsigned short) * 65536); }

int emu_hdlc_rec_size() { return (int)sizeof(HdlcRec); }
int emu_hdlc_rule_size() { return (int)sizeof(HdlcRule); }

// the plan at the device's constants: out[4] = carry_words, rec_cap, byte_cap, out_bytes_cap; 0 where it refuses
int emu_hdlc_plan(int lmin, int lmax, int nchan, int max_bits, int max_pdus, long long* out)
{
    if (HdlcPlan::check(lmin, lmax, nchan, max_bits, max_pdus))
        return 0;
    const HdlcPlan pl(lmin, lmax, nchan, max_bits, max_pdus);
    const long long v[4] = { pl.carry_words, pl.rec_cap, pl.byte_cap, pl.out_bytes_cap };
    memcpy(out, v, sizeof v);
    return 1;
}

}
