// emul_hdlc_events.cpp -- CPU model of the batched HDLC deframer with the error-event repair (TEST INFRASTRUCTURE, see
// ../emul/emul.cpp and ../emul_hdlc_repair/emul_hdlc_repair.cpp): the kernel bodies of gr-ais_amd/csrc/k_hdlc.h run one
// OS thread per lane, driven the way aisx_hdlc.hip drives them on the device -- hdlc_deframe_body<Ctx, true, true> with
// the mask's table for a handle with rules and a mask that is not the single event alone, hdlc_deframe_body<Ctx, true>
// with the single-error table for the single event, the plain body for a handle without rules, the marks carried by
// hdlc_gather_body.  The tables are the host form's (aisx_framing.cpp, built into this library), as on the device.
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/aisx_repair.h"
#include "../../gr-ais_amd/csrc/k_hdlc.h"

namespace {

struct EmuHdlcEvents {
    int lmin, lmax, nchan, max_bits, max_pdus, carry_words, rec_cap, byte_cap;
    std::vector<HdlcState> st;
    std::vector<unsigned long long> carry;
    std::vector<HdlcRec> srec, out;
    std::vector<unsigned char> sbytes, out_bytes;
    std::vector<int> cnt, nbytes, sfix, out_fix;
    std::vector<long long> rec_base, byte_base;
    std::vector<HdlcRule> rules;
    std::vector<unsigned short> syn_inv, ev_tab;
    int events = AISX_HDLC_EV_SINGLE;
    int count[4] = { 0, 0, 0, 0 };
};

} // namespace

extern "C" {

void* emu_hdlce_create(int lmin, int lmax, int nchan, int max_bits, int max_pdus)
{
    if (lmin < 2 || lmax < lmin || lmax > HD_MAX_OCTETS || nchan < 1 || max_bits < 1 || max_bits > (1 << 28) || max_pdus < 1)
        return nullptr;
    EmuHdlcEvents* h = new EmuHdlcEvents();
    h->lmin = lmin;
    h->lmax = lmax;
    h->nchan = nchan;
    h->max_bits = max_bits;
    h->max_pdus = max_pdus;
    const long long span = 8LL * (lmax + 1) + max_bits;
    h->carry_words = (8 * (lmax + 1) + 63) / 64;
    h->rec_cap = (int)(span / (8LL * lmin + 1) + 2);
    h->byte_cap = (int)(span / 8 + 8);
    h->st.assign(nchan, HdlcState{});
    h->carry.assign((size_t)nchan * h->carry_words, 0);
    h->srec.resize((size_t)nchan * h->rec_cap);
    h->sbytes.resize((size_t)nchan * h->byte_cap);
    h->sfix.assign((size_t)nchan * h->rec_cap, -7);
    h->cnt.assign(nchan, 0);
    h->nbytes.assign(nchan, 0);
    h->rec_base.assign(nchan, 0);
    h->byte_base.assign(nchan, 0);
    h->out.resize(max_pdus);
    h->out_fix.assign(max_pdus, -1);
    h->out_bytes.resize((size_t)max_pdus * (lmax - 1) + 1);
    h->syn_inv.assign(aisx::hdlc_syndrome_table(), aisx::hdlc_syndrome_table() + 65536);
    return h;
}

void emu_hdlce_destroy(void* hv) { delete (EmuHdlcEvents*)hv; }

// the rules and the mask as aisx_hdlc_batch_set_repair_events takes them, already checked by the caller; nrules == 0: off
void emu_hdlce_set_repair(void* hv, const HdlcRule* rules, int nrules, int events)
{
    EmuHdlcEvents* h = (EmuHdlcEvents*)hv;
    if (nrules == 0 && !h->rules.empty())
        h->out_fix.assign(h->max_pdus, -1);
    h->rules.assign(rules, rules + nrules);
    h->events = events;
    if (events != AISX_HDLC_EV_SINGLE) {
        h->ev_tab.resize(65536);
        aisx::hdlc_event_table(events, h->ev_tab.data());
    }
}

void emu_hdlce_process(void* hv, const unsigned char* bits, long stride, const int* nbits)
{
    EmuHdlcEvents* h = (EmuHdlcEvents*)hv;
    const bool repair = !h->rules.empty();
    HdlcParams p;
    p.bits = bits;
    p.stride = stride;
    p.nbits = nbits;
    p.max_bits = h->max_bits;
    p.lmin = h->lmin;
    p.lmax = h->lmax;
    p.st = h->st.data();
    p.carry = h->carry.data();
    p.carry_words = h->carry_words;
    p.srec = h->srec.data();
    p.rec_cap = h->rec_cap;
    p.sbytes = h->sbytes.data();
    p.byte_cap = h->byte_cap;
    p.cnt = h->cnt.data();
    p.nbytes = h->nbytes.data();
    p.flags = h->count + 2;
    if (repair) {
        p.rules = h->rules.data();
        p.nrules = (int)h->rules.size();
        p.sfix = h->sfix.data();
        if (h->events == AISX_HDLC_EV_SINGLE) {
            p.syn_inv = h->syn_inv.data();
            run_grid(h->nchan, 1, HD_T, HD_LDS_BYTES_REPAIR, [&](EmuCtx& cx) { hdlc_deframe_body<EmuCtx, true>(cx, p); });
        } else {
            p.syn_inv = h->ev_tab.data();
            run_grid(h->nchan, 1, HD_T, HD_LDS_BYTES_REPAIR, [&](EmuCtx& cx) { hdlc_deframe_body<EmuCtx, true, true>(cx, p); });
        }
    } else {
        run_grid(h->nchan, 1, HD_T, HD_LDS_BYTES, [&](EmuCtx& cx) { hdlc_deframe_body(cx, p); });
    }
    HdlcScanParams s;
    s.cnt = p.cnt;
    s.nbytes = p.nbytes;
    s.rec_base = h->rec_base.data();
    s.byte_base = h->byte_base.data();
    s.nchan = h->nchan;
    s.max_pdus = h->max_pdus;
    s.count = h->count;
    run_grid(1, 1, 64, 2 * 64 * 8, [&](EmuCtx& cx) { hdlc_scan_body(cx, s); }); // (the device runs HD_SCAN_T threads)
    HdlcGatherParams g;
    g.srec = h->srec.data();
    g.rec_cap = h->rec_cap;
    g.sbytes = h->sbytes.data();
    g.byte_cap = h->byte_cap;
    g.cnt = p.cnt;
    g.nbytes = p.nbytes;
    g.rec_base = s.rec_base;
    g.byte_base = s.byte_base;
    g.max_pdus = h->max_pdus;
    g.out = h->out.data();
    g.out_bytes = h->out_bytes.data();
    if (repair) {
        g.sfix = h->sfix.data();
        g.out_fix = h->out_fix.data();
    }
    run_grid(h->nchan, 1, HD_T, 64, [&](EmuCtx& cx) { hdlc_gather_body(cx, g); });
}

// count[0] found, [1] kept, [2] bad-count flag (cleared here); records, bytes and marks of the kept ones
void emu_hdlce_read(void* hv, HdlcRec* pdus, unsigned char* bytes, int* fix, int* count)
{
    EmuHdlcEvents* h = (EmuHdlcEvents*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(pdus, h->out.data(), sizeof(HdlcRec) * kept);
    memcpy(fix, h->out_fix.data(), sizeof(int) * kept);
    const long long nb = kept ? h->out[kept - 1].offset + h->out[kept - 1].len : 0;
    memcpy(bytes, h->out_bytes.data(), (size_t)nb);
}

// the host form's single-error table (not part of the C ABI), for the test that compares the event tables with it
void emu_hdlce_syndrome_table(unsigned short* out) { memcpy(out, aisx::hdlc_syndrome_table(), sizeof(unsigned short) * 65536); }

int emu_hdlce_rec_size() { return (int)sizeof(HdlcRec); }
int emu_hdlce_rule_size() { return (int)sizeof(HdlcRule); }

}
