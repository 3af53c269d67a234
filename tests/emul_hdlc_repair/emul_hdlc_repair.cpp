// emul_hdlc_repair.cpp -- CPU model of the batched HDLC deframer with single-bit repair (TEST INFRASTRUCTURE, see
// ../emul/emul.cpp and ../emul_hdlc/emul_hdlc.cpp): the kernel bodies of gr-ais_amd/csrc/k_hdlc.h run one OS thread per
// lane, driven the way aisx_hdlc.hip drives them on the device -- hdlc_deframe_body<Ctx, true> for a handle with rules,
// the plain body for one without, the marks carried by hdlc_gather_body.
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_hdlc.h"

namespace {

struct EmuHdlcRepair {
    int lmin, lmax, nchan, max_bits, max_pdus, carry_words, rec_cap, byte_cap;
    std::vector<HdlcState> st;
    std::vector<unsigned long long> carry;
    std::vector<HdlcRec> srec, out;
    std::vector<unsigned char> sbytes, out_bytes;
    std::vector<int> cnt, nbytes, sfix, out_fix;
    std::vector<long long> rec_base, byte_base;
    std::vector<HdlcRule> rules;
    std::vector<unsigned short> syn_inv;
    int count[4] = { 0, 0, 0, 0 };
};

} // namespace

extern "C" {

void* emu_hdlcr_create(int lmin, int lmax, int nchan, int max_bits, int max_pdus)
{
    if (lmin < 2 || lmax < lmin || lmax > HD_MAX_OCTETS || nchan < 1 || max_bits < 1 || max_bits > (1 << 28) || max_pdus < 1)
        return nullptr;
    EmuHdlcRepair* h = new EmuHdlcRepair();
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
    // the single-error syndromes: 0x8000 for the frame's last bit, one step of the CRC register per bit before it
    h->syn_inv.assign(65536, 0);
    unsigned s = 0x8000u;
    for (int d = 0; d < 32767; d++) {
        if (!h->syn_inv[s])
            h->syn_inv[s] = (unsigned short)(d + 1);
        s = (s >> 1) ^ ((s & 1u) ? 0x8408u : 0u);
    }
    return h;
}

void emu_hdlcr_destroy(void* hv) { delete (EmuHdlcRepair*)hv; }

// the rules as aisx_hdlc_batch_set_repair takes them, already checked by the caller; nrules == 0: off
void emu_hdlcr_set_repair(void* hv, const HdlcRule* rules, int nrules)
{
    EmuHdlcRepair* h = (EmuHdlcRepair*)hv;
    if (nrules == 0 && !h->rules.empty())
        h->out_fix.assign(h->max_pdus, -1);
    h->rules.assign(rules, rules + nrules);
}

void emu_hdlcr_process(void* hv, const unsigned char* bits, long stride, const int* nbits)
{
    EmuHdlcRepair* h = (EmuHdlcRepair*)hv;
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
        p.syn_inv = h->syn_inv.data();
        p.sfix = h->sfix.data();
        run_grid(h->nchan, 1, HD_T, HD_LDS_BYTES_REPAIR, [&](EmuCtx& cx) { hdlc_deframe_body<EmuCtx, true>(cx, p); });
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
void emu_hdlcr_read(void* hv, HdlcRec* pdus, unsigned char* bytes, int* fix, int* count)
{
    EmuHdlcRepair* h = (EmuHdlcRepair*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(pdus, h->out.data(), sizeof(HdlcRec) * kept);
    memcpy(fix, h->out_fix.data(), sizeof(int) * kept);
    const long long nb = kept ? h->out[kept - 1].offset + h->out[kept - 1].len : 0;
    memcpy(bytes, h->out_bytes.data(), (size_t)nb);
}

int emu_hdlcr_rec_size() { return (int)sizeof(HdlcRec); }
int emu_hdlcr_rule_size() { return (int)sizeof(HdlcRule); }

}
