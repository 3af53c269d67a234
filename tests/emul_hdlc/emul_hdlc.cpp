// emul_hdlc.cpp -- CPU model of the batched HDLC deframer (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// bodies of gr-ais_amd/csrc/k_hdlc.h run one OS thread per lane under the same EmuCtx, driven the way
// aisx_hdlc.hip drives them on the device (host memory in place of device memory).
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_hdlc.h"

namespace {

struct EmuHdlc {
    int lmin, lmax, nchan, max_bits, max_pdus, carry_words, rec_cap, byte_cap;
    std::vector<HdlcState> st;
    std::vector<unsigned long long> carry;
    std::vector<HdlcRec> srec, out;
    std::vector<unsigned char> sbytes, out_bytes;
    std::vector<int> cnt, nbytes;
    std::vector<long long> rec_base, byte_base;
    int count[4] = { 0, 0, 0, 0 };
};

} // namespace

extern "C" {

// the argument checks are the product's (aisx_hdlc_batch_create); returns nullptr where it returns AISX_ERR_INVALID
void* emu_hdlc_create(int lmin, int lmax, int nchan, int max_bits, int max_pdus)
{
    if (lmin < 2 || lmax < lmin || lmax > HD_MAX_OCTETS || nchan < 1 || max_bits < 1 || max_bits > (1 << 28) || max_pdus < 1)
        return nullptr;
    EmuHdlc* h = new EmuHdlc();
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
    h->cnt.assign(nchan, 0);
    h->nbytes.assign(nchan, 0);
    h->rec_base.assign(nchan, 0);
    h->byte_base.assign(nchan, 0);
    h->out.resize(max_pdus);
    h->out_bytes.resize((size_t)max_pdus * (lmax - 1) + 1);
    return h;
}

void emu_hdlc_destroy(void* hv) { delete (EmuHdlc*)hv; }

void emu_hdlc_process(void* hv, const unsigned char* bits, long stride, const int* nbits)
{
    EmuHdlc* h = (EmuHdlc*)hv;
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
    run_grid(h->nchan, 1, HD_T, HD_LDS_BYTES, [&](EmuCtx& cx) { hdlc_deframe_body(cx, p); });
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
    run_grid(h->nchan, 1, HD_T, 64, [&](EmuCtx& cx) { hdlc_gather_body(cx, g); });
}

// count[0] found, [1] kept, [2] bad-count flag (cleared here); records and bytes of the kept ones
void emu_hdlc_read(void* hv, HdlcRec* pdus, unsigned char* bytes, int* count)
{
    EmuHdlc* h = (EmuHdlc*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(pdus, h->out.data(), sizeof(HdlcRec) * kept);
    const long long nb = kept ? h->out[kept - 1].offset + h->out[kept - 1].len : 0;
    memcpy(bytes, h->out_bytes.data(), (size_t)nb);
}

int emu_hdlc_rec_size() { return (int)sizeof(HdlcRec); }

}
