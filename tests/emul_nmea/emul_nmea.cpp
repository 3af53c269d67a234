// emul_nmea.cpp -- CPU model of the batched NMEA armouring (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// bodies of gr-ais_amd/csrc/k_nmea.h run one OS thread per lane under the same EmuCtx, driven the way aisx_nmea.hip
// drives them on the device (host memory in place of device memory).
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_nmea.h"

namespace {

constexpr int EMU_SCAN_T = 128;  // (the device runs NM_SCAN_T threads: two waves keep the cross-wave scan in play)
constexpr int EMU_W_T = 128;
constexpr int EMU_W_GROUPS = 3;  // (the device takes up to NM_W_MAX_GROUPS: a few waves make every wave loop)

struct EmuNmea {
    int nchan, max_pdus, lmax;
    long long text_cap;
    std::vector<char> desig, text;
    std::vector<unsigned char> dlen;
    std::vector<HdlcRec> out;
    int count[4] = { 0, 0, 0, 0 };
};

} // namespace

extern "C" {

// the argument checks and the text capacity are the product's (aisx_nmea_batch_create); returns nullptr where it
// returns AISX_ERR_INVALID
void* emu_nmea_create(const char* const* designators, int nchan, int max_pdus, int length_max, long text_cap)
{
    if (!designators || nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > NM_MAX_OCTETS || text_cap < 0)
        return nullptr;
    int max_dlen = 0;
    for (int c = 0; c < nchan; c++) {
        const size_t n = designators[c] ? strnlen(designators[c], NM_DESIG + 1) : NM_DESIG + 1;
        if (n > (size_t)NM_DESIG)
            return nullptr;
        max_dlen = std::max(max_dlen, (int)n);
    }
    EmuNmea* h = new EmuNmea();
    h->nchan = nchan;
    h->max_pdus = max_pdus;
    h->lmax = length_max;
    const long long worst = (long long)max_pdus * (nm_text_len(length_max - 1, max_dlen) + 1);
    h->text_cap = text_cap == 0 || text_cap > worst ? worst : text_cap;
    h->desig.assign((size_t)nchan * NM_DESIG, 0);
    h->dlen.assign(nchan, 0);
    for (int c = 0; c < nchan; c++) {
        h->dlen[c] = (unsigned char)strlen(designators[c]);
        memcpy(h->desig.data() + (size_t)c * NM_DESIG, designators[c], h->dlen[c]);
    }
    h->out.resize(max_pdus);
    h->text.assign((size_t)h->text_cap, 0);
    return h;
}

void emu_nmea_destroy(void* hv) { delete (EmuNmea*)hv; }

long emu_nmea_text_cap(void* hv) { return (long)((EmuNmea*)hv)->text_cap; }

int emu_nmea_text_len(int len, int dlen) { return nm_text_len(len, dlen); }

void emu_nmea_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound)
{
    EmuNmea* h = (EmuNmea*)hv;
    NmeaScanParams s;
    s.in = pdus;
    s.npdus = npdus;
    s.nfound = nfound;
    s.dlen = h->dlen.data();
    s.nchan = h->nchan;
    s.max_pdus = h->max_pdus;
    s.max_len = h->lmax - 1;
    s.text_cap = h->text_cap;
    s.out = h->out.data();
    s.count = h->count;
    run_grid(1, 1, EMU_SCAN_T, (2 * (EMU_SCAN_T / 64) + 2) * 4, [&](EmuCtx& cx) { nmea_scan_body(cx, s); });
    NmeaWriteParams w;
    w.in = pdus;
    w.bytes = bytes;
    w.out = h->out.data();
    w.count = h->count;
    w.desig = h->desig.data();
    w.dlen = h->dlen.data();
    w.text = h->text.data();
    w.nwaves = EMU_W_GROUPS * (EMU_W_T / 64);
    run_grid(EMU_W_GROUPS, 1, EMU_W_T, 0, [&](EmuCtx& cx) { nmea_write_body(cx, w); });
}

// count[0] found, [1] records written, [2] bad-input flag (cleared here); the records written and the text up to
// the last one's end
void emu_nmea_read(void* hv, HdlcRec* recs, char* text, int* count)
{
    EmuNmea* h = (EmuNmea*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    const int kept = h->count[1];
    memcpy(recs, h->out.data(), sizeof(HdlcRec) * kept);
    const HdlcRec* last = kept ? &h->out[kept - 1] : nullptr;
    const long long nt = last ? last->offset + last->len + (last->len > 0) : 0;
    memcpy(text, h->text.data(), (size_t)nt);
}

}
