// emul_nmea_parse.cpp -- CPU model of the batched NMEA parser (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// bodies of gr-ais_amd/csrc/k_nmea_parse.h run one OS thread per lane under the same EmuCtx, driven the way
// aisx_nmea_parse.hip drives them on the device (host memory in place of device memory).
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_nmea_parse.h"

namespace {

constexpr int EMU_T = 128;      // (the device runs NP_T threads: two waves keep the cross-wave scans in play)
constexpr int EMU_SCAN_T = 128; // (the device runs NP_SCAN_T)
constexpr int EMU_GROUPS = 3;   // (the device takes up to NP_MAX_GROUPS: a few make every strided loop turn)

struct EmuNmp {
    int nchan, lmax, max_line, flags, max_lines, max_pdus;
    long long max_bytes;
    std::vector<char> desig;
    std::vector<unsigned char> dlen, lcarry, gcarry, bytes;
    std::vector<NmpState> st;
    std::vector<int> tcount, toff, meta, cidx, aux, count, mlen, tl, bstat;
    std::vector<long long> lend, pos, tm, times, tlb;
    std::vector<NmpKey> key;
    std::vector<HdlcRec> rec;
    NmpNext next;
};

void emu_nmp_clear(EmuNmp* h)
{
    h->st.assign(2, NmpState{});
    h->meta.assign(NP_M_N, 0);
    h->count.assign(NP_NCNT, 0);
    h->next = NmpNext{};
}

} // namespace

extern "C" {

// (the arguments are taken as they come: the product's checks are the product's, aisx_nmea_parse_batch_create)
void* emu_nmp_create(const char* const* designators, int nchan, int length_max, int max_line, int flags, long max_bytes,
                     int max_lines, int max_pdus)
{
    EmuNmp* h = new EmuNmp();
    h->nchan = nchan;
    h->lmax = length_max;
    h->max_line = max_line;
    h->flags = flags;
    h->max_bytes = max_bytes;
    h->max_lines = max_lines;
    h->max_pdus = max_pdus;
    h->desig.assign((size_t)nchan * NM_DESIG, 0);
    h->dlen.assign(nchan, 0);
    for (int c = 0; c < nchan; c++) {
        h->dlen[c] = (unsigned char)strlen(designators[c]);
        memcpy(h->desig.data() + (size_t)c * NM_DESIG, designators[c], h->dlen[c]);
    }
    const size_t ntiles = (size_t)((max_bytes + EMU_T * NP_CHUNK - 1) / (EMU_T * NP_CHUNK));
    h->lcarry.assign(2 * (size_t)max_line, 0);
    h->gcarry.assign(2 * (size_t)NP_GMAX * max_line, 0);
    h->bytes.assign((size_t)max_pdus * (length_max - 1), 0);
    h->tcount.assign(ntiles, 0);
    h->toff.assign(ntiles, 0);
    h->cidx.assign(max_lines, 0);
    h->mlen.assign((size_t)max_lines + NP_GMAX, 0);
    h->tl.assign(((size_t)max_lines + NP_GMAX + EMU_T - 1) / EMU_T, 0);
    h->tlb.assign(h->tl.size(), 0);
    h->bstat.assign((size_t)NP_MAX_GROUPS * 8, 0);
    h->aux.assign(max_pdus, 0);
    h->lend.assign(max_lines, 0);
    h->pos.assign(max_lines, 0);
    h->tm.assign(max_lines, 0);
    h->times.assign(max_pdus, 0);
    h->key.assign(max_lines, NmpKey{});
    h->rec.assign(max_pdus, HdlcRec{});
    emu_nmp_clear(h);
    return h;
}

void emu_nmp_destroy(void* hv) { delete (EmuNmp*)hv; }
void emu_nmp_reset(void* hv) { emu_nmp_clear((EmuNmp*)hv); }

// `text` must hold *nbytes bytes when that count is in range; nothing else of it is read
void emu_nmp_process(void* hv, const unsigned char* text, const long long* nbytes)
{
    EmuNmp* h = (EmuNmp*)hv;
    NmpParams p;
    p.text = text;
    p.nbytes = nbytes;
    p.max_bytes = h->max_bytes;
    p.max_lines = h->max_lines;
    p.max_pdus = h->max_pdus;
    p.max_len = h->lmax - 1;
    p.max_line = h->max_line;
    p.flags = h->flags;
    p.nchan = h->nchan;
    p.desig = h->desig.data();
    p.dlen = h->dlen.data();
    p.st = h->st.data();
    p.lcarry = h->lcarry.data();
    p.gcarry = h->gcarry.data();
    p.tcount = h->tcount.data();
    p.toff = h->toff.data();
    p.meta = h->meta.data();
    p.lend = h->lend.data();
    p.key = h->key.data();
    p.pos = h->pos.data();
    p.tm = h->tm.data();
    p.cidx = h->cidx.data();
    p.mlen = h->mlen.data();
    p.tl = h->tl.data();
    p.tlb = h->tlb.data();
    p.bstat = h->bstat.data();
    p.rec = h->rec.data();
    p.aux = h->aux.data();
    p.times = h->times.data();
    p.bytes = h->bytes.data();
    p.count = h->count.data();
    p.next = &h->next;
    p.ngroups = EMU_GROUPS;
    p.nwaves = EMU_GROUPS * (EMU_T / 64);
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_count_body(cx, p); });
    run_grid(1, 1, EMU_SCAN_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_scan_body(cx, p, EMU_T); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_index_body(cx, p); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_parse_body(cx, p); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gcount_body(cx, p); });
    run_grid(1, 1, EMU_SCAN_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gscan1_body(cx, p, EMU_T); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gcompact_body(cx, p); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gmsg_body(cx, p); });
    run_grid(1, 1, EMU_SCAN_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gscan2_body(cx, p, EMU_T); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_gplace_body(cx, p); });
    run_grid(EMU_GROUPS, 1, EMU_T, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_write_body(cx, p); });
    run_grid(1, 1, 64, NP_LDS_BYTES, [&](EmuCtx& cx) { nmp_carry_body(cx, p); });
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

}
