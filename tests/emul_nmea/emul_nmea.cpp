// emul_nmea.cpp -- CPU model of the batched NMEA armouring (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// bodies of gr-ais_amd/csrc/k_nmea.h run one OS thread per lane under the same EmuCtx, driven by the launch plan that
// drives them on the device (NmeaPlan, k_nmea.h) with host memory in place of device memory.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_nmea.h"

namespace {

constexpr int EMU_SCAN_T = 128;  // (the device runs NM_SCAN_T threads: two waves keep the cross-wave scan in play)
constexpr int EMU_W_T = 128;
constexpr int EMU_W_GROUPS = 3;  // (the device takes up to NM_W_MAX_GROUPS: a few waves make every wave loop)

struct EmuNmea {
    explicit EmuNmea(NmeaPlan&& plan) : pl(std::move(plan)) {}
    const NmeaPlan pl;
    std::vector<char> text;
    std::vector<HdlcRec> out;
    std::vector<int> count;
};

} // namespace

extern "C" {

// returns nullptr where aisx_nmea_batch_create returns AISX_ERR_INVALID
void* emu_nmea_create(const char* const* designators, int nchan, int max_pdus, int length_max, long text_cap)
{
    if (NmeaPlan::check(designators, nchan, max_pdus, length_max, text_cap) || nm_bad_designator(designators, nchan) >= 0)
        return nullptr;
    EmuNmea* h = new EmuNmea(NmeaPlan(designators, nchan, max_pdus, length_max, text_cap, EMU_SCAN_T, EMU_W_T, EMU_W_GROUPS));
    emu_alloc(h->out, h->pl.out);
    emu_alloc(h->text, h->pl.text);
    emu_alloc(h->count, h->pl.count);
    return h;
}

void emu_nmea_destroy(void* hv) { delete (EmuNmea*)hv; }

long emu_nmea_text_cap(void* hv) { return (long)((EmuNmea*)hv)->pl.text_cap; }

int emu_nmea_text_len(int len, int dlen) { return nm_text_len(len, dlen); }

void emu_nmea_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound)
{
    EmuNmea* h = (EmuNmea*)hv;
    const NmeaBufs b = { h->pl.desig_host.data(), h->pl.dlen_host.data(), h->out.data(), h->text.data(), h->count.data() };
    h->pl.process(b, pdus, bytes, npdus, nfound, [&](const PlanLaunch& l, const NmeaCall& c) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) {
            if (l.kernel == NM_K_SCAN)
                nmea_scan_body(cx, c.s);
            else
                nmea_write_body(cx, c.w);
        });
        return true;
    });
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

// the plan at the device's constants: out[2] = text_cap, write_groups; 0 where it refuses
int emu_nmea_plan(const char* const* designators, int nchan, int max_pdus, int length_max, long text_cap, long long* out)
{
    if (NmeaPlan::check(designators, nchan, max_pdus, length_max, text_cap) || nm_bad_designator(designators, nchan) >= 0)
        return 0;
    const NmeaPlan pl(designators, nchan, max_pdus, length_max, text_cap);
    out[0] = pl.text_cap;
    out[1] = pl.write_groups;
    return 1;
}

}
