// emul_nmea_std.cpp -- CPU model of the batched NMEA armouring in the standard form (TEST INFRASTRUCTURE, see
// ../emul/emul.cpp): the kernel bodies of gr-ais_amd/csrc/k_nmea_std.h run one OS thread per lane under the same EmuCtx,
// driven by the launch plan that drives them on the device (NmeaStdPlan) with host memory in place of device memory.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_nmea_std.h"

namespace {

constexpr int EMU_SCAN_T = 128;  // (the device runs NM_SCAN_T threads: two waves keep the cross-wave scan in play, and a
                                 // scan tile is 128 x NM_ITEMS = 1024 records)
constexpr int EMU_W_T = 128;
constexpr int EMU_W_GROUPS = 3;  // (the device takes up to NM_W_MAX_GROUPS: a few waves make every wave loop)

struct EmuNmeaStd {
    explicit EmuNmeaStd(NmeaStdPlan&& plan) : pl(std::move(plan)) {}
    const NmeaStdPlan pl;
    std::vector<char> text;
    std::vector<HdlcRec> out;
    std::vector<int> count;
    std::vector<unsigned char> ids;
    long long time = -1;
};

bool args_ok(const char* const* designators, const char* const* stations, int nchan, int max_pdus, int length_max, long text_cap)
{
    return !NmeaStdPlan::check(designators, nchan, max_pdus, length_max, text_cap) && nm_bad_designator(designators, nchan) < 0 &&
           nms_bad_station(stations, nchan) < 0;
}

} // namespace

extern "C" {

// returns nullptr where aisx_nmea_batch_create_std returns AISX_ERR_INVALID
void* emu_nmea_std_create(const char* const* designators, const char* const* stations, int nchan, int max_pdus, int length_max,
                          long text_cap)
{
    if (!args_ok(designators, stations, nchan, max_pdus, length_max, text_cap))
        return nullptr;
    EmuNmeaStd* h = new EmuNmeaStd(NmeaStdPlan(designators, stations, nchan, max_pdus, length_max, text_cap, EMU_SCAN_T, EMU_W_T, EMU_W_GROUPS));
    emu_alloc(h->out, h->pl.out);
    emu_alloc(h->text, h->pl.text);
    emu_alloc(h->count, h->pl.count);
    emu_alloc(h->ids, h->pl.ids);
    return h;
}

void emu_nmea_std_destroy(void* hv) { delete (EmuNmeaStd*)hv; }

long emu_nmea_std_text_cap(void* hv) { return (long)((EmuNmeaStd*)hv)->pl.text_cap; }

int emu_nmea_std_scan_tile() { return EMU_SCAN_T * NM_ITEMS; }

// 0 where aisx_nmea_batch_set_time returns AISX_ERR_INVALID
int emu_nmea_std_set_time(void* hv, long long time)
{
    if (!nms_time_ok(time))
        return 0;
    ((EmuNmeaStd*)hv)->time = time;
    return 1;
}

void emu_nmea_std_reset(void* hv)
{
    EmuNmeaStd* h = (EmuNmeaStd*)hv;
    h->count[3] = 0;
    h->time = -1;
}

int emu_nmea_std_next_id(void* hv) { return ((EmuNmeaStd*)hv)->count[3]; }

void emu_nmea_std_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound)
{
    EmuNmeaStd* h = (EmuNmeaStd*)hv;
    const NmeaStdBufs b = { { h->pl.desig_host.data(), h->pl.dlen_host.data(), h->out.data(), h->text.data(), h->count.data() },
                            h->pl.station_host.data(), h->pl.slen_host.data(), h->ids.data() };
    h->pl.process(b, pdus, bytes, npdus, nfound, h->time, [&](const PlanLaunch& l, const NmeaStdCall& c) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) {
            if (l.kernel == NM_K_STD_SCAN)
                nmea_std_scan_body(cx, c.s);
            else
                nmea_std_write_body(cx, c.w);
        });
        return true;
    });
}

// count[0] found, [1] records written, [2] bad-input flag (cleared here); the records written and the text up to
// the last one's end
void emu_nmea_std_read(void* hv, HdlcRec* recs, char* text, int* count)
{
    EmuNmeaStd* h = (EmuNmeaStd*)hv;
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
int emu_nmea_std_plan(const char* const* designators, const char* const* stations, int nchan, int max_pdus, int length_max,
                      long text_cap, long long* out)
{
    if (!args_ok(designators, stations, nchan, max_pdus, length_max, text_cap))
        return 0;
    const NmeaStdPlan pl(designators, stations, nchan, max_pdus, length_max, text_cap);
    out[0] = pl.text_cap;
    out[1] = pl.write_groups;
    return 1;
}

}
