// emul_msg.cpp -- CPU model of the batched message-field decoder (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the
// kernel body of gr-ais_amd/csrc/k_msg.h runs one OS thread per lane under the same EmuCtx, driven by the launch plan
// that drives it on the device (MsgPlan, k_msg.h) with host memory in place of device memory.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_msg.h"

namespace {

constexpr int EMU_MSG_T = 128;     // (the device runs MSG_T threads: two waves keep the per-wave LDS regions apart)
constexpr int EMU_MSG_GROUPS = 2;  // (the device takes up to MSG_MAX_GROUPS: a few waves make every wave loop)
const MsgTab EMU_TAB = msg_make_tab();

struct EmuMsg {
    explicit EmuMsg(const MsgPlan& plan) : pl(plan) {}
    const MsgPlan pl;
    std::vector<int32_t> cols; // (a row that is not written shows)
    std::vector<uint32_t> strs;
    std::vector<int> count;
};

} // namespace

extern "C" {

// returns nullptr where aisx_msg_batch_create returns AISX_ERR_INVALID
void* emu_msg_create(int nchan, int max_pdus, int length_max)
{
    if (MsgPlan::check(nchan, max_pdus, length_max))
        return nullptr;
    EmuMsg* h = new EmuMsg(MsgPlan(nchan, max_pdus, length_max, EMU_MSG_T, EMU_MSG_GROUPS));
    emu_alloc(h->cols, h->pl.cols);
    emu_alloc(h->strs, h->pl.strs);
    emu_alloc(h->count, h->pl.count);
    return h;
}

void emu_msg_destroy(void* hv) { delete (EmuMsg*)hv; }

int emu_msg_group_records() { return EMU_MSG_T; } // records one workgroup takes per pass

void emu_msg_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound)
{
    EmuMsg* h = (EmuMsg*)hv;
    const MsgBufs b = { &EMU_TAB.f[0][0], h->cols.data(), h->strs.data(), h->count.data() };
    h->pl.process(b, pdus, bytes, npdus, nfound, [&](const PlanLaunch& l, const MsgParams& p) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) { msg_body(cx, p); });
        return true;
    });
}

// count[0] found, [1] rows written, [2] bad-input flag (cleared here); the whole table, written or not:
// cols [MSG_NCOL][max_pdus], strs [max_pdus][MSG_STR]
void emu_msg_read(void* hv, int32_t* cols, char* strs, int* count)
{
    EmuMsg* h = (EmuMsg*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    memcpy(cols, h->cols.data(), sizeof(int32_t) * h->pl.cols.n);
    memcpy(strs, h->strs.data(), sizeof(uint32_t) * h->pl.strs.n);
}

// the plan at the device's constants: out[1] = groups; 0 where it refuses
int emu_msg_plan(int nchan, int max_pdus, int length_max, long long* out)
{
    if (MsgPlan::check(nchan, max_pdus, length_max))
        return 0;
    out[0] = MsgPlan(nchan, max_pdus, length_max).groups;
    return 1;
}

}
