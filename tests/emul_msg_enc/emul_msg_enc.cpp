// emul_msg_enc.cpp -- CPU model of the batched message-field encoder (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the
// kernel body of gr-ais_amd/csrc/k_msg_enc.h runs one OS thread per lane under the same EmuCtx, driven by the launch
// plan that drives it on the device (MsgEncPlan, k_msg_enc.h) with host memory in place of device memory.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_msg_enc.h"

namespace {

constexpr int EMU_MENC_T = 128;    // (the device runs MENC_T threads: two waves keep the per-wave LDS regions apart)
constexpr int EMU_MENC_GROUPS = 2; // (the device takes up to MENC_MAX_GROUPS: a few waves make every wave loop)
const MsgEncTab EMU_ENC_TAB = msg_make_enc_tab();

struct EmuMsgEnc {
    explicit EmuMsgEnc(const MsgEncPlan& plan) : pl(plan) {}
    const MsgEncPlan pl;
    std::vector<HdlcRec> pdus; // (a record that is not written shows)
    std::vector<uint32_t> bytes;
    std::vector<int32_t> status;
    std::vector<int> count;
};

} // namespace

extern "C" {

// returns nullptr where aisx_msg_enc_batch_create returns AISX_ERR_INVALID
void* emu_msg_enc_create(int nchan, int max_rows, int table_rows)
{
    if (MsgEncPlan::check(nchan, max_rows, table_rows))
        return nullptr;
    EmuMsgEnc* h = new EmuMsgEnc(MsgEncPlan(nchan, max_rows, table_rows, EMU_MENC_T, EMU_MENC_GROUPS));
    emu_alloc(h->pdus, h->pl.pdus);
    emu_alloc(h->bytes, h->pl.bytes);
    emu_alloc(h->status, h->pl.status);
    emu_alloc(h->count, h->pl.count);
    return h;
}

void emu_msg_enc_destroy(void* hv) { delete (EmuMsgEnc*)hv; }

int emu_msg_enc_group_records() { return EMU_MENC_T; } // records one workgroup takes per pass

// 0 where aisx_msg_enc_batch_process returns AISX_ERR_INVALID for its strides and alignment
int emu_msg_enc_process(void* hv, const int32_t* cols, long long col_stride, const char* strs, const int32_t* idx, const int* nrows,
                        const int32_t* chan, int as_type, int as_part)
{
    EmuMsgEnc* h = (EmuMsgEnc*)hv;
    if (h->pl.check_call(col_stride, strs))
        return 0;
    const MsgEncBufs b = { (const uint32_t*)&EMU_ENC_TAB, h->pdus.data(), h->bytes.data(), h->status.data(), h->count.data() };
    h->pl.process(
        b, cols, col_stride, (const uint32_t*)strs, idx, nrows, chan, as_type, as_part,
        [&](int* first, int n) {
            memset(first, 0, sizeof(int) * (size_t)n);
            return true;
        },
        [&](const PlanLaunch& l, const MsgEncParams& p) {
            run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) { msg_enc_body(cx, p); });
            return true;
        });
    return 1;
}

// count[MENC_NCNT] (the bad-count flag cleared here); the whole list, written or not: pdus [max_rows], bytes
// [max_rows][56], status [max_rows]
void emu_msg_enc_read(void* hv, HdlcRec* pdus, unsigned char* bytes, int32_t* status, int* count)
{
    EmuMsgEnc* h = (EmuMsgEnc*)hv;
    for (int k = 0; k < MENC_NCNT; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    memcpy(pdus, h->pdus.data(), sizeof(HdlcRec) * h->pl.pdus.n);
    memcpy(bytes, h->bytes.data(), sizeof(uint32_t) * h->pl.bytes.n);
    memcpy(status, h->status.data(), sizeof(int32_t) * h->pl.status.n);
}

// the plan at the device's constants: out[0] = groups; 0 where it refuses
int emu_msg_enc_plan(int nchan, int max_rows, int table_rows, long long* out)
{
    if (MsgEncPlan::check(nchan, max_rows, table_rows))
        return 0;
    out[0] = MsgEncPlan(nchan, max_rows, table_rows).groups;
    return 1;
}

}
