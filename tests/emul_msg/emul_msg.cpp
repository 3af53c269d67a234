// emul_msg.cpp -- CPU model of the batched message-field decoder (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the
// kernel body of gr-ais_amd/csrc/k_msg.h runs one OS thread per lane under the same EmuCtx, driven the way
// aisx_msg.hip drives it on the device (host memory in place of device memory).
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_msg.h"

namespace {

constexpr int EMU_MSG_T = 128;     // (the device runs MSG_T threads: two waves keep the per-wave LDS regions apart)
constexpr int EMU_MSG_GROUPS = 2;  // (the device takes up to MSG_MAX_GROUPS: a few waves make every wave loop)
const MsgTab EMU_TAB = msg_make_tab();

struct EmuMsg {
    int nchan, max_pdus, lmax;
    std::vector<int32_t> cols;
    std::vector<uint32_t> strs;
    int count[4] = { 0, 0, 0, 0 };
};

} // namespace

extern "C" {

// the argument checks are the product's (aisx_msg_batch_create); returns nullptr where it returns AISX_ERR_INVALID
void* emu_msg_create(int nchan, int max_pdus, int length_max)
{
    if (nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > MSG_MAX_OCTETS)
        return nullptr;
    EmuMsg* h = new EmuMsg();
    h->nchan = nchan;
    h->max_pdus = max_pdus;
    h->lmax = length_max;
    h->cols.assign((size_t)MSG_NCOL * max_pdus, 0x5a5a5a5a); // (a row that is not written shows)
    h->strs.assign((size_t)MSG_STR_WORDS * max_pdus, 0x5a5a5a5au);
    return h;
}

void emu_msg_destroy(void* hv) { delete (EmuMsg*)hv; }

int emu_msg_group_records() { return EMU_MSG_T; } // records one workgroup takes per pass

void emu_msg_process(void* hv, const HdlcRec* pdus, const unsigned char* bytes, const int* npdus, const int* nfound)
{
    EmuMsg* h = (EmuMsg*)hv;
    MsgParams p;
    p.in = pdus;
    p.bytes = bytes;
    p.npdus = npdus;
    p.nfound = nfound;
    p.tab = &EMU_TAB.f[0][0];
    p.nchan = h->nchan;
    p.max_pdus = h->max_pdus;
    p.max_len = h->lmax - 1;
    p.nwaves = EMU_MSG_GROUPS * (EMU_MSG_T / 64);
    p.cols = h->cols.data();
    p.strs = h->strs.data();
    p.count = h->count;
    run_grid(EMU_MSG_GROUPS, 1, EMU_MSG_T, msg_lds_bytes(EMU_MSG_T), [&](EmuCtx& cx) { msg_body(cx, p); });
}

// count[0] found, [1] rows written, [2] bad-input flag (cleared here); the whole table, written or not:
// cols [MSG_NCOL][max_pdus], strs [max_pdus][MSG_STR]
void emu_msg_read(void* hv, int32_t* cols, char* strs, int* count)
{
    EmuMsg* h = (EmuMsg*)hv;
    for (int k = 0; k < 3; k++)
        count[k] = h->count[k];
    h->count[2] = 0;
    memcpy(cols, h->cols.data(), sizeof(int32_t) * h->cols.size());
    memcpy(strs, h->strs.data(), sizeof(uint32_t) * h->strs.size());
}

}
