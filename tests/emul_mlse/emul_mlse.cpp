// emul_mlse.cpp -- CPU model of the batched sequence detector (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// body of gr-ais_amd/csrc/k_mlse.h runs one OS thread per lane, driven the way aisx_mlse.hip drives it on the device
// (host memory in place of device memory, the same two alternating state buffers).
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_mlse.h"

namespace {

struct EmuMlse {
    int nchan, max_syms, groups, cur = 0, flag = 0;
    MlseRot rot;
    std::vector<MlseState> st[2];
    std::vector<cf> carry[2];
};

MlseParams params(EmuMlse* h, unsigned char* bits, long bits_stride, int* nbits)
{
    MlseParams p = {};
    p.max_syms = h->max_syms;
    p.bits = bits;
    p.bit_stride = bits_stride;
    p.nbits = nbits;
    p.st_in = h->st[h->cur].data();
    p.st_out = h->st[h->cur ^ 1].data();
    p.carry_in = h->carry[h->cur].data();
    p.carry_out = h->carry[h->cur ^ 1].data();
    p.flag = &h->flag;
    p.rot = h->rot;
    return p;
}

} // namespace

extern "C" {

// rot16: {cos, sin} of the eight triples as aisx_mlse_model gives them; the argument checks are the product's
void* emu_mlse_create(const float* rot16, int nchan, int max_syms)
{
    if (nchan < 1 || max_syms < 1 || max_syms > (1 << 27))
        return nullptr;
    EmuMlse* h = new EmuMlse();
    h->nchan = nchan;
    h->max_syms = max_syms;
    h->groups = std::max(1, ((max_syms + MLSE_B - 1) / MLSE_B + MLSE_T - 1) / MLSE_T);
    for (int i = 0; i < 8; i++) {
        h->rot.c[i] = rot16[2 * i];
        h->rot.s[i] = rot16[2 * i + 1];
    }
    for (int k = 0; k < 2; k++) {
        h->st[k].assign((size_t)nchan, MlseState{ 0, 0, 0 });
        h->carry[k].assign((size_t)nchan * MLSE_CARRY, mk(1.0e30f, -1.0e30f)); // (what is not written shows)
    }
    return h;
}

void emu_mlse_destroy(void* hv) { delete (EmuMlse*)hv; }

void emu_mlse_reset(void* hv)
{
    EmuMlse* h = (EmuMlse*)hv;
    for (int k = 0; k < 2; k++)
        h->st[k].assign((size_t)h->nchan, MlseState{ 0, 0, 0 });
    h->cur = h->flag = 0;
}

void emu_mlse_process(void* hv, const cf* syms, long syms_stride, const int* nsyms, unsigned char* bits, long bits_stride, int* nbits)
{
    EmuMlse* h = (EmuMlse*)hv;
    MlseParams p = params(h, bits, bits_stride, nbits);
    p.syms = syms;
    p.sym_stride = syms_stride;
    p.nsyms = nsyms;
    run_grid(h->nchan, h->groups, MLSE_T, MLSE_LDS_BYTES, [&](EmuCtx& cx) { mlse_body<EmuCtx, false>(cx, p); });
    h->cur ^= 1;
}

void emu_mlse_flush(void* hv, unsigned char* bits, long bits_stride, int* nbits)
{
    EmuMlse* h = (EmuMlse*)hv;
    const MlseParams p = params(h, bits, bits_stride, nbits);
    run_grid(h->nchan, 1, MLSE_T, MLSE_LDS_BYTES, [&](EmuCtx& cx) { mlse_body<EmuCtx, true>(cx, p); });
    h->cur ^= 1;
}

// the bad-count word, cleared by the read
int emu_mlse_status(void* hv)
{
    EmuMlse* h = (EmuMlse*)hv;
    const int f = h->flag;
    h->flag = 0;
    return f;
}

}
