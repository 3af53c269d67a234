// emul_mlse.cpp -- CPU model of the batched sequence detector (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// body of gr-ais_amd/csrc/k_mlse.h runs one OS thread per lane, driven by the launch plan that drives it on the device
// (MlsePlan, k_mlse.h) with host memory in place of device memory: the same two alternating state buffers.
#include "../emul/emul.cpp"
#include "../emul/emul_plan.h"
#include "../../gr-ais_amd/csrc/k_mlse.h"

namespace {

struct EmuMlse {
    explicit EmuMlse(const MlsePlan& plan) : pl(plan) {}
    MlsePlan pl;
    std::vector<MlseState> st[2];
    std::vector<cf> carry[2];
    std::vector<int> flag;
};

void run(EmuMlse* h, const cf* syms, long syms_stride, const int* nsyms, unsigned char* bits, long bits_stride, int* nbits)
{
    const MlseBufs b = { { h->st[0].data(), h->st[1].data() }, { h->carry[0].data(), h->carry[1].data() }, h->flag.data() };
    h->pl.process(b, syms, syms_stride, nsyms, bits, bits_stride, nbits, [&](const PlanLaunch& l, const MlseParams& p) {
        run_grid(l.gx, l.gy, l.threads, l.lds, [&](EmuCtx& cx) {
            if (l.kernel == MLSE_K_PROCESS)
                mlse_body<EmuCtx, false>(cx, p);
            else
                mlse_body<EmuCtx, true>(cx, p);
        });
        return true;
    });
}

} // namespace

extern "C" {

// rot16: {cos, sin} of the eight triples as aisx_mlse_model gives them (the bt they came from was taken by it); returns
// nullptr where aisx_mlse_batch_create returns AISX_ERR_INVALID
void* emu_mlse_create(const float* rot16, int nchan, int max_syms)
{
    if (MlsePlan::check(nchan, max_syms, true))
        return nullptr;
    MlseRot rot;
    for (int i = 0; i < 8; i++) {
        rot.c[i] = rot16[2 * i];
        rot.s[i] = rot16[2 * i + 1];
    }
    EmuMlse* h = new EmuMlse(MlsePlan(rot, nchan, max_syms));
    for (int k = 0; k < 2; k++) {
        emu_alloc(h->st[k], h->pl.st);
        emu_alloc(h->carry[k], h->pl.carry);
    }
    emu_alloc(h->flag, h->pl.flag);
    return h;
}

void emu_mlse_destroy(void* hv) { delete (EmuMlse*)hv; }

void emu_mlse_reset(void* hv)
{
    EmuMlse* h = (EmuMlse*)hv;
    for (int k = 0; k < 2; k++)
        emu_alloc(h->st[k], h->pl.st);
    h->flag[0] = 0;
    h->pl.reset();
}

void emu_mlse_process(void* hv, const cf* syms, long syms_stride, const int* nsyms, unsigned char* bits, long bits_stride, int* nbits)
{
    run((EmuMlse*)hv, syms, syms_stride, nsyms, bits, bits_stride, nbits);
}

void emu_mlse_flush(void* hv, unsigned char* bits, long bits_stride, int* nbits)
{
    run((EmuMlse*)hv, nullptr, 0, nullptr, bits, bits_stride, nbits);
}

// the bad-count word, cleared by the read
int emu_mlse_status(void* hv)
{
    EmuMlse* h = (EmuMlse*)hv;
    const int f = h->flag[0];
    h->flag[0] = 0;
    return f;
}

// the plan at the device's constants: out[1] = groups; 0 where it refuses
int emu_mlse_plan(int nchan, int max_syms, long long* out)
{
    if (MlsePlan::check(nchan, max_syms, true))
        return 0;
    out[0] = MlsePlan(MlseRot{}, nchan, max_syms).groups;
    return 1;
}

}
