// emul_xlate.cpp -- CPU model of the batched freq_xlating FIR (TEST INFRASTRUCTURE, see ../emul/emul.cpp): the kernel
// body of gr-ais_amd/csrc/k_xlate.h runs one OS thread per lane under the same EmuCtx, driven the way aisx_xlate.hip
// drives it on the device (host memory in place of device memory).  The host half (plan, phases, stream position) is
// the product's own XlateHost.
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_xlate.h"

namespace {

struct EmuXlate {
    XlateHost hs;
    int nt = 0;
    int hsel = 0;
    std::vector<cf> hist[2];
};

template <int R>
void run(EmuXlate* h, const XlateParams& p, int ntiles)
{
    run_grid(ntiles, h->hs.ns, h->nt, sizeof(cf) * XL_LDS_ITEMS,
             [&](EmuCtx& cx) { xlate_body<R>(cx, p, h->hs.taps.data()); });
}

} // namespace

extern "C" {

// nt: threads per workgroup (the device runs XL_T); returns nullptr where aisx_xlate_create returns AISX_ERR_INVALID
void* emu_xlate_create(int decim, const float* taps, int ntaps, const double* freqs, int nch, double fs, int ns,
                       int max_items, int nt)
{
    if (XlateHost::check(decim, taps, ntaps, freqs, nch, fs, ns, max_items) || nt < 1 || nt > XL_T)
        return nullptr;
    EmuXlate* h = new EmuXlate();
    h->nt = nt;
    h->hs.init(decim, taps, ntaps, freqs, nch, fs, ns, max_items, nt);
    for (auto& v : h->hist)
        v.assign((size_t)ns * h->hs.Lh + 1, mk(0.f, 0.f));
    return h;
}

void emu_xlate_destroy(void* hv) { delete (EmuXlate*)hv; }

// R, P, S, G, U, Utot
void emu_xlate_plan(void* hv, int* out)
{
    const XlatePlan& pl = ((EmuXlate*)hv)->hs.plan;
    const int v[6] = { pl.R, pl.P, pl.S, pl.G, pl.U, pl.Utot };
    memcpy(out, v, sizeof v);
}

int emu_xlate_output_count(void* hv, int n) { return ((EmuXlate*)hv)->hs.count(n); }

int emu_xlate_set_center_freq(void* hv, int stream, int chan, double f)
{
    EmuXlate* h = (EmuXlate*)hv;
    if (stream < 0 || stream >= h->hs.ns || chan < 0 || chan >= h->hs.nch || !xlate_freq_ok(f, h->hs.fs))
        return -1;
    h->hs.retune(stream * h->hs.nch + chan, f);
    return 0;
}

void emu_xlate_reset(void* hv)
{
    EmuXlate* h = (EmuXlate*)hv;
    h->hs.reset();
    for (auto& v : h->hist)
        std::fill(v.begin(), v.end(), mk(0.f, 0.f));
    h->hsel = 0;
}

// returns the outputs of this call (written to columns 0.. of every row of out)
int emu_xlate_process(void* hv, const cf* in, long in_stride, int n, cf* out, long out_stride)
{
    EmuXlate* h = (EmuXlate*)hv;
    XlateParams p = h->hs.params(n, in_stride, out_stride);
    p.in = in;
    p.hist_in = h->hist[h->hsel].data();
    p.hist_out = h->hist[h->hsel ^ 1].data();
    p.tab = h->hs.tab.data();
    p.par = h->hs.par.data();
    p.out = out;
    const int ntiles = h->hs.tiles(p.nout);
    switch (h->hs.plan.R) {
    case 8: run<8>(h, p, ntiles); break;
    case 4: run<4>(h, p, ntiles); break;
    case 2: run<2>(h, p, ntiles); break;
    default: run<1>(h, p, ntiles); break;
    }
    h->hsel ^= 1;
    return p.nout;
}
}
