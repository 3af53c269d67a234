// emul_xlate_fmt.cpp -- CPU model of the batched freq_xlating FIR fed the source's own sample format (TEST
// INFRASTRUCTURE, see ../emul/emul.cpp and ../emul_xlate/emul_xlate.cpp): xlate_body of gr-ais_amd/csrc/k_xlate.h with
// each of its four loaders, one OS thread per lane, driven the way aisx_xlate_process_fmt drives it on the device.
#include "../emul/emul.cpp"
#include "../../gr-ais_amd/csrc/k_xlate.h"

namespace {

struct EmuXlateFmt {
    XlateHost hs;
    int nt = 0;
    int hsel = 0;
    std::vector<cf> hist[2];
};

template <int R, class Ld>
void run(EmuXlateFmt* h, const XlateParams& p, int ntiles)
{
    run_grid(ntiles, h->hs.ns, h->nt, sizeof(cf) * XL_LDS_ITEMS,
             [&](EmuCtx& cx) { xlate_body<R, EmuCtx, Ld>(cx, p, h->hs.taps.data()); });
}

template <class Ld>
void run_r(EmuXlateFmt* h, const XlateParams& p, int ntiles)
{
    switch (h->hs.plan.R) {
    case 8: run<8, Ld>(h, p, ntiles); break;
    case 4: run<4, Ld>(h, p, ntiles); break;
    case 2: run<2, Ld>(h, p, ntiles); break;
    default: run<1, Ld>(h, p, ntiles); break;
    }
}

} // namespace

extern "C" {

void* emu_xlate_fmt_create(int decim, const float* taps, int ntaps, const double* freqs, int nch, double fs, int ns,
                           int max_items, int nt)
{
    if (XlateHost::check(decim, taps, ntaps, freqs, nch, fs, ns, max_items) || nt < 1 || nt > XL_T)
        return nullptr;
    EmuXlateFmt* h = new EmuXlateFmt();
    h->nt = nt;
    h->hs.init(decim, taps, ntaps, freqs, nch, fs, ns, max_items, nt);
    for (auto& v : h->hist)
        v.assign((size_t)ns * h->hs.Lh + 1, mk(0.f, 0.f));
    return h;
}

void emu_xlate_fmt_destroy(void* hv) { delete (EmuXlateFmt*)hv; }

int emu_xlate_fmt_output_count(void* hv, int n) { return ((EmuXlateFmt*)hv)->hs.count(n); }

int emu_xlate_fmt_item_bytes(int fmt) { return xlate_fmt_ok(fmt, 1.f, 0.f) ? xlate_item_bytes(fmt) : -1; }

// in: items of `fmt` (in_stride in items); returns the outputs of this call, or -1 where aisx_xlate_process_fmt
// returns AISX_ERR_INVALID for the format arguments
int emu_xlate_fmt_process(void* hv, const void* in, int fmt, float scale, float bias, long in_stride, int n, cf* out,
                          long out_stride)
{
    EmuXlateFmt* h = (EmuXlateFmt*)hv;
    if (!xlate_fmt_ok(fmt, scale, bias))
        return -1;
    XlateParams p = h->hs.params(n, in_stride, out_stride);
    p.in = in;
    p.scale = scale;
    p.bias = bias;
    p.hist_in = h->hist[h->hsel].data();
    p.hist_out = h->hist[h->hsel ^ 1].data();
    p.tab = h->hs.tab.data();
    p.par = h->hs.par.data();
    p.out = out;
    const int ntiles = h->hs.tiles(p.nout);
    switch (fmt) {
    case XL_FMT_CS16: run_r<XlLoadCS16>(h, p, ntiles); break;
    case XL_FMT_CS8: run_r<XlLoadCS8>(h, p, ntiles); break;
    case XL_FMT_CU8: run_r<XlLoadCU8>(h, p, ntiles); break;
    default: run_r<XlLoadCF32>(h, p, ntiles); break;
    }
    h->hsel ^= 1;
    return p.nout;
}
}
