// aisx_xlate.hip -- C ABI of the batched freq_xlating_fir_filter_ccf (include/aisx.h, aisx_xlate_*): one launch per
// call (k_xlate.h: xlate_body) on the caller's stream.  The handle keeps the phase of every row on the host (64-bit
// increment and offset, k_xlate.h) and uploads it, with the rows' in-block rotation tables, ahead of the first call
// after a change.
#include <string.h>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_xlate.h"

using namespace aisx;

template <int R>
__global__ __launch_bounds__(XL_T) void k_xlate(XlateParams p, const float* __restrict__ taps)
{
    __shared__ __attribute__((aligned(16))) cf smem[XL_LDS_ITEMS];
    DevCtx cx{ (char*)smem };
    xlate_body<R>(cx, p, taps);
}

// the same body reading the source's own sample format (AISX_FMT_CS16 / CS8 / CU8), converted where it is staged
template <int R, class Ld>
__global__ __launch_bounds__(XL_T) void k_xlate_fmt(XlateParams p, const float* __restrict__ taps)
{
    __shared__ __attribute__((aligned(16))) cf smem[XL_LDS_ITEMS];
    DevCtx cx{ (char*)smem };
    xlate_body<R, DevCtx, Ld>(cx, p, taps);
}

struct aisx_xlate {
    int dev = 0;
    XlateHost hs;                          // geometry, plan, phases, stream position (k_xlate.h)
    int hsel = 0;                          // which history buffer holds the current history
    bool dirty = true;                     // phases / tables differ from the device's copy
    DevBuf<cf> d_hist[2];                  // [ns][Lh] each
    DevBuf<float> d_taps;                  // [Utot][R]
    DevBuf<cf> d_tab;                      // [nrows][XL_B]
    DevBuf<unsigned long long> d_par;      // [nrows][2]
    PinnedBuf<cf> h_tab;                   // pinned staging of the uploads
    PinnedBuf<unsigned long long> h_par;
    Event ev_up, ev_done;
};

extern "C" int aisx_xlate_destroy(aisx_xlate* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    if (h->ev_done)
        (void)hipEventSynchronize(h->ev_done);
    if (h->ev_up)
        (void)hipEventSynchronize(h->ev_up);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_xlate_create(aisx_xlate** out, int decim, const float* taps, int ntaps, const double* center_freqs,
                                 int nchan_per_stream, double samp_rate, int nstreams, int max_items)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = XlateHost::check(decim, taps, ntaps, center_freqs, nchan_per_stream, samp_rate, nstreams, max_items)) {
        set_err("aisx_xlate_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_xlate, aisx_xlate_destroy> h(new aisx_xlate());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    XlateHost& hs = h->hs;
    hs.init(decim, taps, ntaps, center_freqs, nchan_per_stream, samp_rate, nstreams, max_items, XL_T);
    const size_t hist = (size_t)nstreams * hs.Lh, nrows = (size_t)hs.nrows();
    if ((rc = h->d_hist[0].alloc(hist)) != AISX_OK || (rc = h->d_hist[1].alloc(hist)) != AISX_OK ||
        (rc = h->d_taps.alloc(hs.taps.size(), false)) != AISX_OK || (rc = h->d_tab.alloc(nrows * XL_B, false)) != AISX_OK ||
        (rc = h->d_par.alloc(nrows * 2, false)) != AISX_OK || (rc = h->h_tab.alloc(nrows * XL_B)) != AISX_OK ||
        (rc = h->h_par.alloc(nrows * 2)) != AISX_OK || (rc = h->ev_up.create(hipEventDisableTiming)) != AISX_OK ||
        (rc = h->ev_done.create(hipEventDisableTiming)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipMemcpy(h->d_taps, hs.taps.data(), sizeof(float) * hs.taps.size(), hipMemcpyHostToDevice));
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_xlate_geometry(const aisx_xlate* h, int* nstreams, int* nchan_per_stream, int* decim, int* ntaps,
                                   int* max_items)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (nstreams)
        *nstreams = h->hs.ns;
    if (nchan_per_stream)
        *nchan_per_stream = h->hs.nch;
    if (decim)
        *decim = h->hs.D;
    if (ntaps)
        *ntaps = h->hs.L;
    if (max_items)
        *max_items = h->hs.max_items;
    return AISX_OK;
}

extern "C" int aisx_xlate_output_count(const aisx_xlate* h, int n)
{
    if (!h || n < 0) {
        set_err("aisx_xlate_output_count: need a handle and n >= 0");
        return AISX_ERR_INVALID;
    }
    return h->hs.count(n);
}

extern "C" int aisx_xlate_center_freq(const aisx_xlate* h, int stream, int chan, double* center_freq)
{
    if (!h || !center_freq || stream < 0 || stream >= h->hs.ns || chan < 0 || chan >= h->hs.nch) {
        set_err("aisx_xlate_center_freq: need a handle, an output and a stream and channel in range");
        return AISX_ERR_INVALID;
    }
    *center_freq = h->hs.freq[(size_t)stream * h->hs.nch + chan];
    return AISX_OK;
}

extern "C" int aisx_xlate_set_center_freq(aisx_xlate* h, int stream, int chan, double center_freq)
{
    if (!h || stream < 0 || stream >= h->hs.ns || chan < 0 || chan >= h->hs.nch || !xlate_freq_ok(center_freq, h->hs.fs)) {
        set_err("aisx_xlate_set_center_freq: need a handle, a stream and channel in range and |f| <= fs/2");
        return AISX_ERR_INVALID;
    }
    h->hs.retune(stream * h->hs.nch + chan, center_freq);
    h->dirty = true;
    return AISX_OK;
}

extern "C" int aisx_xlate_reset(aisx_xlate* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipEventSynchronize(h->ev_done));
    const size_t hist = sizeof(cf) * (size_t)h->hs.ns * h->hs.Lh;
    if (hist) {
        AISX_HIPCHK(hipMemset(h->d_hist[0], 0, hist));
        AISX_HIPCHK(hipMemset(h->d_hist[1], 0, hist));
    }
    h->hs.reset();
    h->hsel = 0;
    h->dirty = true;
    return AISX_OK;
}

template <int R>
static void launch(const aisx_xlate* h, const XlateParams& p, int fmt, int ntiles, hipStream_t st)
{
    const dim3 grid(ntiles, h->hs.ns), block(XL_T);
    const float* taps = h->d_taps;
    switch (fmt) {
    case XL_FMT_CS16: hipLaunchKernelGGL((k_xlate_fmt<R, XlLoadCS16>), grid, block, 0, st, p, taps); break;
    case XL_FMT_CS8: hipLaunchKernelGGL((k_xlate_fmt<R, XlLoadCS8>), grid, block, 0, st, p, taps); break;
    case XL_FMT_CU8: hipLaunchKernelGGL((k_xlate_fmt<R, XlLoadCU8>), grid, block, 0, st, p, taps); break;
    default: hipLaunchKernelGGL(k_xlate<R>, grid, block, 0, st, p, taps); break;
    }
}

static int xlate_process(const char* who, aisx_xlate* h, const void* d_in, int fmt, float scale, float bias, long in_stride,
                         int n, aisx_cf32* d_out, long out_stride, int* nout, void* stream)
{
    if (!h || !d_in || !d_out || !nout || n < 1 || n > h->hs.max_items || (h->hs.ns > 1 && in_stride < n)) {
        set_err("%s: need a handle, input, output and count; 1 <= n <= max_items (%d), "
                "in_stride >= n", who, h ? h->hs.max_items : 0);
        return AISX_ERR_INVALID;
    }
    if (!xlate_fmt_ok(fmt, scale, bias)) {
        set_err("%s: need a format 0 .. 3 (cf32, cs16, cs8, cu8) and a finite scale and bias", who);
        return AISX_ERR_INVALID;
    }
    const int cnt = h->hs.count(n);
    if (h->hs.nrows() > 1 && out_stride < cnt) {
        set_err("%s: out_stride %ld is below the %d outputs of this call", who, out_stride, cnt);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    XlateHost& hs = h->hs;
    if (h->dirty) {
        // (the previous upload has left the pinned buffers long ago, but it must have)
        AISX_HIPCHK(hipEventSynchronize(h->ev_up));
        memcpy(h->h_par, hs.par.data(), sizeof(unsigned long long) * hs.par.size());
        memcpy(h->h_tab, hs.tab.data(), sizeof(cf) * hs.tab.size());
        AISX_HIPCHK(hipMemcpyAsync(h->d_par, h->h_par, sizeof(unsigned long long) * hs.par.size(), hipMemcpyHostToDevice, st));
        AISX_HIPCHK(hipMemcpyAsync(h->d_tab, h->h_tab, sizeof(cf) * hs.tab.size(), hipMemcpyHostToDevice, st));
        AISX_HIPCHK(hipEventRecord(h->ev_up, st));
        h->dirty = false;
    }
    XlateParams p = hs.params(n, in_stride, out_stride);
    p.in = d_in;
    p.scale = scale;
    p.bias = bias;
    p.hist_in = h->d_hist[h->hsel];
    p.hist_out = h->d_hist[h->hsel ^ 1];
    p.tab = h->d_tab;
    p.par = h->d_par;
    p.out = (cf*)d_out;
    const int ntiles = hs.tiles(cnt);
    switch (hs.plan.R) {
    case 8: launch<8>(h, p, fmt, ntiles, st); break;
    case 4: launch<4>(h, p, fmt, ntiles, st); break;
    case 2: launch<2>(h, p, fmt, ntiles, st); break;
    default: launch<1>(h, p, fmt, ntiles, st); break;
    }
    AISX_HIPCHK(hipGetLastError());
    AISX_HIPCHK(hipEventRecord(h->ev_done, st));
    h->hsel ^= 1;
    *nout = cnt;
    return AISX_OK;
}

extern "C" int aisx_xlate_process(aisx_xlate* h, const aisx_cf32* d_in, long in_stride, int n, aisx_cf32* d_out,
                                  long out_stride, int* nout, void* stream)
{
    return xlate_process("aisx_xlate_process", h, d_in, XL_FMT_CF32, 1.f, 0.f, in_stride, n, d_out, out_stride, nout, stream);
}

extern "C" int aisx_xlate_process_fmt(aisx_xlate* h, const void* d_in, int fmt, float scale, float bias, long in_stride,
                                      int n, aisx_cf32* d_out, long out_stride, int* nout, void* stream)
{
    return xlate_process("aisx_xlate_process_fmt", h, d_in, fmt, scale, bias, in_stride, n, d_out, out_stride, nout, stream);
}
