// aisx_tx.hip -- C ABI of the batched burst transmitter (include/aisx.h, aisx_tx_batch_*): aisx_tx_batch_set_bursts
// checks and sorts a schedule on the host, uploads it and queues k_tx_frame (one wave per burst: payload -> packed
// levels); aisx_tx_batch_render queues k_tx_render (one workgroup per channel and tile of samples: the specification's
// formula per output sample, k_tx.h).  The host specification of both is aisx_tx.cpp.
#include <math.h>

#include <numeric>
#include <vector>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "aisx_tx.h"
#include "k_tx.h"

using namespace aisx;

static_assert(TXF_MAX_SYMS >= TX_MAX_RAMP + TX_MAX_TRAINING + TX_MAX_TAIL + 16 + 8 * (TX_MAX_OCTETS + 2) * 6 / 5, "k_tx_frame's LDS");
static_assert(TXR_LDS_BYTES <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(TXF_T) void k_tx_frame(TxFrameParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[TXF_MAX_SYMS];
    DevCtx cx{ smem };
    tx_frame_body(cx, p);
}

__global__ __launch_bounds__(TXR_T) void k_tx_render(TxRenderParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[TXR_LDS_BYTES];
    DevCtx cx{ smem };
    tx_render_body(cx, p);
}

struct aisx_tx_batch {
    int dev = 0;
    double sps = 0, bt = 0;
    int training = 0, ramp = 0, tail = 0, nchan = 0, max_bursts = 0, length_max = 0;
    int words = 0;   // 64-level words per burst
    int nbursts = 0, max_end = 0;
    int grid_cap = 0; // workgroups of a render call at most
    std::vector<int> order; // order[k] = where burst k of the caller's list went
    DevBuf<TxBurst> d_bursts;
    DevBuf<unsigned char> d_bytes;
    DevBuf<int> d_chan_off;
    DevBuf<unsigned long long> d_levels;
    DevBuf<int> d_wsum;
    DevBuf<int> d_nsyms;
    DevBuf<float> d_qtab;
    Event done; // behind the last render (set_bursts waits for it)
};

extern "C" int aisx_tx_batch_destroy(aisx_tx_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_tx_batch_create(aisx_tx_batch** out, double sps, double bt, int training_bits, int ramp_syms, int tail_syms,
                                    int nchan, int max_bursts, int length_max)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (tx_cfg_check(sps, bt, training_bits, ramp_syms, tail_syms) != AISX_OK)
        return AISX_ERR_INVALID;
    if (nchan < 1 || nchan > (1 << 20) || max_bursts < 1 || max_bursts > (1 << 24) || length_max < 1 || length_max > TX_MAX_OCTETS) {
        set_err("aisx_tx_batch_create: need 1 <= nchan <= 2^20, 1 <= max_bursts <= 2^24, 1 <= length_max <= %d", TX_MAX_OCTETS);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_tx_batch, aisx_tx_batch_destroy> h(new aisx_tx_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->sps = sps;
    h->bt = bt;
    h->training = training_bits;
    h->ramp = ramp_syms;
    h->tail = tail_syms;
    h->nchan = nchan;
    h->max_bursts = max_bursts;
    h->length_max = length_max;
    h->words = (tx_max_nsyms(training_bits, ramp_syms, tail_syms, length_max) + 63) / 64;
    hipDeviceProp_t prop;
    AISX_HIPCHK(hipGetDeviceProperties(&prop, h->dev));
    h->grid_cap = 4 * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256); // 4 x 33 KB of LDS fit a CU's 160
    const size_t nw = (size_t)max_bursts * h->words;
    if ((rc = h->d_bursts.alloc((size_t)max_bursts)) != AISX_OK || (rc = h->d_bytes.alloc((size_t)max_bursts * length_max)) != AISX_OK ||
        (rc = h->d_chan_off.alloc((size_t)nchan + 1)) != AISX_OK || (rc = h->d_levels.alloc(nw)) != AISX_OK ||
        (rc = h->d_wsum.alloc(nw)) != AISX_OK || (rc = h->d_nsyms.alloc((size_t)max_bursts)) != AISX_OK ||
        (rc = h->d_qtab.alloc(TX_QTAB, false)) != AISX_OK || (rc = h->done.create(hipEventDisableTiming)) != AISX_OK)
        return rc;
    // q at k / TX_QSTEPS from the closed form, rounded to float; the ends are exact
    std::vector<float> q(TX_QTAB);
    for (int k = 0; k < TX_QTAB; k++)
        q[(size_t)k] = (float)tx_qpulse((double)k / TX_QSTEPS, bt);
    AISX_HIPCHK(hipMemcpy(h->d_qtab, q.data(), sizeof(float) * TX_QTAB, hipMemcpyHostToDevice));
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_tx_batch_set_bursts(aisx_tx_batch* h, const aisx_burst* bursts, int n, const uint8_t* bytes, int64_t nbytes,
                                        void* stream)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (n > h->max_bursts) {
        set_err("aisx_tx_batch_set_bursts: %d bursts, the handle takes %d", n, h->max_bursts);
        return AISX_ERR_INVALID;
    }
    int rc = tx_bursts_check("aisx_tx_batch_set_bursts", bursts, n, h->nchan, h->length_max, bytes, nbytes);
    if (rc != AISX_OK)
        return rc;
    // sorted by (chan, start, frac), bursts that agree in all three in the caller's order
    std::vector<int> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [bursts](int a, int b) {
        const aisx_burst &x = bursts[a], &y = bursts[b];
        return x.chan != y.chan ? x.chan < y.chan : x.start != y.start ? x.start < y.start : x.frac < y.frac;
    });
    std::vector<TxBurst> recs((size_t)n);
    std::vector<unsigned char> packed;
    std::vector<int> chan_off((size_t)h->nchan + 1, 0), order((size_t)n);
    int max_end = 0;
    for (int k = 0; k < n; k++) {
        const aisx_burst& b = bursts[idx[(size_t)k]];
        TxBurst& r = recs[(size_t)k];
        order[(size_t)idx[(size_t)k]] = k;
        r.start = b.start;
        double x = ldexp((double)b.cfo, 64); // an integer (float cfo, |cfo| >= 2^-40) or rounded to one
        if (x >= 9223372036854775808.0)
            x -= 18446744073709551616.0;
        r.cfo_fix = (unsigned long long)llrint(x);
        r.offset = (long long)packed.size();
        packed.insert(packed.end(), bytes + b.offset, bytes + b.offset + b.len);
        r.frac = (double)b.frac;
        r.nsyms = tx_nsyms(h->training, h->ramp, h->tail, tx_stuffed_bits(bytes + b.offset, b.len));
        tx_extent(h->sps, r.frac, r.nsyms, &r.first, &r.end);
        r.len = b.len;
        r.amp = b.amp;
        const double turn = (double)b.phase / (2.0 * M_PI);
        r.turn = (float)(turn - rint(turn));
        r.chan = b.chan;
        r.pad = 0;
        chan_off[(size_t)b.chan + 1]++;
        max_end = r.end > max_end ? r.end : max_end;
    }
    for (int c = 0; c < h->nchan; c++)
        chan_off[(size_t)c + 1] += chan_off[(size_t)c];
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    AISX_HIPCHK(hipEventSynchronize(h->done)); // (the last render reads the schedule in place)
    if (n > 0) {
        AISX_HIPCHK(hipMemcpyAsync(h->d_bursts, recs.data(), sizeof(TxBurst) * (size_t)n, hipMemcpyHostToDevice, st));
        AISX_HIPCHK(hipMemcpyAsync(h->d_bytes, packed.data(), packed.size(), hipMemcpyHostToDevice, st));
    }
    AISX_HIPCHK(hipMemcpyAsync(h->d_chan_off, chan_off.data(), sizeof(int) * chan_off.size(), hipMemcpyHostToDevice, st));
    AISX_HIPCHK(hipStreamSynchronize(st)); // (the host vectors end with this call)
    h->nbursts = n;
    h->max_end = max_end;
    h->order = std::move(order);
    if (n > 0) {
        TxFrameParams p;
        p.bursts = h->d_bursts;
        p.bytes = h->d_bytes;
        p.nbursts = n;
        p.training = h->training;
        p.ramp = h->ramp;
        p.tail = h->tail;
        p.words = h->words;
        p.levels = h->d_levels;
        p.wsum = h->d_wsum;
        p.nsyms = h->d_nsyms;
        hipLaunchKernelGGL(k_tx_frame, dim3(n), dim3(TXF_T), 0, st, p);
        AISX_HIPCHK(hipGetLastError());
    }
    AISX_HIPCHK(hipEventRecord(h->done, st));
    return AISX_OK;
}

extern "C" int aisx_tx_batch_render(aisx_tx_batch* h, int64_t t0, int64_t n, aisx_cf32* d_out, int64_t out_stride, int accumulate,
                                    void* stream)
{
    if (!h || !d_out || n < 1 || n > (1LL << 30) || out_stride < n || ((size_t)d_out & 7u) || t0 <= -(1LL << 62) || t0 >= (1LL << 62)) {
        set_err("aisx_tx_batch_render: need 1 <= n <= 2^30 items at an 8-byte aligned address, out_stride >= n, |t0| < 2^62");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    TxRenderParams p;
    p.bursts = h->d_bursts;
    p.chan_off = h->d_chan_off;
    p.levels = h->d_levels;
    p.wsum = h->d_wsum;
    p.qtab = h->d_qtab;
    p.words = h->words;
    p.nchan = h->nchan;
    p.max_end = h->max_end;
    p.ramp = h->ramp;
    p.inv_sps = 1.0 / h->sps;
    p.t0 = t0;
    p.n = n;
    p.out = (cf*)d_out;
    p.stride = out_stride;
    p.accumulate = accumulate != 0;
    p.tiles_x = (int)((n + 1 + TX_TILE - 1) / TX_TILE); // (+ 1: a row that begins in the upper half of a 16-byte line)
    p.ntiles = (long long)p.tiles_x * h->nchan;
    const long long grid = p.ntiles < h->grid_cap ? p.ntiles : h->grid_cap;
    hipLaunchKernelGGL(k_tx_render, dim3((unsigned)grid), dim3(TXR_T), 0, st, p);
    AISX_HIPCHK(hipGetLastError());
    AISX_HIPCHK(hipEventRecord(h->done, st));
    return AISX_OK;
}

extern "C" int aisx_tx_batch_read_levels(aisx_tx_batch* h, int index, uint8_t* levels, int cap, int* nsyms, void* stream)
{
    if (!h || !nsyms || index < 0 || index >= h->nbursts || cap < 0 || (cap > 0 && !levels))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const int k = h->order[(size_t)index];
    std::vector<unsigned long long> w((size_t)h->words);
    int ns = 0;
    AISX_HIPCHK(hipMemcpyAsync(&ns, h->d_nsyms + k, sizeof(int), hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipMemcpyAsync(w.data(), h->d_levels + (size_t)k * h->words, sizeof(unsigned long long) * w.size(), hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *nsyms = ns;
    if (ns < 0 || ns > 64 * h->words || ns > cap) {
        set_err("aisx_tx_batch_read_levels: %d symbols, room for %d", ns, cap);
        return AISX_ERR_OVERFLOW;
    }
    for (int i = 0; i < ns; i++)
        levels[i] = (uint8_t)((w[(size_t)(i >> 6)] >> (i & 63)) & 1ull);
    return AISX_OK;
}
