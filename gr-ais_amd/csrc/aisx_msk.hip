// aisx_msk.hip -- C ABI (include/aisx.h) for msk_timing_recovery_cc and the NRZI bit tail,
// plus the __global__ wrappers that run the kernel bodies of k_msk.h on gfx950.  The time-parallel recovery
// (off unless asked for) is aisx_mskp.hip: this file compiles without k_mskp.h.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "aisx_devctx.h"
#include "aisx_msk_impl.h"
#include "aisx_plan.h"
#include "aisx_tables.h"

using namespace aisx;

template <bool AUX, bool OSPS2, int LPW>
__global__ __launch_bounds__(64 * msk_waves(LPW)) void k_msk(MskParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DevCtx cx{ smem };
    // the recurrence is latency-bound and issues little: its waves go first on their SIMDs, ahead
    // of the throughput kernels of the other stream that share them
#ifndef MSK_PRIO
#define MSK_PRIO 3
#endif
    __builtin_amdgcn_s_setprio(MSK_PRIO);
    msk_body<DevCtx, AUX, OSPS2, LPW>(cx, p);
}

// the same kernel as the join of the time-parallel recovery (MskParams::ff)
template <int LPW>
__global__ __launch_bounds__(64 * msk_waves(LPW)) void k_msk_ff(MskParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DevCtx cx{ smem };
    __builtin_amdgcn_s_setprio(MSK_PRIO);
    msk_body<DevCtx, false, false, LPW, true>(cx, p);
}

// the build the chain launches (no err / mu ports, osps 1, 8 channels per wave) with the hand-scheduled pair (MskParams::pair_core)
__global__ __launch_bounds__(64 * msk_waves(8)) void k_msk_core(MskParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DevCtx cx{ smem };
    __builtin_amdgcn_s_setprio(MSK_PRIO);
    msk_body<DevCtx, false, false, 8, false, true>(cx, p);
}

__global__ __launch_bounds__(BT_T) void k_bittail(BitTailParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[260 * 4];
    DevCtx cx{ smem };
    bittail_body(cx, p);
}

// One wave that does nothing for `ticks` periods of the 100 MHz wall clock: queued on a stream
// behind the event of aisx_msk_wait_prepass it gives the recovery kernel, which becomes ready
// at that same event on its own stream, a head start at the dispatcher (see aisx_msk_wait_prepass).
__global__ __launch_bounds__(64) void k_msk_headstart(unsigned ticks)
{
    const unsigned long long t0 = wall_clock64();
    // (bounded whatever the clock does: 2048 sleeps of 32 x 64 cycles are ~2 ms)
    for (int k = 0; k < 2048 && wall_clock64() - t0 < ticks; k++)
        __builtin_amdgcn_s_sleep(32);
}

__global__ __launch_bounds__(256) void k_msk_tagprep(TagPrepParams p)
{
    DevCtx cx{ nullptr };
    tagprep_body(cx, p);
}

// launch the timing-recovery build for (err/mu ports connected, osps == 2, channels per wave)
int aisx::msk_launch(const MskParams& p, int nwg, hipStream_t st)
{
    typedef void (*kfn)(MskParams);
    static const kfn fns[20] = {
        k_msk<false, false, 16>, k_msk<false, true, 16>, k_msk<true, false, 16>, k_msk<true, true, 16>,
        k_msk<false, false, 32>, k_msk<false, true, 32>, k_msk<true, false, 32>, k_msk<true, true, 32>,
        k_msk<false, false, 64>, k_msk<false, true, 64>, k_msk<true, false, 64>, k_msk<true, true, 64>,
        k_msk<false, false, 8>,  k_msk<false, true, 8>,  k_msk<true, false, 8>,  k_msk<true, true, 8>,
        k_msk<false, false, 4>,  k_msk<false, true, 4>,  k_msk<true, false, 4>,  k_msk<true, true, 4>,
    };
    const int li = p.lpw == 16 ? 0 : (p.lpw == 32 ? 1 : (p.lpw == 64 ? 2 : (p.lpw == 8 ? 3 : 4)));
    const int v = li * 4 + (((p.err || p.mu_out) ? 2 : 0) | (p.osps == 2 ? 1 : 0));
    // LDS beyond what the kernel uses keeps other streams' workgroups off this CU: a knob for how
    // much of its SIMDs' issue the recurrence shares (AISX_MSK_LDS_PAD, KiB; experiments)
    static const int pad = [] {
        const char* e = exp_env("AISX_MSK_LDS_PAD");
        return e ? atoi(e) * 1024 : 0;
    }();
    const int lds = std::min(msk_lds_bytes(p.lpw) + pad, 160 * 1024);
    kfn fn = fns[v];
    if (p.ff) { // the join of the time-parallel recovery: a build of its own (stream mode, osps 1, no err / mu)
        static const kfn ffs[5] = { k_msk_ff<16>, k_msk_ff<32>, k_msk_ff<64>, k_msk_ff<8>, k_msk_ff<4> };
        if (p.err || p.mu_out || p.osps == 2) {
            set_err("msk_launch: the join build has no err / mu ports and osps == 1");
            return AISX_ERR_INVALID;
        }
        fn = ffs[li];
    } else if (p.pair_core && v == 3 * 4) { // (the other builds keep the compiler's schedule)
        fn = k_msk_core;
    }
    int rc = ensure_dyn_lds((const void*)fn, lds, "msk_timing_recovery_cc");
    if (rc != AISX_OK)
        return rc;
    // a workgroup = msk_waves(lpw) waves with lpw channels each
    hipLaunchKernelGGL(fn, dim3(nwg), dim3(64 * msk_waves(p.lpw)), lds, st, p);
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

// ---------------------------------------------------------------------------
// msk_timing_recovery_cc
// ---------------------------------------------------------------------------
// What the kernel's LDS rings and the carry buffer are sized for (k_msk.h): one general_work call
// of a single output must fit the carry (forecast(1) + the pre-item), a pair of iterations must
// stay well inside a 64-sample chunk, and omega must stay positive under the clip of :182
// (omega in [d_sps - |limit|, d_sps + |limit|], `limit` is absolute).
static int msk_check_geometry(float d_sps, float gain, float limit)
{
    const float wmin = d_sps - fabsf(limit), wmax = d_sps + fabsf(limit);
    if (!(wmin >= 0.5f) || msk_forecast(d_sps, 1) + 1 > aisx_msk::carry_cap || !(2.f * wmax + 3.f * fabsf(gain) <= 32.f)) {
        set_err("msk_timing_recovery: sps/2 = %g with limit %g and gain %g is outside what the gfx950 kernel is sized for "
                "(sps/2 - |limit| >= 0.5, forecast(1) < %d items, 2 (sps/2 + |limit|) + 3 |gain| <= 32)",
                d_sps, limit, gain, aisx_msk::carry_cap);
        return AISX_ERR_INVALID;
    }
    return AISX_OK;
}
// items per channel one call can produce: without tags every output consumes at least
// 2 (d_sps - |limit|) input items (osps = 1; half of that for osps = 2).  A time_est tag sets
// d_div = 0 (:159): the iteration it resets emits a symbol whatever came before, and it may step
// iidx back by one (:151-154) -- up to two more outputs per tag.  Room for max_items / 64 tags
// per call is added (the stock chain produces one per ~600 samples; a burst gives 3-4 on
// consecutive pairs); a call that needs more ends with AISX_MSK_ST_OUT_FULL.
static int msk_out_cap(const aisx_msk* h)
{
    const double wmin = (double)h->d_sps - fabs((double)h->limit);
    const int tag_room = 2 * std::max(16, h->max_items / 64);
    return ((int)ceil((h->max_items + aisx_msk::carry_cap) / (2.0 * wmin)) + tag_room) * h->osps + 16;
}

static int msk_init_state(aisx_msk* h)
{
    const int nc = h->nchan;
    std::vector<float> mu(nc, 0.5f), om(nc, h->d_sps); // impl :49-56, :71
    AISX_HIPCHK(hipMemcpy(h->d_mu, mu.data(), sizeof(float) * nc, hipMemcpyHostToDevice));
    AISX_HIPCHK(hipMemcpy(h->d_omega, om.data(), sizeof(float) * nc, hipMemcpyHostToDevice));
    AISX_HIPCHK(hipMemset(h->d_div, 0, sizeof(int) * nc));
    AISX_HIPCHK(hipMemset(h->d_dly1, 0, sizeof(cf) * nc));
    AISX_HIPCHK(hipMemset(h->d_dly2, 0, sizeof(cf) * nc));
    AISX_HIPCHK(hipMemset(h->d_diff1, 0, sizeof(cf) * nc));
    for (int k = 0; k < 2; k++) {
        AISX_HIPCHK(hipMemset(h->d_tprev[k], 0, sizeof(cf) * nc));
        AISX_HIPCHK(hipMemset(h->d_tbit[k], 0, nc));
    }
    h->tcur = 0;
    AISX_HIPCHK(hipMemset(h->d_nread, 0, sizeof(unsigned long long) * nc));
    for (int k = 0; k < 2; k++) {
        AISX_HIPCHK(hipMemset(h->d_carry[k], 0, sizeof(cf) * (size_t)nc * aisx_msk::carry_cap));
        AISX_HIPCHK(hipMemset(h->d_carry_len[k], 0, sizeof(int) * nc));
        AISX_HIPCHK(hipMemset(h->d_ctag_n[k], 0, sizeof(int) * nc));
    }
    h->cur = 0;
    h->total_in = 0;
    return AISX_OK;
}

extern "C" int aisx_msk_create(aisx_msk** out, float sps, float gain, float limit, int osps, int nchan, int max_items)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (nchan < 1 || max_items < 1 || !(sps > 0)) {
        set_err("aisx_msk_create: bad argument");
        return AISX_ERR_INVALID;
    }
    if (!(gain > 0)) { // impl :82
        set_err("Gain must be positive");
        return AISX_ERR_OUT_OF_RANGE;
    }
    if (osps != 1 && osps != 2) { // impl :61
        set_err("osps must be 1 or 2");
        return AISX_ERR_OUT_OF_RANGE;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    if ((rc = msk_check_geometry(msk_setup(sps, gain).d_sps, gain, limit)) != AISX_OK)
        return rc;
    HandlePtr<aisx_msk, aisx_msk_destroy> h(new aisx_msk());
    h->nchan = nchan;
    h->max_items = max_items;
    h->osps = osps;
    h->limit = limit;
    h->d_sps = msk_setup(sps, gain).d_sps; // :70
    h->gain = gain;
    h->gain_omega = msk_setup(sps, gain).gain_omega; // :83
    h->out_cap = msk_out_cap(h.get());
    {
        // 8 channels per wave, four waves (one per SIMD), 32 channels and 90 KB of LDS per
        // workgroup: fewer lanes per wave = fewer events of other lanes to wait for (a tag costs
        // the whole wave a general pass), and half of each CU's LDS stays free for the stages
        // that run beside this kernel on the other stream.  Measured on the whole flowgraph:
        // 7.2 / 6.3 / 5.5 ms per launch at 16 / 8 / 4 channels per wave; 8 gives the shortest
        // step (at 4 the kernel sits on all 256 CUs and slows the bandwidth-bound stages more)
        h->lpw = 8;
        if (const char* e = exp_env("AISX_MSK_INLINE_TAGS"))
            h->inline_tags = atoi(e) != 0;
        msk_tp_create(h.get());
        if (const char* e = exp_env("AISX_MSK_MAX_NOUTPUT")) // (experiments; the API is aisx_msk_set_max_noutput_items)
            h->max_noutput = std::max(0, atoi(e));
        if (const char* e = exp_env("AISX_MSK_LPW")) { // (experiments)
            const int v = atoi(e);
            if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64)
                h->lpw = v;
        }
    }
    const size_t nc = (size_t)nchan;
    if ((rc = h->d_mu.alloc(nc)) != AISX_OK || (rc = h->d_omega.alloc(nc)) != AISX_OK || (rc = h->d_div.alloc(nc)) != AISX_OK ||
        (rc = h->d_dly1.alloc(nc)) != AISX_OK || (rc = h->d_dly2.alloc(nc)) != AISX_OK || (rc = h->d_diff1.alloc(nc)) != AISX_OK ||
        (rc = h->d_nread.alloc(nc)) != AISX_OK)
        return rc;
    for (int k = 0; k < 2; k++)
        if ((rc = h->d_tprev[k].alloc(nc)) != AISX_OK || (rc = h->d_tbit[k].alloc(nc)) != AISX_OK ||
            (rc = h->d_carry[k].alloc(nc * aisx_msk::carry_cap)) != AISX_OK || (rc = h->d_carry_len[k].alloc(nc)) != AISX_OK ||
            (rc = h->d_ctag[k].alloc(nc * aisx_msk::ctag_cap)) != AISX_OK || (rc = h->d_ctag_n[k].alloc(nc)) != AISX_OK)
            return rc;
    if ((rc = h->d_produced.alloc(nc)) != AISX_OK || (rc = h->d_produced2.alloc(nc)) != AISX_OK ||
        (rc = h->d_consumed.alloc(nc)) != AISX_OK || (rc = h->d_status.alloc(nc)) != AISX_OK ||
        (rc = h->d_mmse.alloc(129 * 8)) != AISX_OK || (rc = h->d_atan.alloc(257)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_mmse, aisx_mmse_taps, sizeof(float) * 129 * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_atan, aisx_atan_table, sizeof(float) * 257, hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_msk_create: table upload failed");
        return AISX_ERR_HIP;
    }
    // (the compacted tag list for the usual hand-over capacity; grown on demand)
    if ((rc = msk_init_state(h.get())) != AISX_OK || (rc = h->d_ct.alloc(nc * (aisx_msk::ctag_cap + 1024))) != AISX_OK ||
        (rc = h->d_ct_n.alloc(nc)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipDeviceSynchronize());
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_msk_destroy(aisx_msk* h)
{
    delete h; // (~MskTp lets the units' stream come to rest before anything is released)
    return AISX_OK;
}

extern "C" int aisx_msk_set_gain(aisx_msk* h, float gain)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (!(gain > 0)) {
        h->gain = gain; // the reference stores first, then throws (:81-82): get_gain() shows the bad value
        set_err("Gain must be positive");
        return AISX_ERR_OUT_OF_RANGE;
    }
    // a gain the kernel's rings are not sized for is refused BEFORE anything is stored (as
    // set_limit / set_sps do): later calls keep running with the previous, valid loop gains
    const int rc = msk_check_geometry(h->d_sps, gain, h->limit);
    if (rc != AISX_OK)
        return rc;
    h->gain = gain;
    h->gain_omega = (float)(gain * gain * 0.25);
    return AISX_OK;
}
extern "C" float aisx_msk_get_gain(const aisx_msk* h) { return h ? h->gain : 0.f; }
extern "C" int aisx_msk_set_limit(aisx_msk* h, float limit)
{
    if (!h)
        return AISX_ERR_INVALID;
    const int rc = msk_check_geometry(h->d_sps, h->gain, limit);
    if (rc != AISX_OK)
        return rc; // (the reference accepts any value, :90-92; this build is sized, see msk_check_geometry)
    h->limit = limit;
    h->out_cap = msk_out_cap(h); // callers size their outputs by aisx_msk_out_capacity(): ask again
    return AISX_OK;
}
extern "C" float aisx_msk_get_limit(const aisx_msk* h) { return h ? h->limit : 0.f; }
extern "C" int aisx_msk_set_sps(aisx_msk* h, float sps)
{
    if (!h)
        return AISX_ERR_INVALID;
    const int rc = msk_check_geometry((float)(sps / 2.0), h->gain, h->limit);
    if (rc != AISX_OK)
        return rc;
    h->d_sps = (float)(sps / 2.0); // :70
    h->out_cap = msk_out_cap(h);
    std::vector<float> om(h->nchan, h->d_sps); // :71 d_omega = d_sps
    AISX_HIPCHK(hipMemcpy(h->d_omega, om.data(), sizeof(float) * h->nchan, hipMemcpyHostToDevice));
    return AISX_OK;
}
extern "C" float aisx_msk_get_sps(const aisx_msk* h) { return h ? h->d_sps : 0.f; }
extern "C" int aisx_msk_forecast(const aisx_msk* h, int noutput_items)
{
    return h ? msk_forecast(h->d_sps, noutput_items) : AISX_ERR_INVALID;
}
extern "C" int aisx_msk_set_max_noutput_items(aisx_msk* h, int max_noutput_items)
{
    if (!h || max_noutput_items < 0)
        return AISX_ERR_INVALID;
    h->max_noutput = max_noutput_items;
    return AISX_OK;
}
extern "C" int aisx_msk_get_max_noutput_items(const aisx_msk* h) { return h ? h->max_noutput : AISX_ERR_INVALID; }
extern "C" int aisx_msk_out_capacity(const aisx_msk* h) { return h ? h->out_cap : AISX_ERR_INVALID; }
extern "C" int aisx_msk_reset(aisx_msk* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    const int rc = msk_init_state(h);
    if (rc != AISX_OK)
        return rc;
    AISX_HIPCHK(hipDeviceSynchronize()); // (null-stream fills vs. the caller's non-blocking streams)
    return AISX_OK;
}

void aisx::msk_fill_common(aisx_msk* h, MskParams& p)
{
    msk_fill_state(h, p);
    p.osps = h->osps;
    p.ct = h->d_ct;
    p.ct_n = h->d_ct_n;
    p.ct_cap = h->ct_cap();
    p.lds_tab_off = msk_lds_taboff(h->lpw);
    p.lpw = h->lpw;
    p.lds_wave_stride = msk_lds_wave(h->lpw);
    p.tq_stride = h->lpw;
    p.tq_private = 0;
    p.lds_ring_off = msk_lds_ringoff(h->lpw);
    p.inline_tags = h->inline_tags;
    p.pair_core = h->pair_core;
    p.stream_mode = 1;
    p.gr_ninput = 0;
    p.gr_noutput = 0;
    p.ff = 0;
    p.nrst = nullptr;
    p.rst = nullptr;
    p.res = nullptr;
    p.pieces = nullptr;
    p.npieces = nullptr;
    p.ct_nc = nullptr;
}

// room in h->d_ct for `need` tags per channel; a list that grows in mid-life waits for the work on `st` that reads the old one
static int msk_ct_reserve(aisx_msk* h, int need, hipStream_t st)
{
    if (h->d_ct && need <= h->ct_cap())
        return AISX_OK;
    AISX_HIPCHK(hipStreamSynchronize(st));
    const int rc = h->d_ct.reserve((size_t)h->nchan * (size_t)need);
    if (rc != AISX_OK)
        return rc;
    // dev_alloc's zero fill runs on the null stream: it must not trail into the kernels on `st`
    AISX_HIPCHK(hipDeviceSynchronize());
    return AISX_OK;
}

int aisx::msk_launch_tagprep(aisx_msk* h, const tag_rec* d_tags, const int* d_tag_counts, int tag_cap, hipStream_t st, int* d_ct_nc,
                             const msk_ctag* ctl_new, const int* ctl_new_n, int ctl_new_cap, int ctl_new_pre)
{
    const int need = aisx_msk::ctag_cap + (ctl_new ? ctl_new_cap - ctl_new_pre : (d_tags ? tag_cap : 0));
    const int rc = msk_ct_reserve(h, need, st);
    if (rc != AISX_OK)
        return rc;
    TagPrepParams t;
    t.nchan = h->nchan;
    t.ctag_in = h->d_ctag[h->cur];
    t.ctag_n_in = h->d_ctag_n[h->cur];
    t.ctag_cap = aisx_msk::ctag_cap;
    t.tags = d_tags;
    t.tag_count = d_tag_counts;
    t.tag_cap = tag_cap;
    t.nread = h->d_nread;
    t.ct = h->d_ct;
    t.ct_n = h->d_ct_n;
    t.ct_cap = h->ct_cap();
    t.ct_nc = d_ct_nc;
    t.ctl_new = ctl_new;
    t.ctl_new_n = ctl_new_n;
    t.ctl_new_cap = ctl_new_cap;
    t.ctl_new_pre = ctl_new ? ctl_new_pre : 0;
    t.W = ctl_new ? h->total_in : 0;
    hipLaunchKernelGGL(k_msk_tagprep, dim3((h->nchan + 3) / 4), dim3(256), 0, st, t); // a wave per channel
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

// the NRZI bit tail over the symbols the timing-recovery kernel just wrote
static int msk_launch_bittail(aisx_msk* h, const cf* syms, long sym_stride, const int* produced, uint8_t* bits,
                              long bit_stride, int max_out, hipStream_t st)
{
    BitTailParams b;
    b.nchan = h->nchan;
    b.syms = syms;
    b.sym_stride = sym_stride;
    b.produced = produced;
    b.bits = bits;
    b.bit_stride = bit_stride;
    b.prev_sym_in = h->d_tprev[h->tcur];
    b.prev_bit_in = h->d_tbit[h->tcur];
    b.prev_sym_out = h->d_tprev[h->tcur ^ 1];
    b.prev_bit_out = h->d_tbit[h->tcur ^ 1];
    b.atan_tab = h->d_atan;
    const int nseg = std::max(1, (max_out + BT_SEG - 1) / BT_SEG);
    hipLaunchKernelGGL(k_bittail, dim3(nseg, h->nchan), dim3(BT_T), 0, st, b);
    AISX_HIPCHK(hipGetLastError());
    h->tcur ^= 1;
    return AISX_OK;
}

// the serial kernel over the call's items (hipEvents around it for aisx_msk_set_profiling)
static int msk_launch_serial(aisx_msk* h, const MskCall& c, float* d_err, float* d_mu)
{
    MskParams p;
    msk_fill_common(h, p);
    msk_fill_call(c, p);
    p.err = d_err;
    p.mu_out = d_mu;
    p.sym_al16 = ((uintptr_t)c.syms % 16 == 0) && (c.out_stride % 2 == 0);
    if (c.fused_bits) { // the bit tail inside the symbol flush: msk_launch_bittail's ports
        p.bits = c.fused_bits;
        p.bit_stride = c.out_stride;
        p.bit_al2 = ((uintptr_t)c.fused_bits % 2 == 0) && (c.out_stride % 2 == 0);
        p.prev_sym_in = h->d_tprev[h->tcur];
        p.prev_bit_in = h->d_tbit[h->tcur];
        p.prev_sym_out = h->d_tprev[h->tcur ^ 1];
        p.prev_bit_out = h->d_tbit[h->tcur ^ 1];
        p.atan_tab = h->d_atan;
    }
    int rc;
    if ((rc = h->prof.begin(c.st)) != AISX_OK ||
        (rc = msk_launch(p, (h->nchan + msk_wg_channels(h->lpw) - 1) / msk_wg_channels(h->lpw), c.st)) != AISX_OK ||
        (rc = h->prof.end(c.st)) != AISX_OK)
        return rc;
    if (c.fused_bits)
        h->tcur ^= 1; // (as msk_launch_bittail does: fused and unfused calls may alternate)
    return AISX_OK;
}

// The kernel can do the call's bit tail itself: the serial kernel in a build with a symbol stage (k_msk.h, STG: osps 1,
// err / mu ports open, at most 8 channels per wave).  The time-parallel recovery keeps k_bittail (its units' symbols are
// gathered from staging rows).
static bool msk_fused_applies(const aisx_msk* h, bool tp, const float* d_err, const float* d_mu, const uint8_t* d_bits)
{
    return h->fused_tail && d_bits && !tp && h->osps == 1 && !d_err && !d_mu && msk_staged(h->lpw);
}

static int msk_process_stream(aisx_msk* h, const aisx_cf32* d_in, long in_stride, int n, const aisx_tag* d_tags,
                              const int* d_tag_counts, int tag_cap, aisx_cf32* d_syms, float* d_err, float* d_mu, uint8_t* d_bits,
                              long out_stride, int* d_produced, void* stream, void* ready_event)
{
    if (!h || !d_in || n < 1 || n > h->max_items || in_stride < n || (d_tags && (!d_tag_counts || tag_cap < 1))) {
        set_err("aisx_msk_process_stream: bad argument");
        return AISX_ERR_INVALID;
    }
    if (out_stride < 1) {
        set_err("aisx_msk_process_stream: out_stride < 1");
        return AISX_ERR_INVALID;
    }
    if (out_stride >= (1L << 23)) {
        set_err("aisx_msk_process_stream: out_stride %ld too large (the 64 rows of a wave must lie within 4 GiB)", out_stride);
        return AISX_ERR_INVALID;
    }
    const hipStream_t st = (hipStream_t)stream;
    const bool tp = msk_tp_applies(h, d_err, d_mu);
    const int par = h->callpar;
    h->callpar ^= 1;
    MskCall c = { (const cf*)d_in, in_stride, n, (const tag_rec*)d_tags, d_tag_counts, tag_cap, (cf*)d_syms, nullptr, out_stride,
                  (int)std::min<long>(out_stride, 0x7fffffff), par, st, ready_event };
    int rc;
    hipStream_t su = st; // where the prepass runs: the time-parallel one may have a stream of its own
    if ((rc = tp ? msk_tp_prepass(h, c, &su) : msk_launch_tagprep(h, c.tags, c.tag_counts, c.tag_cap, st)) != AISX_OK)
        return rc;
    if (h->ev_prep) { // (the caller's tag records have been read)
        AISX_HIPCHK(hipEventRecord(h->ev_prep, su));
        h->ev_prep_set = true;
    }
    const bool fused = msk_fused_applies(h, tp, d_err, d_mu, d_bits);
    if (fused) {
        // Nothing of this call goes to the tail stream.  Bit tails still queued there (unfused calls before this one) hold
        // the tail state this kernel reads and writes, and the internal `produced` array of this parity: waited for once.
        for (int k = 0; k < 2; k++)
            if (h->tail_on && h->tail_pend[k]) {
                AISX_HIPCHK(hipStreamWaitEvent(st, h->ev_tail[k], 0));
                h->tail_pend[k] = false;
            }
        c.fused_bits = d_bits;
    } else if (h->tail_on && h->ev_tail_set[par]) { // the bit tail of two calls ago may still read this parity's buffers
        AISX_HIPCHK(hipStreamWaitEvent(st, h->ev_tail[par], 0));
        h->tail_pend[par] = false;
    }
    if (!c.syms && !fused) { // the kernel always writes symbols (the bit tail reads them back): give them a home
        const size_t need = (size_t)h->nchan * (size_t)out_stride;
        if (need > h->d_symscratch[par].cap()) {
            AISX_HIPCHK(hipStreamSynchronize(st));
            if ((rc = h->d_symscratch[par].reserve(need)) != AISX_OK)
                return rc;
            AISX_HIPCHK(hipDeviceSynchronize()); // (the zero fill runs on the null stream)
        }
        c.syms = h->d_symscratch[par];
    }
    c.produced = d_produced ? d_produced : (par ? h->d_produced2 : h->d_produced);
    if ((rc = tp ? msk_tp_units_join(h, c) : msk_launch_serial(h, c, d_err, d_mu)) != AISX_OK)
        return rc;
    h->cur ^= 1;
    h->total_in += (unsigned long long)n;
    // the units' symbols: with bits only and a tail stream they are gathered there, ahead of the bit tail; the
    // caller's own symbol rows are complete when `stream` is
    const bool gather_on_tail = tp && !d_syms && d_bits && h->tail_on;
    if (tp && !gather_on_tail && (rc = msk_tp_gather(h, c, false)) != AISX_OK)
        return rc;
    if (!d_bits)
        return AISX_OK;
    h->last_fused = fused;
    h->last_st = st;
    if (fused) // (the kernel wrote them; complete on `stream`, whether a tail stream is set or not)
        return AISX_OK;
    // a call produces at most forecast^-1(n + carry) symbols; out_cap bounds it too
    const double wmin = (double)h->d_sps - fabs((double)h->limit);
    const int max_out = std::min<long>(c.out_cap, (long)ceil((n + aisx_msk::carry_cap) / (2.0 * wmin)) * h->osps + 16);
    hipStream_t ts = st;
    if (h->tail_on) { // the bit tail has no part in the recurrence: let the next call start
        AISX_HIPCHK(hipEventRecord(h->ev_msk, st));
        AISX_HIPCHK(hipStreamWaitEvent(h->tail_stream, h->ev_msk, 0));
        ts = h->tail_stream;
        if (gather_on_tail && (rc = msk_tp_gather(h, c, true)) != AISX_OK)
            return rc;
    }
    if ((rc = msk_launch_bittail(h, c.syms, out_stride, c.produced, d_bits, out_stride, max_out, ts)) != AISX_OK)
        return rc;
    if (h->tail_on) {
        AISX_HIPCHK(hipEventRecord(h->ev_tail[par], h->tail_stream));
        h->ev_tail_set[par] = true;
        h->tail_pend[par] = true;
    }
    return AISX_OK;
}

extern "C" int aisx_msk_process_stream(aisx_msk* h, const aisx_cf32* d_in, long in_stride, int n,
                                       const aisx_tag* d_tags, const int* d_tag_counts, int tag_cap, aisx_cf32* d_syms,
                                       float* d_err, float* d_mu, uint8_t* d_bits, long out_stride, int* d_produced,
                                       void* stream)
{
    return msk_process_stream(h, d_in, in_stride, n, d_tags, d_tag_counts, tag_cap, d_syms, d_err, d_mu, d_bits, out_stride, d_produced,
                              stream, nullptr);
}

extern "C" int aisx_msk_process_stream_after(aisx_msk* h, const aisx_cf32* d_in, long in_stride, int n,
                                             const aisx_tag* d_tags, const int* d_tag_counts, int tag_cap, aisx_cf32* d_syms,
                                             float* d_err, float* d_mu, uint8_t* d_bits, long out_stride, int* d_produced,
                                             void* stream, void* ready_event)
{
    return msk_process_stream(h, d_in, in_stride, n, d_tags, d_tag_counts, tag_cap, d_syms, d_err, d_mu, d_bits, out_stride, d_produced,
                              stream, ready_event);
}

extern "C" int aisx_msk_set_tail_stream(aisx_msk* h, void* tail_stream, int enable)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (!enable) {
        h->tail_on = false;
        return AISX_OK;
    }
    int rc;
    if ((rc = h->ev_msk.ensure(hipEventDisableTiming)) != AISX_OK || (rc = h->ev_tail[0].ensure(hipEventDisableTiming)) != AISX_OK ||
        (rc = h->ev_tail[1].ensure(hipEventDisableTiming)) != AISX_OK)
        return rc;
    h->tail_stream = (hipStream_t)tail_stream;
    h->tail_on = true;
    return AISX_OK;
}

extern "C" int aisx_msk_wait_tail(aisx_msk* h, void* stream)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (h->tail_on) {
        for (int k = 0; k < 2; k++)
            if (h->ev_tail_set[k])
                AISX_HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_tail[k], 0));
        // a fused call's bits are complete on the call's own stream: an event there now stands behind them
        if (h->last_fused && h->last_st != (hipStream_t)stream) {
            AISX_HIPCHK(hipEventRecord(h->ev_msk, h->last_st));
            AISX_HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_msk, 0));
        }
    }
    return AISX_OK;
}

extern "C" int aisx_msk_set_fused_tail(aisx_msk* h, int on)
{
    if (!h)
        return AISX_ERR_INVALID;
    h->fused_tail = on != 0;
    return AISX_OK;
}
extern "C" int aisx_msk_get_fused_tail(const aisx_msk* h) { return h ? (h->fused_tail ? 1 : 0) : AISX_ERR_INVALID; }
extern "C" int aisx_msk_last_tail_fused(const aisx_msk* h) { return h ? (h->last_fused ? 1 : 0) : AISX_ERR_INVALID; }

extern "C" int aisx_msk_set_pair_core(aisx_msk* h, int mode)
{
    if (!h || (mode != 0 && mode != 1))
        return AISX_ERR_INVALID;
    h->pair_core = mode;
    return AISX_OK;
}
extern "C" int aisx_msk_get_pair_core(const aisx_msk* h) { return h ? h->pair_core : AISX_ERR_INVALID; }

extern "C" int aisx_msk_wait_prepass(aisx_msk* h, void* stream)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (!h->ev_prep) // first use: from now on every aisx_msk_process_stream records the event
        return h->ev_prep.ensure(hipEventDisableTiming);
    if (h->ev_prep_set) {
        AISX_HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_prep, 0));
        // The event fires when the tag prepass ends -- the same moment the recovery kernel behind
        // it becomes ready on its own stream: which of the two queues the dispatcher serves first
        // is then a race (it used to be decided by two already-satisfied barrier packets that
        // happened to stand behind this one on `stream`: ~10 us).  A wave that sleeps for
        // aisx_msk_set_head_start()'s microseconds on `stream` decides it (off unless asked for).
        if (h->head_start_ticks > 0) {
            hipLaunchKernelGGL(k_msk_headstart, dim3(1), dim3(64), 0, (hipStream_t)stream, h->head_start_ticks);
            AISX_HIPCHK(hipGetLastError());
        }
    }
    return AISX_OK;
}

extern "C" int aisx_msk_set_head_start(aisx_msk* h, int microseconds)
{
    if (!h || microseconds < 0 || microseconds > 1000) {
        set_err("aisx_msk_set_head_start: 0..1000 microseconds");
        return AISX_ERR_INVALID;
    }
    // the sleeping wave counts wall_clock64() ticks: the constant-rate counter, hipDeviceAttributeWallClockRate kHz
    int dev = 0, khz = 0;
    AISX_HIPCHK(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        khz = 100000; // gfx950: 100 MHz
    h->head_start_ticks = (unsigned)((long long)microseconds * khz / 1000);
    return AISX_OK;
}

extern "C" int aisx_msk_geometry(const aisx_msk* h, int* nchan, int* max_items)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (nchan)
        *nchan = h->nchan;
    if (max_items)
        *max_items = h->max_items;
    return AISX_OK;
}

extern "C" int aisx_msk_placement(const aisx_msk* h, int* workgroups, int* lds_bytes_per_workgroup)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (workgroups)
        *workgroups = (h->nchan + msk_wg_channels(h->lpw) - 1) / msk_wg_channels(h->lpw);
    if (lds_bytes_per_workgroup)
        *lds_bytes_per_workgroup = msk_lds_bytes(h->lpw);
    return AISX_OK;
}

extern "C" int aisx_msk_set_profiling(aisx_msk* h, int on) { return h ? h->prof.set_profiling(on) : AISX_ERR_INVALID; }

extern "C" int aisx_msk_kernel_ms_history(aisx_msk* h, float* ms, int cap, int* n)
{
    return h && ms && n ? h->prof.history(ms, cap, n) : AISX_ERR_INVALID;
}


extern "C" int aisx_msk_last_status(aisx_msk* h, int* status, void* stream)
{
    if (!h || !status)
        return AISX_ERR_INVALID;
    std::vector<int> st(h->nchan);
    AISX_HIPCHK(hipMemcpyAsync(st.data(), h->d_status, sizeof(int) * h->nchan, hipMemcpyDeviceToHost,
                               (hipStream_t)stream));
    AISX_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int acc = 0;
    for (int v : st)
        acc |= v;
    *status = acc;
    return AISX_OK;
}

extern "C" int aisx_msk_status_device(const aisx_msk* h, const int** d_status)
{
    if (!h || !d_status)
        return AISX_ERR_INVALID;
    *d_status = h->d_status;
    return AISX_OK;
}

// GNU Radio path: the call's control words set, and its three result words gathered behind the symbols' header,
// by one-thread kernels -- a blocking hipMemcpy of four bytes costs as much as a launch, and a call had eight of them
__global__ void k_msk_host_setup(int* tagn, int ntags, unsigned long long* nread, unsigned long long R, int* carry_len, int* ctag_n)
{
    *tagn = ntags;
    *nread = R;
    *carry_len = 0;
    *ctag_n = 0;
}
__global__ void k_msk_host_pack(int* hdr, const int* produced, const int* consumed, const int* status)
{
    hdr[0] = *produced;
    hdr[1] = *consumed;
    hdr[2] = *status;
    hdr[3] = 0;
}

extern "C" int aisx_msk_general_work_host(aisx_msk* h, int noutput_items, int ninput_items, const aisx_cf32* in,
                                          aisx_cf32* out, float* out_err, float* out_mu, uint8_t* out_bits,
                                          const aisx_tag* tags, int ntags, uint64_t nitems_read,
                                          int in_has_lookahead, int* consumed, int* produced)
{
    if (!h || !in || !out || !consumed || !produced || noutput_items < 0 || ninput_items < 0 || ntags < 0)
        return AISX_ERR_INVALID;
    if (h->nchan != 1) {
        set_err("aisx_msk_general_work_host: handle has %d channels, the GNU Radio path needs 1", h->nchan);
        return AISX_ERR_INVALID;
    }
    *consumed = 0;
    *produced = 0;
    if (ninput_items == 0 || noutput_items == 0)
        return AISX_OK;
    int rc;
    // the interpolator reads up to in[ninput_items] (one past): stage one spare item
    const int nin = ninput_items + 1;
    // (symbols behind a 16-byte header {produced, consumed, status, 0}: one copy brings back both)
    bool grown = false;
    if ((rc = h->d_st_in.reserve(nin)) != AISX_OK || (rc = h->d_st_blk.reserve((size_t)noutput_items + 2, true, &grown)) != AISX_OK ||
        (rc = h->d_st_err.reserve(noutput_items)) != AISX_OK || (rc = h->d_st_mu.reserve(noutput_items)) != AISX_OK ||
        (rc = h->d_st_bits.reserve(noutput_items)) != AISX_OK || (rc = h->d_st_tags.reserve(ntags + 1)) != AISX_OK ||
        (rc = h->d_st_tagn.reserve(1)) != AISX_OK)
        return rc;
    h->d_st_sym = h->d_st_blk + 2;
    if (grown)
        h->st_host.resize((size_t)noutput_items + 2);
    AISX_HIPCHK(hipMemcpy(h->d_st_in, in, sizeof(cf) * (in_has_lookahead ? nin : ninput_items), hipMemcpyHostToDevice));
    if (!in_has_lookahead)
        AISX_HIPCHK(hipMemset(h->d_st_in + ninput_items, 0, sizeof(cf)));
    if (ntags > 0)
        AISX_HIPCHK(hipMemcpy(h->d_st_tags, tags, sizeof(tag_rec) * ntags, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_msk_host_setup, dim3(1), dim3(1), 0, 0, h->d_st_tagn.get(), ntags, h->d_nread.get(),
                       (unsigned long long)nitems_read, h->d_carry_len[h->cur].get(), h->d_ctag_n[h->cur].get());
    AISX_HIPCHK(hipGetLastError());
    if ((rc = msk_launch_tagprep(h, h->d_st_tags, h->d_st_tagn, ntags + 1, 0)) != AISX_OK)
        return rc;
    MskParams p;
    msk_fill_common(h, p);
    p.in = h->d_st_in;
    p.in_stride = nin;
    p.n = ninput_items;
    p.stream_mode = 0;
    p.gr_ninput = ninput_items;
    p.gr_noutput = noutput_items;
    p.syms = h->d_st_sym;
    p.err = h->d_st_err;
    p.mu_out = h->d_st_mu;
    p.out_stride = noutput_items;
    p.sym_al16 = ((uintptr_t)h->d_st_sym % 16 == 0) && (noutput_items % 2 == 0);
    p.out_cap = noutput_items;
    p.produced = h->d_produced;
    if ((rc = msk_launch(p, 1, 0)) != AISX_OK)
        return rc;
    h->cur ^= 1;
    // (the NRZI bit tail only for a caller that takes its output -- the gr::ais block does not, python/ais_demod.py:48-52
    // are blocks of their own there: its state then carries on from the last call that did)
    if (out_bits && (rc = msk_launch_bittail(h, h->d_st_sym, noutput_items, h->d_produced, h->d_st_bits, noutput_items,
                                             noutput_items, 0)) != AISX_OK)
        return rc;
    hipLaunchKernelGGL(k_msk_host_pack, dim3(1), dim3(1), 0, 0, (int*)h->d_st_blk.get(), h->d_produced.get(), h->d_consumed.get(), h->d_status.get());
    AISX_HIPCHK(hipGetLastError());
    // header + every symbol the call may have produced in one copy (at most noutput_items of them: a few KB)
    AISX_HIPCHK(hipMemcpy(h->st_host.data(), h->d_st_blk, sizeof(cf) * ((size_t)noutput_items + 2), hipMemcpyDeviceToHost));
    const int* hdr = (const int*)h->st_host.data();
    *produced = hdr[0];
    *consumed = hdr[1];
    const int st = hdr[2];
    const int np = *produced;
    if (np > 0) {
        memcpy(out, h->st_host.data() + 2, sizeof(cf) * (size_t)np);
        if (out_err)
            AISX_HIPCHK(hipMemcpy(out_err, h->d_st_err, sizeof(float) * np, hipMemcpyDeviceToHost));
        if (out_mu)
            AISX_HIPCHK(hipMemcpy(out_mu, h->d_st_mu, sizeof(float) * np, hipMemcpyDeviceToHost));
        if (out_bits)
            AISX_HIPCHK(hipMemcpy(out_bits, h->d_st_bits, np, hipMemcpyDeviceToHost));
    }
    if (st & MSK_ST_INTERP_RANGE) {
        set_err("mmse_fir_interpolator_cc: imu out of bounds."); // upstream std::runtime_error
        return AISX_ERR_RUNTIME;
    }
    return AISX_OK;
}
