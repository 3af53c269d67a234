// aisx_hdlc.hip -- C ABI of the batched HDLC deframer (include/aisx.h, aisx_hdlc_batch_*): per call, one wave per
// channel deframes that channel's bits (k_hdlc.h: hdlc_deframe_body) into a staging area of its own, one workgroup
// places the channels' records one behind the other (hdlc_scan_body) and one wave per channel copies them there
// (hdlc_gather_body).  Everything is queued on the caller's stream; the per-channel bit counts are read on the device.
#include <limits.h>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "aisx_repair.h"
#include "k_hdlc.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(sizeof(HdlcRule) == sizeof(aisx_hdlc_rule) && HD_MAX_RULES == AISX_HDLC_MAX_RULES, "repair rule layout");
static_assert(HD_LDS_BYTES_REPAIR + 2 * HD_SCAN_T * 8 <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(HD_T) void k_hdlc_deframe(HdlcParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[HD_LDS_BYTES];
    DevCtx cx{ smem };
    hdlc_deframe_body(cx, p);
}

// the deframer of a handle with repair rules
__global__ __launch_bounds__(HD_T) void k_hdlc_deframe_repair(HdlcParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[HD_LDS_BYTES_REPAIR];
    DevCtx cx{ smem };
    hdlc_deframe_body<DevCtx, true>(cx, p);
}

// the deframer of a handle with repair rules and an event mask that is not the single event alone
__global__ __launch_bounds__(HD_T) void k_hdlc_deframe_events(HdlcParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[HD_LDS_BYTES_REPAIR];
    DevCtx cx{ smem };
    hdlc_deframe_body<DevCtx, true, true>(cx, p);
}

__global__ __launch_bounds__(HD_SCAN_T) void k_hdlc_scan(HdlcScanParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * HD_SCAN_T * 8];
    DevCtx cx{ smem };
    hdlc_scan_body(cx, p);
}

__global__ __launch_bounds__(HD_T) void k_hdlc_gather(HdlcGatherParams p)
{
    DevCtx cx{ nullptr };
    hdlc_gather_body(cx, p);
}

struct aisx_hdlc_batch {
    explicit aisx_hdlc_batch(const HdlcPlan& plan) : pl(plan) {}
    int dev = 0;
    const HdlcPlan pl;         // the arguments, the sizes derived from them and the per-call sequence (k_hdlc.h)
    DevBuf<HdlcState> d_st;
    DevBuf<unsigned long long> d_carry;
    DevBuf<HdlcRec> d_srec;
    DevBuf<unsigned char> d_sbytes;
    DevBuf<int> d_cnt;         // [nchan] records, [nchan] bytes
    DevBuf<long long> d_base;  // [nchan] record bases, [nchan] byte bases
    DevBuf<int> d_count;       // [0] found, [1] kept, [2] bad-count flag
    Event done;                // behind the last call's work (reset waits for it)
    DevBuf<HdlcRec> d_out;
    DevBuf<unsigned char> d_out_bytes;
    DevBuf<int> d_fix;         // [max_pdus] the records' repair marks: all -1 while the handle has no rules
    // single-bit repair, made by the first aisx_hdlc_batch_set_repair with rules
    int nrules = 0;
    DevBuf<HdlcRule> d_rules;
    DevBuf<unsigned short> d_syn_inv;
    DevBuf<int> d_sfix;        // [nchan][rec_cap]
    // error events (aisx_hdlc_batch_set_repair_events): the mask, and for one that is not the single event alone its table
    int events = AISX_HDLC_EV_SINGLE;
    int ev_tab_events = 0;     // the mask d_ev_tab holds the table of, 0 = none yet
    DevBuf<unsigned short> d_ev_tab;
};

extern "C" int aisx_hdlc_batch_destroy(aisx_hdlc_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_create(aisx_hdlc_batch** out, int length_min, int length_max, int nchan, int max_bits,
                                      int max_pdus)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = HdlcPlan::check(length_min, length_max, nchan, max_bits, max_pdus)) {
        set_err("aisx_hdlc_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_hdlc_batch, aisx_hdlc_batch_destroy> h(new aisx_hdlc_batch(HdlcPlan(length_min, length_max, nchan, max_bits, max_pdus)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const HdlcPlan& pl = h->pl;
    if ((rc = h->d_st.alloc(pl.st)) != AISX_OK || (rc = h->d_carry.alloc(pl.carry)) != AISX_OK ||
        (rc = h->d_srec.alloc(pl.srec)) != AISX_OK || (rc = h->d_sbytes.alloc(pl.sbytes)) != AISX_OK ||
        (rc = h->d_cnt.alloc(pl.cnt)) != AISX_OK || (rc = h->d_base.alloc(pl.base)) != AISX_OK ||
        (rc = h->d_count.alloc(pl.count)) != AISX_OK || (rc = h->d_out.alloc(pl.out)) != AISX_OK ||
        (rc = h->d_out_bytes.alloc(pl.out_bytes)) != AISX_OK || (rc = h->d_fix.alloc(pl.fix)) != AISX_OK ||
        (rc = h->done.create(hipEventDisableTiming)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipMemset(h->d_fix, 0xFF, sizeof(int) * pl.fix.n));
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_reset(aisx_hdlc_batch* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipEventSynchronize(h->done)); // (the last call's kernels; nothing else on the device)
    AISX_HIPCHK(hipMemsetAsync(h->d_st, 0, sizeof(HdlcState) * h->pl.st.n, nullptr));
    AISX_HIPCHK(hipMemsetAsync(h->d_carry, 0, sizeof(unsigned long long) * h->pl.carry.n, nullptr));
    AISX_HIPCHK(hipMemsetAsync(h->d_cnt, 0, sizeof(int) * h->pl.cnt.n, nullptr));
    AISX_HIPCHK(hipMemsetAsync(h->d_count, 0, sizeof(int) * h->pl.count.n, nullptr));
    AISX_HIPCHK(hipStreamSynchronize(nullptr)); // (done before the next call, whatever stream that is queued on)
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_set_repair(aisx_hdlc_batch* h, const aisx_hdlc_rule* rules, int nrules)
{
    return aisx_hdlc_batch_set_repair_events(h, rules, nrules, AISX_HDLC_EV_SINGLE);
}

extern "C" int aisx_hdlc_batch_set_repair_events(aisx_hdlc_batch* h, const aisx_hdlc_rule* rules, int nrules, int events)
{
    if (!h || !hdlc_events_ok(events) || hdlc_rules_check(rules, nrules, h->pl.lmin, h->pl.lmax) != AISX_OK) {
        set_err("aisx_hdlc_batch_set_repair: need a handle, at most %d rules with distinct payload lengths in "
                "[length_min - 2, length_max - 2] and reserved = 0, and a mask of AISX_HDLC_EV_* events",
                AISX_HDLC_MAX_RULES);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipEventSynchronize(h->done)); // (the last call's kernels read the rules and the table in place)
    int rc;
    DevBuf<unsigned short> ev_tab; // (a mask's table is made beside the one in use, which stays if anything below fails)
    const bool new_tab = nrules > 0 && events != AISX_HDLC_EV_SINGLE && h->ev_tab_events != events;
    if (new_tab) {
        if ((rc = ev_tab.alloc(h->pl.syn)) != AISX_OK)
            return rc;
        AISX_HIPCHK(hipMemcpy(ev_tab, hdlc_event_table(events), sizeof(unsigned short) * 65536, hipMemcpyHostToDevice));
    }
    if (nrules > 0) {
        if (!h->d_syn_inv) {
            DevBuf<HdlcRule> r;
            DevBuf<unsigned short> t;
            DevBuf<int> f;
            if ((rc = r.alloc(h->pl.rules)) != AISX_OK || (rc = t.alloc(h->pl.syn)) != AISX_OK || (rc = f.alloc(h->pl.sfix)) != AISX_OK)
                return rc;
            AISX_HIPCHK(hipMemcpy(t, hdlc_syndrome_table(), sizeof(unsigned short) * 65536, hipMemcpyHostToDevice));
            h->d_rules = std::move(r);
            h->d_syn_inv = std::move(t);
            h->d_sfix = std::move(f);
        }
        AISX_HIPCHK(hipMemcpy(h->d_rules, rules, sizeof(HdlcRule) * nrules, hipMemcpyHostToDevice));
    } else if (h->nrules > 0) {
        AISX_HIPCHK(hipMemset(h->d_fix, 0xFF, sizeof(int) * h->pl.fix.n)); // (nothing writes the marks without rules)
        AISX_HIPCHK(hipStreamSynchronize(nullptr));
    }
    if (new_tab) {
        h->d_ev_tab = std::move(ev_tab);
        h->ev_tab_events = events;
    }
    h->nrules = nrules;
    h->events = events;
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_process(aisx_hdlc_batch* h, const uint8_t* d_bits, long bits_stride, const int* d_nbits,
                                       void* stream)
{
    if (!h || !d_bits || !d_nbits || bits_stride < h->pl.max_bits) {
        set_err("aisx_hdlc_batch_process: bits, counts and a row stride of at least max_bits (%d) are needed",
                h ? h->pl.max_bits : 0);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const bool single = h->events == AISX_HDLC_EV_SINGLE;
    const HdlcBufs b = { h->d_st,  h->d_carry,     h->d_srec, h->d_sbytes, h->d_cnt,  h->d_base, h->d_count,
                         h->d_out, h->d_out_bytes, h->d_fix,  h->d_rules,  h->d_sfix, single ? h->d_syn_inv : h->d_ev_tab };
    hipError_t err = hipSuccess;
    h->pl.process(b, d_bits, bits_stride, d_nbits, h->nrules, !single, [&](const PlanLaunch& l, const HdlcCall& c) {
        const dim3 grid(l.gx, l.gy), threads(l.threads);
        switch (l.kernel) {
        case HD_K_DEFRAME: hipLaunchKernelGGL(k_hdlc_deframe, grid, threads, 0, st, c.p); break;
        case HD_K_DEFRAME_REPAIR: hipLaunchKernelGGL(k_hdlc_deframe_repair, grid, threads, 0, st, c.p); break;
        case HD_K_DEFRAME_EVENTS: hipLaunchKernelGGL(k_hdlc_deframe_events, grid, threads, 0, st, c.p); break;
        case HD_K_SCAN: hipLaunchKernelGGL(k_hdlc_scan, grid, threads, 0, st, c.s); break;
        case HD_K_GATHER: hipLaunchKernelGGL(k_hdlc_gather, grid, threads, 0, st, c.g); break;
        }
        return (err = hipGetLastError()) == hipSuccess;
    });
    AISX_LAUNCHCHK(err);
    AISX_HIPCHK(hipEventRecord(h->done, st));
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_results_device(const aisx_hdlc_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                              const int** d_count)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_pdus)
        *d_pdus = (const aisx_pdu*)h->d_out.get();
    if (d_bytes)
        *d_bytes = h->d_out_bytes;
    if (d_count)
        *d_count = h->d_count;
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_read(aisx_hdlc_batch* h, aisx_pdu* pdus, int pdu_cap, uint8_t* bytes, long bytes_cap,
                                    int* npdus, void* stream)
{
    if (!h || !npdus || pdu_cap < 0 || bytes_cap < 0 || (pdu_cap > 0 && !pdus) || (bytes_cap > 0 && !bytes))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[3] = { 0, 0, 0 };
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    int k = cnt[1] < pdu_cap ? cnt[1] : pdu_cap;
    if (k > 0)
        AISX_HIPCHK(hipMemcpyAsync(pdus, h->d_out, sizeof(aisx_pdu) * k, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    while (k > 0 && pdus[k - 1].offset + pdus[k - 1].len > bytes_cap) // (records are in byte order: a prefix again)
        k--;
    const long long nb = k > 0 ? pdus[k - 1].offset + pdus[k - 1].len : 0;
    if (nb > 0)
        AISX_HIPCHK(hipMemcpyAsync(bytes, h->d_out_bytes, (size_t)nb, hipMemcpyDeviceToHost, st));
    if (cnt[2])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + 2, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *npdus = cnt[0];
    if (cnt[2]) {
        set_err("aisx_hdlc_batch_read: a channel's bit count was outside [0, %d]: that channel was not advanced",
                h->pl.max_bits);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[0]) {
        set_err("aisx_hdlc_batch_read: %d PDUs found, %d kept", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_repairs_device(const aisx_hdlc_batch* h, const int32_t** d_fix_bits)
{
    if (!h || !d_fix_bits)
        return AISX_ERR_INVALID;
    *d_fix_bits = h->d_fix;
    return AISX_OK;
}

extern "C" int aisx_hdlc_batch_read_repairs(aisx_hdlc_batch* h, int32_t* fix_bits, int cap, int* n, void* stream)
{
    if (!h || !n || cap < 0 || (cap > 0 && !fix_bits))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[2] = { 0, 0 };
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    const int k = cnt[1] < cap ? cnt[1] : cap;
    if (k > 0)
        AISX_HIPCHK(hipMemcpyAsync(fix_bits, h->d_fix, sizeof(int32_t) * k, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *n = cnt[0];
    if (k < cnt[0]) {
        set_err("aisx_hdlc_batch_read_repairs: %d PDUs found, the marks of %d kept", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
