// aisx_dedup.hip -- C ABI of the duplicate suppression in device memory (include/aisx.h, aisx_dedup_batch_*; bodies in
// k_dedup.h): five small kernels per call, queued on the caller's stream; the record count is read on the device.
#include <string.h>

#include <algorithm>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_dedup.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(DD_NCNT == AISX_DEDUP_NCNT, "counts layout");

#define DD_KERNEL(name, body)                                                \
    __global__ __launch_bounds__(DD_T) void name(DdParams p)                 \
    {                                                                        \
        __shared__ __attribute__((aligned(16))) char smem[DD_LDS_BYTES];     \
        DevCtx cx{ smem };                                                   \
        body(cx, p);                                                         \
    }
DD_KERNEL(k_dd_clear, dd_clear_body)
DD_KERNEL(k_dd_find, dd_find_body)
DD_KERNEL(k_dd_classify, dd_classify_body)
DD_KERNEL(k_dd_assign, dd_assign_body)
DD_KERNEL(k_dd_fill, dd_fill_body)

struct aisx_dedup_batch {
    explicit aisx_dedup_batch(const DdPlan& plan) : pl(plan) {}
    int dev = 0;
    DdPlan pl;                   // the arguments, the sizes derived from them, the ring's stamps and the per-call sequence
    const uint8_t* d_bytes = nullptr; // the last call's producer's
    DevBuf<dd_u64> d_ckey, d_ring;
    DevBuf<int> d_cfirst, d_ccount, d_cval, d_rslot, d_bsum, d_count;
    DevBuf<HdlcRec> d_out;
    DevBuf<int32_t> d_first, d_copies, d_omarks;
};

extern "C" int aisx_dedup_batch_destroy(aisx_dedup_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    (void)hipDeviceSynchronize(); // (work may still be queued on the caller's streams)
    delete h;
    return AISX_OK;
}

extern "C" int aisx_dedup_batch_create(aisx_dedup_batch** out, int window, int max_pdus, int length_max)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = DdPlan::check(window, max_pdus, length_max)) {
        set_err("aisx_dedup_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_dedup_batch, aisx_dedup_batch_destroy> h(new aisx_dedup_batch(DdPlan(window, max_pdus, length_max)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const DdPlan& pl = h->pl;
    if ((rc = h->d_ckey.alloc(pl.ckey)) != AISX_OK || (rc = h->d_ring.alloc(pl.ring)) != AISX_OK ||
        (rc = h->d_cfirst.alloc(pl.cfirst)) != AISX_OK || (rc = h->d_ccount.alloc(pl.ccount)) != AISX_OK ||
        (rc = h->d_cval.alloc(pl.cval)) != AISX_OK || (rc = h->d_rslot.alloc(pl.rslot)) != AISX_OK ||
        (rc = h->d_bsum.alloc(pl.bsum)) != AISX_OK || (rc = h->d_count.alloc(pl.count)) != AISX_OK ||
        (rc = h->d_out.alloc(pl.out)) != AISX_OK || (rc = h->d_first.alloc(pl.first)) != AISX_OK ||
        (rc = h->d_copies.alloc(pl.copies)) != AISX_OK || (rc = h->d_omarks.alloc(pl.omarks)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipDeviceSynchronize()); // (the counts were zeroed on the null stream, which the caller's streams do not follow)
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_dedup_batch_reset(aisx_dedup_batch* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipDeviceSynchronize());
    AISX_HIPCHK(hipMemset(h->d_count, 0, sizeof(int) * DD_COUNT_WORDS));
    AISX_HIPCHK(hipDeviceSynchronize());
    h->pl.reset(); // (no set of the ring counts as filled: each is cleared by the call that fills it)
    return AISX_OK;
}

extern "C" int aisx_dedup_batch_process(aisx_dedup_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes, const int* d_npdus,
                                        const int* d_nfound, const int32_t* d_marks, int32_t stamp, void* stream)
{
    if (!h || !d_pdus || !d_bytes || !d_npdus) {
        set_err("aisx_dedup_batch_process: a handle, records, their bytes and a record count are needed");
        return AISX_ERR_INVALID;
    }
    if (!h->pl.stamp_ok(stamp)) {
        set_err("aisx_dedup_batch_process: stamp %d is not above the previous call's (%lld): nothing was queued", (int)stamp, h->pl.prev);
        return AISX_ERR_OUT_OF_RANGE;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const DdBufs b = { h->d_ckey, h->d_cfirst, h->d_ccount, h->d_cval, h->d_ring, h->d_rslot, h->d_bsum,
                       h->d_out,  h->d_first,  h->d_copies, h->d_omarks, h->d_count };
    h->d_bytes = d_bytes;
    h->pl.process(b, (const HdlcRec*)d_pdus, d_bytes, d_npdus, d_nfound, d_marks, stamp, [&](const PlanLaunch& l, const DdParams& p) {
        static void (*const kernels[DD_NKERNELS])(DdParams) = { k_dd_clear, k_dd_find, k_dd_classify, k_dd_assign, k_dd_fill };
        hipLaunchKernelGGL(kernels[l.kernel], dim3(l.gx), dim3(l.threads), 0, st, p);
        return true;
    });
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

extern "C" int aisx_dedup_batch_results_device(const aisx_dedup_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                               const int** d_count, const int32_t** d_first, const int32_t** d_copies,
                                               const int32_t** d_marks)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_pdus)
        *d_pdus = (const aisx_pdu*)h->d_out.get();
    if (d_bytes)
        *d_bytes = h->d_bytes;
    if (d_count)
        *d_count = h->d_count;
    if (d_first)
        *d_first = h->d_first;
    if (d_copies)
        *d_copies = h->d_copies;
    if (d_marks)
        *d_marks = h->d_omarks;
    return AISX_OK;
}

extern "C" int aisx_dedup_batch_read(aisx_dedup_batch* h, aisx_pdu* pdus, int32_t* copies, int32_t* marks, int pdu_cap,
                                     int32_t* first, int first_cap, int* counts, int* nfound, void* stream)
{
    if (!h || !counts || pdu_cap < 0 || first_cap < 0 || (first_cap > 0 && !first))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[DD_COUNT_WORDS];
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    const int kept = std::max(0, std::min(cnt[DC_WRITTEN], h->pl.max_pdus)), in = std::max(0, std::min(cnt[DC_CNT + DN_IN], h->pl.max_pdus));
    const int k = std::min(kept, pdu_cap), f = std::min(in, first_cap);
    if (k > 0 && pdus)
        AISX_HIPCHK(hipMemcpyAsync(pdus, h->d_out, sizeof(aisx_pdu) * (size_t)k, hipMemcpyDeviceToHost, st));
    if (k > 0 && copies)
        AISX_HIPCHK(hipMemcpyAsync(copies, h->d_copies, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, st));
    if (k > 0 && marks)
        AISX_HIPCHK(hipMemcpyAsync(marks, h->d_omarks, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, st));
    if (f > 0)
        AISX_HIPCHK(hipMemcpyAsync(first, h->d_first, sizeof(int32_t) * (size_t)f, hipMemcpyDeviceToHost, st));
    if (cnt[DC_BAD])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + DC_BAD, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    memcpy(counts, cnt + DC_CNT, sizeof(int) * DD_NCNT);
    if (nfound)
        *nfound = cnt[DC_FOUND];
    if (cnt[DC_BAD]) {
        set_err("aisx_dedup_batch_read: a call since the last read met a record count outside [0, %d]: it kept nothing", h->pl.max_pdus);
        return AISX_ERR_INVALID;
    }
    if (k < kept || f < in || cnt[DC_FOUND] > kept) {
        set_err("aisx_dedup_batch_read: %d records kept of %d in (the producer found %d more than it handed over); the buffers hold %d and %d",
                kept, in, cnt[DC_FOUND] - kept, pdu_cap, first_cap);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
