// aisx_msg.hip -- C ABI of the batched message-field decoder (include/aisx.h, aisx_msg_batch_*): one kernel per call,
// one lane per record (k_msg.h: msg_body).  Everything is queued on the caller's stream; the record count is read on
// the device.
#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_msg.h"

using namespace aisx;

namespace aisx {
extern const MsgTab MSG_TAB; // aisx_msg.cpp
}

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(sizeof(MsgTab) == sizeof(uint32_t) * MSG_TAB_WORDS, "table layout");

__global__ __launch_bounds__(MSG_T) void k_msg(MsgParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[msg_lds_bytes(MSG_T)];
    DevCtx cx{ smem };
    msg_body(cx, p);
}

struct aisx_msg_batch {
    explicit aisx_msg_batch(const MsgPlan& plan) : pl(plan) {}
    int dev = 0;
    const MsgPlan pl;        // the arguments, the sizes derived from them and the per-call sequence (k_msg.h)
    DevBuf<uint32_t> d_tab;  // [MSG_TAB_WORDS]
    DevBuf<int32_t> d_cols;  // [MSG_NCOL][max_pdus]
    DevBuf<uint32_t> d_strs; // [max_pdus][MSG_STR_WORDS]
    DevBuf<int> d_count;     // [0] found, [1] rows written, [2] bad-input flag
};

extern "C" int aisx_msg_batch_destroy(aisx_msg_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_msg_batch_create(aisx_msg_batch** out, int nchan, int max_pdus, int length_max)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = MsgPlan::check(nchan, max_pdus, length_max)) {
        set_err("aisx_msg_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_msg_batch, aisx_msg_batch_destroy> h(new aisx_msg_batch(MsgPlan(nchan, max_pdus, length_max)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    if ((rc = h->d_tab.alloc(h->pl.tab)) != AISX_OK || (rc = h->d_cols.alloc(h->pl.cols)) != AISX_OK ||
        (rc = h->d_strs.alloc(h->pl.strs)) != AISX_OK || (rc = h->d_count.alloc(h->pl.count)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_tab, &MSG_TAB, sizeof(MsgTab), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_msg_batch_create: copying the field table failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_msg_batch_process(aisx_msg_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes, const int* d_npdus,
                                      const int* d_nfound, void* stream)
{
    if (!h || !d_pdus || !d_bytes || !d_npdus) {
        set_err("aisx_msg_batch_process: a handle, records, bytes and a record count are needed");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const MsgBufs b = { h->d_tab, h->d_cols, h->d_strs, h->d_count };
    h->pl.process(b, (const HdlcRec*)d_pdus, d_bytes, d_npdus, d_nfound, [&](const PlanLaunch& l, const MsgParams& p) {
        hipLaunchKernelGGL(k_msg, dim3(l.gx), dim3(l.threads), 0, (hipStream_t)stream, p);
        return true;
    });
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

extern "C" int aisx_msg_batch_results_device(const aisx_msg_batch* h, const int32_t** d_cols, long* col_stride,
                                             const char** d_strs, const int** d_count)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_cols)
        *d_cols = h->d_cols;
    if (col_stride)
        *col_stride = h->pl.max_pdus;
    if (d_strs)
        *d_strs = (const char*)h->d_strs.get();
    if (d_count)
        *d_count = h->d_count;
    return AISX_OK;
}

extern "C" int aisx_msg_batch_read(aisx_msg_batch* h, int32_t* cols, long col_stride, char* strs, int cap, int* nrecs,
                                   int* nfound, void* stream)
{
    if (!h || !nrecs || cap < 0 || col_stride < cap || (cap > 0 && (!cols || !strs)))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[3] = { 0, 0, 0 };
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    const int k = cnt[1] < cap ? cnt[1] : cap;
    if (k > 0) {
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_cols, sizeof(int32_t) * (size_t)h->pl.max_pdus,
                                     sizeof(int32_t) * (size_t)k, MSG_NCOL, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(strs, h->d_strs, (size_t)MSG_STR * k, hipMemcpyDeviceToHost, st));
    }
    if (cnt[2])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + 2, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *nrecs = k;
    if (nfound)
        *nfound = cnt[0];
    if (cnt[2]) {
        set_err("aisx_msg_batch_read: a call since the last read met a record count outside [0, %d], a channel outside "
                "[0, %d) or a payload longer than %d octets: those rows hold no fields", h->pl.max_pdus, h->pl.nchan, h->pl.lmax - 1);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[0]) {
        set_err("aisx_msg_batch_read: %d PDUs found, %d rows read", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
