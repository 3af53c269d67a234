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
    int dev = 0;
    int nchan = 0, max_pdus = 0, lmax = 0, groups = 0;
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
    if (nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > MSG_MAX_OCTETS) {
        set_err("aisx_msg_batch_create: need nchan >= 1, max_pdus >= 1, 2 <= length_max <= %d", MSG_MAX_OCTETS);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_msg_batch, aisx_msg_batch_destroy> h(new aisx_msg_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->nchan = nchan;
    h->max_pdus = max_pdus;
    h->lmax = length_max;
    const long long groups = ((long long)max_pdus + MSG_T - 1) / MSG_T;
    h->groups = (int)(groups < MSG_MAX_GROUPS ? groups : MSG_MAX_GROUPS);
    if ((rc = h->d_tab.alloc((size_t)MSG_TAB_WORDS, false)) != AISX_OK || (rc = h->d_cols.alloc((size_t)MSG_NCOL * max_pdus, false)) != AISX_OK ||
        (rc = h->d_strs.alloc((size_t)MSG_STR_WORDS * max_pdus, false)) != AISX_OK || (rc = h->d_count.alloc(4)) != AISX_OK)
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
    MsgParams p;
    p.in = (const HdlcRec*)d_pdus;
    p.bytes = d_bytes;
    p.npdus = d_npdus;
    p.nfound = d_nfound;
    p.tab = h->d_tab;
    p.nchan = h->nchan;
    p.max_pdus = h->max_pdus;
    p.max_len = h->lmax - 1;
    p.nwaves = h->groups * (MSG_T / 64);
    p.cols = h->d_cols;
    p.strs = h->d_strs;
    p.count = h->d_count;
    hipLaunchKernelGGL(k_msg, dim3(h->groups), dim3(MSG_T), 0, (hipStream_t)stream, p);
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
        *col_stride = h->max_pdus;
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
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_cols, sizeof(int32_t) * (size_t)h->max_pdus,
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
                "[0, %d) or a payload longer than %d octets: those rows hold no fields", h->max_pdus, h->nchan, h->lmax - 1);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[0]) {
        set_err("aisx_msg_batch_read: %d PDUs found, %d rows read", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
