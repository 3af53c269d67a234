// aisx_msg_enc.hip -- C ABI of the batched message-field encoder (include/aisx.h, aisx_msg_enc_batch_*): one memset of
// two counters and one kernel per call, one lane per record (k_msg_enc.h: msg_enc_body).  Everything is queued on the
// caller's stream; the row count is read on the device.
#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_msg_enc.h"

using namespace aisx;

namespace aisx {
extern const MsgEncTab MSG_ENC_TAB; // aisx_msg_enc.cpp
}

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(MENC_NCNT == 5, "the counts include/aisx.h describes");

__global__ __launch_bounds__(MENC_T) void k_msg_enc(MsgEncParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[menc_lds_bytes(MENC_T)];
    DevCtx cx{ smem };
    msg_enc_body(cx, p);
}

struct aisx_msg_enc_batch {
    explicit aisx_msg_enc_batch(const MsgEncPlan& plan) : pl(plan) {}
    int dev = 0;
    const MsgEncPlan pl;       // the arguments, the sizes derived from them and the per-call sequence (k_msg_enc.h)
    DevBuf<uint32_t> d_tab;    // [MSG_ENC_TAB_WORDS]
    DevBuf<HdlcRec> d_pdus;    // [max_rows]
    DevBuf<uint32_t> d_bytes;  // [max_rows][MSG_ENC_WORDS]
    DevBuf<int32_t> d_status;  // [max_rows]
    DevBuf<int> d_count;       // [MENC_NCNT]
};

extern "C" int aisx_msg_enc_batch_destroy(aisx_msg_enc_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_msg_enc_batch_create(aisx_msg_enc_batch** out, int nchan, int max_rows, int table_rows)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = MsgEncPlan::check(nchan, max_rows, table_rows)) {
        set_err("aisx_msg_enc_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_msg_enc_batch, aisx_msg_enc_batch_destroy> h(new aisx_msg_enc_batch(MsgEncPlan(nchan, max_rows, table_rows)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    if ((rc = h->d_tab.alloc(h->pl.tab)) != AISX_OK || (rc = h->d_pdus.alloc(h->pl.pdus)) != AISX_OK ||
        (rc = h->d_bytes.alloc(h->pl.bytes)) != AISX_OK || (rc = h->d_status.alloc(h->pl.status)) != AISX_OK ||
        (rc = h->d_count.alloc(h->pl.count)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_tab, &MSG_ENC_TAB, sizeof(MsgEncTab), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_msg_enc_batch_create: copying the field table failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_msg_enc_batch_process(aisx_msg_enc_batch* h, const int32_t* d_cols, long col_stride, const char* d_strs,
                                          const int32_t* d_idx, const int* d_nrows, const int32_t* d_chan, int as_type, int as_part,
                                          void* stream)
{
    if (!h || !d_cols || !d_nrows) {
        set_err("aisx_msg_enc_batch_process: a handle, columns and a row count are needed");
        return AISX_ERR_INVALID;
    }
    if (const char* why = h->pl.check_call(col_stride, d_strs)) {
        set_err("aisx_msg_enc_batch_process: %s", why);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const MsgEncBufs b = { h->d_tab, h->d_pdus, h->d_bytes, h->d_status, h->d_count };
    hipError_t e = hipSuccess;
    h->pl.process(
        b, d_cols, col_stride, (const uint32_t*)d_strs, d_idx, d_nrows, d_chan, as_type, as_part,
        [&](int* first, int n) {
            e = hipMemsetAsync(first, 0, sizeof(int) * (size_t)n, st);
            return e == hipSuccess;
        },
        [&](const PlanLaunch& l, const MsgEncParams& p) {
            hipLaunchKernelGGL(k_msg_enc, dim3(l.gx), dim3(l.threads), 0, st, p);
            return true;
        });
    AISX_HIPCHK(e);
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

extern "C" int aisx_msg_enc_batch_results_device(const aisx_msg_enc_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                                 const int** d_count, const int32_t** d_status)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_pdus)
        *d_pdus = (const aisx_pdu*)h->d_pdus.get();
    if (d_bytes)
        *d_bytes = (const uint8_t*)h->d_bytes.get();
    if (d_count)
        *d_count = h->d_count;
    if (d_status)
        *d_status = h->d_status;
    return AISX_OK;
}

extern "C" int aisx_msg_enc_batch_read(aisx_msg_enc_batch* h, aisx_pdu* pdus, int32_t* status, int cap, uint8_t* bytes,
                                       long bytes_cap, int* nrecs, int* counts, void* stream)
{
    if (!h || !nrecs || cap < 0 || bytes_cap < 0 || (cap > 0 && (!pdus || !status)) || (bytes_cap > 0 && !bytes))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[MENC_NCNT] = {};
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    const long fit = bytes_cap / MSG_ENC_OCTETS;
    int k = cnt[1] < cap ? cnt[1] : cap;
    if (k > fit)
        k = (int)fit;
    if (k > 0) {
        AISX_HIPCHK(hipMemcpyAsync(pdus, h->d_pdus, sizeof(HdlcRec) * (size_t)k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(status, h->d_status, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(bytes, h->d_bytes, (size_t)MSG_ENC_OCTETS * k, hipMemcpyDeviceToHost, st));
    }
    if (cnt[2])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + 2, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *nrecs = k;
    if (counts)
        for (int j = 0; j < MENC_NCNT; j++)
            counts[j] = cnt[j];
    if (cnt[2]) {
        set_err("aisx_msg_enc_batch_read: a call since the last read met a row count outside [0, %d]: it made no records",
                h->pl.max_rows);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[1]) {
        set_err("aisx_msg_enc_batch_read: %d records made, %d read", cnt[1], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
