// aisx_mlse.hip -- C ABI of the batched sequence detector (include/aisx.h, aisx_mlse_batch_*; body in k_mlse.h): per
// call one kernel, a wave per 64 blocks of every channel, queued on the caller's stream; the per-channel symbol counts
// are read on the device, and the channels' carried symbols alternate between two buffers, so that the workgroups of
// a call all read the state the call began with.
#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_mlse.h"

using namespace aisx;

static_assert(MLSE_LDS_BYTES <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(MLSE_T) void k_mlse(MlseParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[MLSE_LDS_BYTES];
    DevCtx cx{ smem };
    mlse_body<DevCtx, false>(cx, p);
}

__global__ __launch_bounds__(MLSE_T) void k_mlse_flush(MlseParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[MLSE_LDS_BYTES];
    DevCtx cx{ smem };
    mlse_body<DevCtx, true>(cx, p);
}

struct aisx_mlse_batch {
    explicit aisx_mlse_batch(const MlsePlan& plan) : pl(plan) {}
    int dev = 0;
    MlsePlan pl;              // the arguments, the sizes derived from them and the per-call sequence (k_mlse.h)
    DevBuf<MlseState> d_st[2];
    DevBuf<cf> d_carry[2];    // [nchan][MLSE_CARRY]
    DevBuf<int> d_flag;
    Event done;               // behind the last call's work (reset waits for it)
};

extern "C" int aisx_mlse_batch_destroy(aisx_mlse_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_mlse_batch_create(aisx_mlse_batch** out, double bt, int nchan, int max_syms)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    MlseRot rot;
    if (const char* why = MlsePlan::check(nchan, max_syms, mlse_model(bt, nullptr, nullptr, &rot) == AISX_OK)) {
        set_err("aisx_mlse_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_mlse_batch, aisx_mlse_batch_destroy> h(new aisx_mlse_batch(MlsePlan(rot, nchan, max_syms)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    for (int k = 0; k < 2; k++)
        if ((rc = h->d_st[k].alloc(h->pl.st)) != AISX_OK || (rc = h->d_carry[k].alloc(h->pl.carry)) != AISX_OK)
            return rc;
    if ((rc = h->d_flag.alloc(h->pl.flag)) != AISX_OK || (rc = h->done.create(hipEventDisableTiming)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipDeviceSynchronize()); // (the zero fill ran on the null stream)
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_mlse_batch_reset(aisx_mlse_batch* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipEventSynchronize(h->done)); // (the last call's kernel; nothing else on the device)
    for (int k = 0; k < 2; k++)
        AISX_HIPCHK(hipMemsetAsync(h->d_st[k], 0, sizeof(MlseState) * h->pl.st.n, nullptr));
    AISX_HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), nullptr));
    AISX_HIPCHK(hipStreamSynchronize(nullptr)); // (done before the next call, whatever stream that is queued on)
    h->pl.reset();
    return AISX_OK;
}

// a call (d_syms == nullptr: the flush) queued on `st` by the handle's plan
static int mlse_run(aisx_mlse_batch* h, const cf* d_syms, long syms_stride, const int* d_nsyms, uint8_t* d_bits, long bits_stride,
                    int* d_nbits, hipStream_t st)
{
    const MlseBufs b = { { h->d_st[0], h->d_st[1] }, { h->d_carry[0], h->d_carry[1] }, h->d_flag };
    hipError_t err = hipSuccess;
    h->pl.process(b, d_syms, syms_stride, d_nsyms, d_bits, bits_stride, d_nbits, [&](const PlanLaunch& l, const MlseParams& p) {
        if (l.kernel == MLSE_K_PROCESS)
            hipLaunchKernelGGL(k_mlse, dim3(l.gx, l.gy), dim3(l.threads), 0, st, p);
        else
            hipLaunchKernelGGL(k_mlse_flush, dim3(l.gx, l.gy), dim3(l.threads), 0, st, p);
        return (err = hipGetLastError()) == hipSuccess;
    });
    AISX_LAUNCHCHK(err);
    AISX_HIPCHK(hipEventRecord(h->done, st));
    return AISX_OK;
}

extern "C" int aisx_mlse_batch_process(aisx_mlse_batch* h, const aisx_cf32* d_syms, long syms_stride, const int* d_nsyms,
                                       uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream)
{
    if (!h || !d_syms || !d_nsyms || !d_bits || !d_nbits || syms_stride < h->pl.max_syms || bits_stride < (long)h->pl.max_syms + MLSE_EXTRA ||
        ((size_t)d_syms & 7)) {
        set_err("aisx_mlse_batch_process: symbols (8-byte aligned) with a row stride of at least max_syms (%d), counts, and bits with a "
                "row stride of at least max_syms + %d are needed", h ? h->pl.max_syms : 0, MLSE_EXTRA);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    return mlse_run(h, (const cf*)d_syms, syms_stride, d_nsyms, d_bits, bits_stride, d_nbits, (hipStream_t)stream);
}

extern "C" int aisx_mlse_batch_flush(aisx_mlse_batch* h, uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream)
{
    if (!h || !d_bits || !d_nbits || bits_stride < MLSE_EXTRA) {
        set_err("aisx_mlse_batch_flush: a handle, bits with a row stride of at least %d and counts are needed", MLSE_EXTRA);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    return mlse_run(h, nullptr, 0, nullptr, d_bits, bits_stride, d_nbits, (hipStream_t)stream);
}

extern "C" int aisx_mlse_batch_status_device(const aisx_mlse_batch* h, const int** d_status)
{
    if (!h || !d_status)
        return AISX_ERR_INVALID;
    *d_status = h->d_flag;
    return AISX_OK;
}

extern "C" int aisx_mlse_batch_status(aisx_mlse_batch* h, int* status, void* stream)
{
    if (!h || !status)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int f = 0;
    AISX_HIPCHK(hipMemcpyAsync(&f, h->d_flag, sizeof f, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    if (f)
        AISX_HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), st));
    *status = f;
    return AISX_OK;
}
