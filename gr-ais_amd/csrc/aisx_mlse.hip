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
    int dev = 0;
    int nchan = 0, max_syms = 0, groups = 0;
    int cur = 0;              // which state / carry buffer the calls queued so far leave the channels in
    MlseRot rot = {};
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
    if (nchan < 1 || nchan > (1 << 20) || max_syms < 1 || max_syms > (1 << 27) || mlse_model(bt, nullptr, nullptr, &rot) != AISX_OK) {
        set_err("aisx_mlse_batch_create: need 0.1 <= bt <= 1, 1 <= nchan <= 2^20 and 1 <= max_syms <= 2^27");
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_mlse_batch, aisx_mlse_batch_destroy> h(new aisx_mlse_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->nchan = nchan;
    h->max_syms = max_syms;
    h->rot = rot;
    // a call decides at most (max_syms + MLSE_B - 1) / MLSE_B blocks of a channel
    const int blocks = (max_syms + MLSE_B - 1) / MLSE_B;
    h->groups = std::max(1, (blocks + MLSE_T - 1) / MLSE_T);
    for (int k = 0; k < 2; k++)
        if ((rc = h->d_st[k].alloc((size_t)nchan)) != AISX_OK || (rc = h->d_carry[k].alloc((size_t)nchan * MLSE_CARRY)) != AISX_OK)
            return rc;
    if ((rc = h->d_flag.alloc(1)) != AISX_OK || (rc = h->done.create(hipEventDisableTiming)) != AISX_OK)
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
        AISX_HIPCHK(hipMemsetAsync(h->d_st[k], 0, sizeof(MlseState) * h->nchan, nullptr));
    AISX_HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), nullptr));
    AISX_HIPCHK(hipStreamSynchronize(nullptr)); // (done before the next call, whatever stream that is queued on)
    h->cur = 0;
    return AISX_OK;
}

static MlseParams mlse_params(aisx_mlse_batch* h, uint8_t* d_bits, long bits_stride, int* d_nbits)
{
    MlseParams p = {};
    p.max_syms = h->max_syms;
    p.bits = d_bits;
    p.bit_stride = bits_stride;
    p.nbits = d_nbits;
    p.st_in = h->d_st[h->cur];
    p.st_out = h->d_st[h->cur ^ 1];
    p.carry_in = h->d_carry[h->cur];
    p.carry_out = h->d_carry[h->cur ^ 1];
    p.flag = h->d_flag;
    p.rot = h->rot;
    return p;
}

extern "C" int aisx_mlse_batch_process(aisx_mlse_batch* h, const aisx_cf32* d_syms, long syms_stride, const int* d_nsyms,
                                       uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream)
{
    if (!h || !d_syms || !d_nsyms || !d_bits || !d_nbits || syms_stride < h->max_syms || bits_stride < (long)h->max_syms + MLSE_EXTRA ||
        ((size_t)d_syms & 7)) {
        set_err("aisx_mlse_batch_process: symbols (8-byte aligned) with a row stride of at least max_syms (%d), counts, and bits with a "
                "row stride of at least max_syms + %d are needed", h ? h->max_syms : 0, MLSE_EXTRA);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    MlseParams p = mlse_params(h, d_bits, bits_stride, d_nbits);
    p.syms = (const cf*)d_syms;
    p.sym_stride = syms_stride;
    p.nsyms = d_nsyms;
    hipLaunchKernelGGL(k_mlse, dim3(h->nchan, h->groups), dim3(MLSE_T), 0, st, p);
    AISX_HIPCHK(hipGetLastError());
    AISX_HIPCHK(hipEventRecord(h->done, st));
    h->cur ^= 1;
    return AISX_OK;
}

extern "C" int aisx_mlse_batch_flush(aisx_mlse_batch* h, uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream)
{
    if (!h || !d_bits || !d_nbits || bits_stride < MLSE_EXTRA) {
        set_err("aisx_mlse_batch_flush: a handle, bits with a row stride of at least %d and counts are needed", MLSE_EXTRA);
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const MlseParams p = mlse_params(h, d_bits, bits_stride, d_nbits);
    hipLaunchKernelGGL(k_mlse_flush, dim3(h->nchan, 1), dim3(MLSE_T), 0, st, p); // (at most two blocks of a channel are left)
    AISX_HIPCHK(hipGetLastError());
    AISX_HIPCHK(hipEventRecord(h->done, st));
    h->cur ^= 1;
    return AISX_OK;
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
