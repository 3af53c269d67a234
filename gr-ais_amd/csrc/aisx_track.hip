// aisx_track.hip -- C ABI of the vessel table in device memory (include/aisx.h, aisx_track_batch_*; bodies in
// k_track.h): six small kernels per update, two per expire, one per gather, all queued on the caller's stream; the row
// count is read on the device.
#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_track.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");

#define TRK_KERNEL(name, body)                                               \
    __global__ __launch_bounds__(TRK_T) void name(TrkParams p)               \
    {                                                                        \
        __shared__ __attribute__((aligned(16))) char smem[TRK_LDS_BYTES];    \
        DevCtx cx{ smem };                                                   \
        body(cx, p);                                                         \
    }
TRK_KERNEL(k_trk_clear, trk_clear_body)
TRK_KERNEL(k_trk_find, trk_find_body)
TRK_KERNEL(k_trk_classify, trk_classify_body)
TRK_KERNEL(k_trk_assign, trk_assign_body)
TRK_KERNEL(k_trk_winner, trk_winner_body)
TRK_KERNEL(k_trk_apply, trk_apply_body)
TRK_KERNEL(k_trk_gather, trk_gather_body)

__global__ __launch_bounds__(TRK_T) void k_trk_keep(TrkParams p, int32_t min_stamp)
{
    __shared__ __attribute__((aligned(16))) char smem[TRK_LDS_BYTES];
    DevCtx cx{ smem };
    trk_keep_body(cx, p, min_stamp);
}

__global__ __launch_bounds__(TRK_T) void k_trk_compact(TrkParams p, int32_t min_stamp)
{
    __shared__ __attribute__((aligned(16))) char smem[TRK_LDS_BYTES];
    DevCtx cx{ smem };
    trk_compact_body(cx, p, min_stamp);
}

struct aisx_track_batch {
    explicit aisx_track_batch(const TrkPlan& plan) : pl(plan) {}
    int dev = 0;
    TrkPlan pl;                  // the arguments, the sizes derived from them and the per-call sequences (k_track.h)
    DevBuf<int32_t> d_tab[2];    // [TRK_NCOL][capacity]
    DevBuf<uint32_t> d_strs[2];  // [capacity][MSG_STR_WORDS]
    DevBuf<int32_t> d_hkey;      // [1 << hbits]
    DevBuf<int> d_hval;
    DevBuf<int32_t> d_bkey;      // [1 << bbits]
    DevBuf<int> d_bfirst, d_bval, d_bj;
    DevBuf<int> d_rslot;         // [max_rows]
    DevBuf<int> d_bsum;          // [2][max(row_groups, cap_groups)]
    DevBuf<int> d_win;           // [TRK_NWIN][max_rows]
    DevBuf<int> d_changed;       // [max_rows]
    DevBuf<int32_t> d_gcols;     // [TRK_NCOL][max_rows]   the changed vessels' rows, gathered
    DevBuf<uint32_t> d_gstrs;    // [max_rows][MSG_STR_WORDS]
    DevBuf<int> d_count;         // [TRK_COUNT_WORDS]
};

static TrkBufs trk_bufs(const aisx_track_batch* h)
{
    return TrkBufs{ { h->d_tab[0], h->d_tab[1] }, { h->d_strs[0], h->d_strs[1] }, h->d_hkey, h->d_hval, h->d_bkey, h->d_bfirst,
                    h->d_bval, h->d_bj, h->d_rslot, h->d_bsum, h->d_win, h->d_changed, h->d_gcols, h->d_gstrs, h->d_count };
}

// a launch of the plan's on `st`: the kernel of its id
static bool trk_launch(const PlanLaunch& l, const TrkCall& c, hipStream_t st)
{
    const dim3 grid(l.gx), threads(l.threads);
    switch (l.kernel) {
    case TRK_K_CLEAR: hipLaunchKernelGGL(k_trk_clear, grid, threads, 0, st, c.p); break;
    case TRK_K_FIND: hipLaunchKernelGGL(k_trk_find, grid, threads, 0, st, c.p); break;
    case TRK_K_CLASSIFY: hipLaunchKernelGGL(k_trk_classify, grid, threads, 0, st, c.p); break;
    case TRK_K_ASSIGN: hipLaunchKernelGGL(k_trk_assign, grid, threads, 0, st, c.p); break;
    case TRK_K_WINNER: hipLaunchKernelGGL(k_trk_winner, grid, threads, 0, st, c.p); break;
    case TRK_K_APPLY: hipLaunchKernelGGL(k_trk_apply, grid, threads, 0, st, c.p); break;
    case TRK_K_KEEP: hipLaunchKernelGGL(k_trk_keep, grid, threads, 0, st, c.p, c.min_stamp); break;
    case TRK_K_COMPACT: hipLaunchKernelGGL(k_trk_compact, grid, threads, 0, st, c.p, c.min_stamp); break;
    case TRK_K_GATHER: hipLaunchKernelGGL(k_trk_gather, grid, threads, 0, st, c.p); break;
    }
    return true;
}

extern "C" int aisx_track_batch_destroy(aisx_track_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

// an empty table: the hash free, no vessels, no counts (on the null stream, behind everything)
static int trk_empty(aisx_track_batch* h)
{
    AISX_HIPCHK(hipDeviceSynchronize());
    AISX_HIPCHK(hipMemsetD32(h->d_hkey, TRK_EMPTY, h->pl.hkey.n));
    AISX_HIPCHK(hipMemset(h->d_count, 0, sizeof(int) * TRK_COUNT_WORDS));
    AISX_HIPCHK(hipDeviceSynchronize());
    h->pl.reset();
    return AISX_OK;
}

extern "C" int aisx_track_batch_create(aisx_track_batch** out, int capacity, int max_rows)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = TrkPlan::check(capacity, max_rows)) {
        set_err("aisx_track_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_track_batch, aisx_track_batch_destroy> h(new aisx_track_batch(TrkPlan(capacity, max_rows)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const TrkPlan& pl = h->pl;
    for (int k = 0; k < 2; k++)
        if ((rc = h->d_tab[k].alloc(pl.tab)) != AISX_OK || (rc = h->d_strs[k].alloc(pl.strs)) != AISX_OK)
            return rc;
    if ((rc = h->d_hkey.alloc(pl.hkey)) != AISX_OK || (rc = h->d_hval.alloc(pl.hval)) != AISX_OK ||
        (rc = h->d_bkey.alloc(pl.bkey)) != AISX_OK || (rc = h->d_bfirst.alloc(pl.bfirst)) != AISX_OK ||
        (rc = h->d_bval.alloc(pl.bval)) != AISX_OK || (rc = h->d_bj.alloc(pl.bj)) != AISX_OK ||
        (rc = h->d_rslot.alloc(pl.rslot)) != AISX_OK || (rc = h->d_bsum.alloc(pl.bsum)) != AISX_OK ||
        (rc = h->d_win.alloc(pl.win)) != AISX_OK || (rc = h->d_changed.alloc(pl.changed)) != AISX_OK ||
        (rc = h->d_gcols.alloc(pl.gcols)) != AISX_OK || (rc = h->d_gstrs.alloc(pl.gstrs)) != AISX_OK ||
        (rc = h->d_count.alloc(pl.count)) != AISX_OK || (rc = trk_empty(h.get())) != AISX_OK)
        return rc;
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_track_batch_reset(aisx_track_batch* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    return trk_empty(h);
}

extern "C" int aisx_track_batch_process(aisx_track_batch* h, const int32_t* d_cols, long col_stride, const char* d_strs,
                                        const aisx_pdu* d_pdus, const int* d_nrows, int32_t stamp, void* stream)
{
    if (!h || !d_cols || !d_strs || !d_nrows || col_stride < h->pl.max_rows || ((size_t)d_strs & 3)) {
        set_err("aisx_track_batch_process: a handle, columns of a stride of at least max_rows, strings aligned to four bytes and "
                "a row count are needed");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    h->pl.process(trk_bufs(h), d_cols, col_stride, (const uint32_t*)d_strs, (const HdlcRec*)d_pdus, d_nrows, stamp,
                  [&](const PlanLaunch& l, const TrkCall& c) { return trk_launch(l, c, st); });
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

extern "C" int aisx_track_batch_expire(aisx_track_batch* h, int32_t min_stamp, void* stream)
{
    if (!h) {
        set_err("aisx_track_batch_expire: need a handle");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    hipError_t err = hipSuccess;
    h->pl.expire(trk_bufs(h), min_stamp, [&](const PlanLaunch& l, const TrkCall& c) {
        return trk_launch(l, c, st) && (l.kernel != TRK_K_COMPACT || (err = hipGetLastError()) == hipSuccess);
    });
    AISX_LAUNCHCHK(err);
    return AISX_OK;
}

extern "C" int aisx_track_batch_results_device(const aisx_track_batch* h, const int32_t** d_cols, long* col_stride,
                                               const char** d_strs, const int** d_changed, const int** d_count)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_cols)
        *d_cols = h->d_tab[h->pl.cur];
    if (col_stride)
        *col_stride = h->pl.capacity;
    if (d_strs)
        *d_strs = (const char*)h->d_strs[h->pl.cur].get();
    if (d_changed)
        *d_changed = h->d_changed;
    if (d_count)
        *d_count = h->d_count;
    return AISX_OK;
}

// the counts on the host; a set bad-input flag is cleared behind the copy when `clear`
static int trk_counts(aisx_track_batch* h, int* cnt, bool clear, hipStream_t st)
{
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof(int) * TRK_NCNT, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    if (clear && cnt[TN_BAD])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + TN_BAD, 0, sizeof(int), st));
    return AISX_OK;
}

static int trk_bad(const aisx_track_batch* h, const char* who)
{
    set_err("%s: a call since the last read met a row count outside [0, %d]: it merged nothing", who, h->pl.max_rows);
    return AISX_ERR_INVALID;
}

extern "C" int aisx_track_batch_counts(aisx_track_batch* h, int* counts, void* stream)
{
    if (!h || !counts)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    return trk_counts(h, counts, false, (hipStream_t)stream);
}

extern "C" int aisx_track_batch_read(aisx_track_batch* h, int first, int n, int32_t* cols, long col_stride, char* strs,
                                     int* nvessels, void* stream)
{
    if (!h || !nvessels || first < 0 || n < 0 || col_stride < n || (n > 0 && (!cols || !strs)))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[TRK_NCNT], rc;
    if ((rc = trk_counts(h, cnt, true, st)) != AISX_OK)
        return rc;
    const int nv = std::max(0, std::min(cnt[TN_VESSELS], h->pl.capacity));
    const int k = std::max(0, std::min(n, nv - first));
    if (k > 0) {
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_tab[h->pl.cur] + first,
                                     sizeof(int32_t) * (size_t)h->pl.capacity, sizeof(int32_t) * (size_t)k, TRK_NCOL, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(strs, h->d_strs[h->pl.cur] + (size_t)first * MSG_STR_WORDS, (size_t)MSG_STR * k, hipMemcpyDeviceToHost, st));
    }
    AISX_HIPCHK(hipStreamSynchronize(st));
    *nvessels = nv;
    return cnt[TN_BAD] ? trk_bad(h, "aisx_track_batch_read") : AISX_OK;
}

extern "C" int aisx_track_batch_read_changed(aisx_track_batch* h, int* idx, int32_t* cols, long col_stride, char* strs, int cap,
                                             int* nchanged, void* stream)
{
    if (!h || !nchanged || cap < 0 || col_stride < cap || (cap > 0 && (!idx || !cols || !strs)))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    h->pl.gather(trk_bufs(h), [&](const PlanLaunch& l, const TrkCall& c) { return trk_launch(l, c, st); });
    AISX_HIPCHK(hipGetLastError());
    int cnt[TRK_NCNT], rc;
    if ((rc = trk_counts(h, cnt, true, st)) != AISX_OK)
        return rc;
    const int k = std::max(0, std::min(cnt[TN_CHANGED], h->pl.max_rows));
    *nchanged = k;
    if (k > cap) {
        set_err("aisx_track_batch_read_changed: %d vessels changed, the buffers hold %d", k, cap);
        return AISX_ERR_OVERFLOW;
    }
    if (k > 0) {
        AISX_HIPCHK(hipMemcpyAsync(idx, h->d_changed, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_gcols, sizeof(int32_t) * (size_t)h->pl.max_rows,
                                     sizeof(int32_t) * (size_t)k, TRK_NCOL, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(strs, h->d_gstrs, (size_t)MSG_STR * k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipStreamSynchronize(st));
    }
    return cnt[TN_BAD] ? trk_bad(h, "aisx_track_batch_read_changed") : AISX_OK;
}
