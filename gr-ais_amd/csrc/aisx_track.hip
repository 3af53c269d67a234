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
    int dev = 0;
    int capacity = 0, max_rows = 0, hbits = 0, bbits = 0, row_groups = 0, cap_groups = 0, clear_groups = 0;
    int cur = 0;                 // which table buffer the calls queued so far leave the table in
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

static TrkParams trk_params(const aisx_track_batch* h)
{
    TrkParams p = {};
    p.capacity = h->capacity;
    p.max_rows = h->max_rows;
    p.tab = h->d_tab[h->cur];
    p.strs = h->d_strs[h->cur];
    p.hkey = h->d_hkey;
    p.hval = h->d_hval;
    p.hbits = h->hbits;
    p.bkey = h->d_bkey;
    p.bfirst = h->d_bfirst;
    p.bval = h->d_bval;
    p.bj = h->d_bj;
    p.bbits = h->bbits;
    p.rslot = h->d_rslot;
    p.bsum = h->d_bsum;
    p.nbmax = std::max(h->row_groups, h->cap_groups);
    p.win = h->d_win;
    p.changed = h->d_changed;
    p.count = h->d_count;
    return p;
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
    AISX_HIPCHK(hipMemsetD32(h->d_hkey, TRK_EMPTY, (size_t)1 << h->hbits));
    AISX_HIPCHK(hipMemset(h->d_count, 0, sizeof(int) * TRK_COUNT_WORDS));
    AISX_HIPCHK(hipDeviceSynchronize());
    h->cur = 0;
    return AISX_OK;
}

extern "C" int aisx_track_batch_create(aisx_track_batch** out, int capacity, int max_rows)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (capacity < 1 || capacity > TRK_MAX || max_rows < 1 || max_rows > TRK_MAX) {
        set_err("aisx_track_batch_create: need 1 <= capacity <= %d and 1 <= max_rows <= %d", TRK_MAX, TRK_MAX);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_track_batch, aisx_track_batch_destroy> h(new aisx_track_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->capacity = capacity;
    h->max_rows = max_rows;
    h->hbits = trk_hash_bits(capacity);
    h->bbits = trk_hash_bits(max_rows);
    h->row_groups = (max_rows + TRK_T - 1) / TRK_T;
    h->cap_groups = (capacity + TRK_T - 1) / TRK_T;
    h->clear_groups = std::min(h->row_groups, 1024);
    const size_t H = (size_t)1 << h->hbits, B = (size_t)1 << h->bbits, R = (size_t)max_rows, C = (size_t)capacity;
    for (int k = 0; k < 2; k++)
        if ((rc = h->d_tab[k].alloc(TRK_NCOL * C, false)) != AISX_OK || (rc = h->d_strs[k].alloc(MSG_STR_WORDS * C, false)) != AISX_OK)
            return rc;
    if ((rc = h->d_hkey.alloc(H, false)) != AISX_OK || (rc = h->d_hval.alloc(H, false)) != AISX_OK ||
        (rc = h->d_bkey.alloc(B, false)) != AISX_OK || (rc = h->d_bfirst.alloc(B, false)) != AISX_OK ||
        (rc = h->d_bval.alloc(B, false)) != AISX_OK || (rc = h->d_bj.alloc(B, false)) != AISX_OK ||
        (rc = h->d_rslot.alloc(R, false)) != AISX_OK ||
        (rc = h->d_bsum.alloc(2 * (size_t)std::max(h->row_groups, h->cap_groups), false)) != AISX_OK ||
        (rc = h->d_win.alloc(TRK_NWIN * R, false)) != AISX_OK || (rc = h->d_changed.alloc(R, false)) != AISX_OK ||
        (rc = h->d_gcols.alloc(TRK_NCOL * R, false)) != AISX_OK || (rc = h->d_gstrs.alloc(MSG_STR_WORDS * R, false)) != AISX_OK ||
        (rc = h->d_count.alloc(TRK_COUNT_WORDS)) != AISX_OK || (rc = trk_empty(h.get())) != AISX_OK)
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
    if (!h || !d_cols || !d_strs || !d_nrows || col_stride < h->max_rows || ((size_t)d_strs & 3)) {
        set_err("aisx_track_batch_process: a handle, columns of a stride of at least max_rows, strings aligned to four bytes and "
                "a row count are needed");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    TrkParams p = trk_params(h);
    p.in_cols = d_cols;
    p.in_stride = col_stride;
    p.in_strs = (const uint32_t*)d_strs;
    p.in_recs = (const HdlcRec*)d_pdus;
    p.nrows = d_nrows;
    p.stamp = stamp;
    p.grid = h->clear_groups;
    hipLaunchKernelGGL(k_trk_clear, dim3(h->clear_groups), dim3(TRK_T), 0, st, p);
    p.grid = h->row_groups;
    hipLaunchKernelGGL(k_trk_find, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
    hipLaunchKernelGGL(k_trk_classify, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
    hipLaunchKernelGGL(k_trk_assign, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
    hipLaunchKernelGGL(k_trk_winner, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
    hipLaunchKernelGGL(k_trk_apply, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
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
    TrkParams p = trk_params(h);
    p.tab2 = h->d_tab[h->cur ^ 1];
    p.strs2 = h->d_strs[h->cur ^ 1];
    p.grid = h->cap_groups;
    hipLaunchKernelGGL(k_trk_keep, dim3(h->cap_groups), dim3(TRK_T), 0, st, p, min_stamp);
    hipLaunchKernelGGL(k_trk_compact, dim3(h->cap_groups), dim3(TRK_T), 0, st, p, min_stamp);
    AISX_HIPCHK(hipGetLastError());
    h->cur ^= 1;
    return AISX_OK;
}

extern "C" int aisx_track_batch_results_device(const aisx_track_batch* h, const int32_t** d_cols, long* col_stride,
                                               const char** d_strs, const int** d_changed, const int** d_count)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_cols)
        *d_cols = h->d_tab[h->cur];
    if (col_stride)
        *col_stride = h->capacity;
    if (d_strs)
        *d_strs = (const char*)h->d_strs[h->cur].get();
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
    set_err("%s: a call since the last read met a row count outside [0, %d]: it merged nothing", who, h->max_rows);
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
    const int nv = std::max(0, std::min(cnt[TN_VESSELS], h->capacity));
    const int k = std::max(0, std::min(n, nv - first));
    if (k > 0) {
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_tab[h->cur] + first,
                                     sizeof(int32_t) * (size_t)h->capacity, sizeof(int32_t) * (size_t)k, TRK_NCOL, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(strs, h->d_strs[h->cur] + (size_t)first * MSG_STR_WORDS, (size_t)MSG_STR * k, hipMemcpyDeviceToHost, st));
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
    TrkParams p = trk_params(h);
    p.tab2 = h->d_gcols;
    p.strs2 = h->d_gstrs;
    p.grid = h->row_groups;
    hipLaunchKernelGGL(k_trk_gather, dim3(h->row_groups), dim3(TRK_T), 0, st, p);
    AISX_HIPCHK(hipGetLastError());
    int cnt[TRK_NCNT], rc;
    if ((rc = trk_counts(h, cnt, true, st)) != AISX_OK)
        return rc;
    const int k = std::max(0, std::min(cnt[TN_CHANGED], h->max_rows));
    *nchanged = k;
    if (k > cap) {
        set_err("aisx_track_batch_read_changed: %d vessels changed, the buffers hold %d", k, cap);
        return AISX_ERR_OVERFLOW;
    }
    if (k > 0) {
        AISX_HIPCHK(hipMemcpyAsync(idx, h->d_changed, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpy2DAsync(cols, sizeof(int32_t) * (size_t)col_stride, h->d_gcols, sizeof(int32_t) * (size_t)h->max_rows,
                                     sizeof(int32_t) * (size_t)k, TRK_NCOL, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(strs, h->d_gstrs, (size_t)MSG_STR * k, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipStreamSynchronize(st));
    }
    return cnt[TN_BAD] ? trk_bad(h, "aisx_track_batch_read_changed") : AISX_OK;
}
