// aisx_nmea_parse.hip -- C ABI of the batched NMEA parser (include/aisx.h, aisx_nmea_parse_batch_*): per call the twelve
// kernels of k_nmea_parse.h, queued on the caller's stream; the byte count is read on the device, and so is everything
// the handle carries from call to call.
#include <string.h>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_nmea_parse.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(NP_NCNT == AISX_NMEAP_NCNT, "counts layout");
static_assert(AISX_NMEA_PARSE_REF_TAIL == 1, "the flag NmpPlan::check takes");

#define NMP_KERNEL(name, threads, call)                                              \
    __global__ __launch_bounds__(threads) void name(NmpParams p)                    \
    {                                                                                \
        __shared__ __attribute__((aligned(16))) char smem[NP_LDS_BYTES];            \
        DevCtx cx{ smem };                                                           \
        call;                                                                        \
    }
NMP_KERNEL(k_nmp_count, NP_T, nmp_count_body(cx, p))
NMP_KERNEL(k_nmp_scan, NP_SCAN_T, nmp_scan_body(cx, p, NP_T))
NMP_KERNEL(k_nmp_index, NP_T, nmp_index_body(cx, p))
NMP_KERNEL(k_nmp_parse, NP_T, nmp_parse_body(cx, p))
NMP_KERNEL(k_nmp_gcount, NP_T, nmp_gcount_body(cx, p))
NMP_KERNEL(k_nmp_gscan1, NP_SCAN_T, nmp_gscan1_body(cx, p, NP_T))
NMP_KERNEL(k_nmp_gcompact, NP_T, nmp_gcompact_body(cx, p))
NMP_KERNEL(k_nmp_gmsg, NP_T, nmp_gmsg_body(cx, p))
NMP_KERNEL(k_nmp_gscan2, NP_SCAN_T, nmp_gscan2_body(cx, p, NP_T))
NMP_KERNEL(k_nmp_gplace, NP_T, nmp_gplace_body(cx, p))
NMP_KERNEL(k_nmp_write, NP_T, nmp_write_body(cx, p))
NMP_KERNEL(k_nmp_carry, 64, nmp_carry_body(cx, p))

struct aisx_nmea_parse_batch {
    explicit aisx_nmea_parse_batch(NmpPlan&& plan) : pl(std::move(plan)) {}
    int dev = 0;
    const NmpPlan pl; // the arguments, the sizes derived from them and the per-call sequence (k_nmea_parse.h)
    DevBuf<char> d_desig;
    DevBuf<unsigned char> d_dlen, d_lcarry, d_gcarry, d_bytes;
    DevBuf<NmpState> d_st;
    DevBuf<int> d_tcount, d_toff, d_meta, d_cidx, d_aux, d_count, d_mlen, d_tl, d_bstat;
    DevBuf<long long> d_lend, d_pos, d_tm, d_times, d_tlb;
    DevBuf<NmpKey> d_key;
    DevBuf<HdlcRec> d_rec;
    DevBuf<NmpNext> d_next;
};

extern "C" int aisx_nmea_parse_batch_destroy(aisx_nmea_parse_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    (void)hipDeviceSynchronize(); // (work may still be queued on the caller's streams)
    delete h;
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_batch_create(aisx_nmea_parse_batch** out, const char* const* designators, int nchan,
                                            int length_max, int max_line, int flags, long max_bytes, int max_lines,
                                            int max_pdus)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = NmpPlan::check(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus)) {
        set_err("aisx_nmea_parse_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    if (const int c = nm_bad_designator(designators, nchan); c >= 0) {
        set_err("aisx_nmea_parse_batch_create: designator %d is missing or longer than %d bytes", c, NM_DESIG);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_nmea_parse_batch, aisx_nmea_parse_batch_destroy> h(
        new aisx_nmea_parse_batch(NmpPlan(designators, nchan, length_max, max_line, flags, max_bytes, max_lines, max_pdus)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const NmpPlan& pl = h->pl;
    if ((rc = h->d_desig.alloc(pl.desig)) != AISX_OK || (rc = h->d_dlen.alloc(pl.dlen)) != AISX_OK ||
        (rc = h->d_lcarry.alloc(pl.lcarry)) != AISX_OK || (rc = h->d_gcarry.alloc(pl.gcarry)) != AISX_OK ||
        (rc = h->d_bytes.alloc(pl.bytes)) != AISX_OK || (rc = h->d_st.alloc(pl.st)) != AISX_OK ||
        (rc = h->d_tcount.alloc(pl.tcount)) != AISX_OK || (rc = h->d_toff.alloc(pl.toff)) != AISX_OK ||
        (rc = h->d_meta.alloc(pl.meta)) != AISX_OK || (rc = h->d_cidx.alloc(pl.cidx)) != AISX_OK ||
        (rc = h->d_aux.alloc(pl.aux)) != AISX_OK || (rc = h->d_count.alloc(pl.count)) != AISX_OK ||
        (rc = h->d_lend.alloc(pl.lend)) != AISX_OK || (rc = h->d_pos.alloc(pl.pos)) != AISX_OK ||
        (rc = h->d_tm.alloc(pl.tm)) != AISX_OK || (rc = h->d_times.alloc(pl.times)) != AISX_OK ||
        (rc = h->d_key.alloc(pl.key)) != AISX_OK || (rc = h->d_rec.alloc(pl.rec)) != AISX_OK ||
        (rc = h->d_next.alloc(pl.next)) != AISX_OK || (rc = h->d_mlen.alloc(pl.mlen)) != AISX_OK ||
        (rc = h->d_tl.alloc(pl.tl)) != AISX_OK || (rc = h->d_tlb.alloc(pl.tlb)) != AISX_OK ||
        (rc = h->d_bstat.alloc(pl.bstat)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_desig, pl.desig_host.data(), pl.desig.n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_dlen, pl.dlen_host.data(), pl.dlen.n, hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_nmea_parse_batch_create: copying the designators failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_batch_reset(aisx_nmea_parse_batch* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipDeviceSynchronize());
    AISX_HIPCHK(hipMemset(h->d_st, 0, h->pl.st.n * sizeof(NmpState)));
    AISX_HIPCHK(hipMemset(h->d_meta, 0, h->pl.meta.n * sizeof(int)));
    AISX_HIPCHK(hipMemset(h->d_count, 0, h->pl.count.n * sizeof(int)));
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_batch_process(aisx_nmea_parse_batch* h, const char* d_text, const long long* d_nbytes,
                                             void* stream)
{
    if (!h || !d_text || !d_nbytes) {
        set_err("aisx_nmea_parse_batch_process: a handle, text and a byte count are needed");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    const NmpBufs b = { h->d_desig, h->d_dlen, h->d_st,  h->d_lcarry, h->d_gcarry, h->d_tcount, h->d_toff, h->d_meta,
                        h->d_lend,  h->d_key,  h->d_pos, h->d_tm,     h->d_cidx,   h->d_mlen,   h->d_tl,   h->d_tlb,
                        h->d_bstat, h->d_rec,  h->d_aux, h->d_times,  h->d_bytes,  h->d_count,  h->d_next };
    hipError_t err = hipSuccess;
    h->pl.process(b, (const unsigned char*)d_text, d_nbytes, [&](const PlanLaunch& l, const NmpParams& p) {
        static void (*const kernels[NP_NKERNELS])(NmpParams) = { k_nmp_count,    k_nmp_scan, k_nmp_index,  k_nmp_parse,  k_nmp_gcount, k_nmp_gscan1,
                                                                  k_nmp_gcompact, k_nmp_gmsg, k_nmp_gscan2, k_nmp_gplace, k_nmp_write,  k_nmp_carry };
        hipLaunchKernelGGL(kernels[l.kernel], dim3(l.gx), dim3(l.threads), 0, st, p);
        // (checked behind the last kernel of the lines and sentences, and behind the last of all)
        return (l.kernel != NP_K_GPLACE && l.kernel != NP_K_CARRY) || (err = hipGetLastError()) == hipSuccess;
    });
    AISX_LAUNCHCHK(err);
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_batch_results_device(const aisx_nmea_parse_batch* h, const aisx_pdu** d_pdus,
                                                    const uint8_t** d_bytes, const int** d_count, const int64_t** d_times)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_pdus)
        *d_pdus = (const aisx_pdu*)h->d_rec.get();
    if (d_bytes)
        *d_bytes = h->d_bytes;
    if (d_count)
        *d_count = h->d_count;
    if (d_times)
        *d_times = (const int64_t*)h->d_times.get();
    return AISX_OK;
}

extern "C" int aisx_nmea_parse_batch_read(aisx_nmea_parse_batch* h, aisx_pdu* pdus, int pdu_cap, uint8_t* bytes,
                                          long bytes_cap, int64_t* times, int* counts, void* stream)
{
    if (!h || !counts || pdu_cap < 0 || bytes_cap < 0 || (pdu_cap > 0 && !pdus) || (bytes_cap > 0 && !bytes))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[NP_NCNT];
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    int k = cnt[AISX_NMEAP_KEPT] < pdu_cap ? cnt[AISX_NMEAP_KEPT] : pdu_cap;
    if (k > 0)
        AISX_HIPCHK(hipMemcpyAsync(pdus, h->d_rec, sizeof(aisx_pdu) * k, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    while (k > 0 && pdus[k - 1].offset + pdus[k - 1].len > bytes_cap)
        k--;
    const long long nb = k > 0 ? pdus[k - 1].offset + pdus[k - 1].len : 0;
    if (nb > 0)
        AISX_HIPCHK(hipMemcpyAsync(bytes, h->d_bytes, (size_t)nb, hipMemcpyDeviceToHost, st));
    if (times && k > 0)
        AISX_HIPCHK(hipMemcpyAsync(times, h->d_times, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st));
    if (cnt[AISX_NMEAP_BAD_INPUT])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + AISX_NMEAP_BAD_INPUT, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    cnt[AISX_NMEAP_KEPT] = k;
    memcpy(counts, cnt, sizeof cnt);
    if (cnt[AISX_NMEAP_BAD_INPUT]) {
        set_err("aisx_nmea_parse_batch_read: a call since the last read had a byte count outside [0, %lld] or more than %d "
                "line ends: it was refused and advanced nothing", h->pl.max_bytes, h->pl.max_lines);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[AISX_NMEAP_FOUND]) {
        set_err("aisx_nmea_parse_batch_read: %d messages found, %d records kept", cnt[AISX_NMEAP_FOUND], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
