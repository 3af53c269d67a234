// aisx_nmea_parse.hip -- C ABI of the batched NMEA parser (include/aisx.h, aisx_nmea_parse_batch_*): per call the twelve
// kernels of k_nmea_parse.h, queued on the caller's stream; the byte count is read on the device, and so is everything
// the handle carries from call to call.
#include <string.h>

#include <vector>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_nmea_parse.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");
static_assert(NP_NCNT == AISX_NMEAP_NCNT, "counts layout");

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
    int dev = 0;
    int nchan = 0, lmax = 0, max_line = 0, flags = 0, max_lines = 0, max_pdus = 0;
    long long max_bytes = 0;
    int tile_groups = 0, line_groups = 0, pdu_groups = 0, ltile_groups = 0;
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
    if (!designators || nchan < 1 || length_max < 2 || length_max > NM_MAX_OCTETS || max_line < 64 || max_line > 4096 ||
        (flags & ~AISX_NMEA_PARSE_REF_TAIL) || max_bytes < 1 || max_bytes > (1l << 30) || max_lines < 1 ||
        max_lines > (1 << 26) || max_pdus < 1) {
        set_err("aisx_nmea_parse_batch_create: need designators, nchan >= 1, 2 <= length_max <= %d, 64 <= max_line <= 4096, "
                "flags 0 or 1, 1 <= max_bytes <= 2^30, 1 <= max_lines <= 2^26, max_pdus >= 1", NM_MAX_OCTETS);
        return AISX_ERR_INVALID;
    }
    for (int c = 0; c < nchan; c++)
        if (!designators[c] || strnlen(designators[c], NM_DESIG + 1) > (size_t)NM_DESIG) {
            set_err("aisx_nmea_parse_batch_create: designator %d is missing or longer than %d bytes", c, NM_DESIG);
            return AISX_ERR_INVALID;
        }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_nmea_parse_batch, aisx_nmea_parse_batch_destroy> h(new aisx_nmea_parse_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->nchan = nchan;
    h->lmax = length_max;
    h->max_line = max_line;
    h->flags = flags;
    h->max_bytes = max_bytes;
    h->max_lines = max_lines;
    h->max_pdus = max_pdus;
    auto groups = [](long long items, int per_group) {
        const long long g = (items + per_group - 1) / per_group;
        return (int)(g < 1 ? 1 : g < NP_MAX_GROUPS ? g : NP_MAX_GROUPS);
    };
    const long long ntiles = (max_bytes + NP_T * NP_CHUNK - 1) / (NP_T * NP_CHUNK);
    h->tile_groups = groups(ntiles, 1);
    h->line_groups = groups(max_lines, NP_T / 64);
    h->pdu_groups = groups(max_pdus, NP_T / 64);
    const size_t nlt = ((size_t)max_lines + NP_GMAX + NP_T - 1) / NP_T; // tiles of lines / sentences
    h->ltile_groups = groups((long long)nlt, 1);
    std::vector<char> desig((size_t)nchan * NM_DESIG, 0);
    std::vector<unsigned char> dlen(nchan);
    for (int c = 0; c < nchan; c++) {
        dlen[c] = (unsigned char)strlen(designators[c]);
        memcpy(desig.data() + (size_t)c * NM_DESIG, designators[c], dlen[c]);
    }
    const size_t nl = (size_t)max_lines, np = (size_t)max_pdus;
    if ((rc = h->d_desig.alloc(desig.size(), false)) != AISX_OK || (rc = h->d_dlen.alloc(dlen.size(), false)) != AISX_OK ||
        (rc = h->d_lcarry.alloc(2 * (size_t)max_line)) != AISX_OK || (rc = h->d_gcarry.alloc(2 * (size_t)NP_GMAX * max_line)) != AISX_OK ||
        (rc = h->d_bytes.alloc(np * (size_t)(length_max - 1), false)) != AISX_OK || (rc = h->d_st.alloc(2)) != AISX_OK ||
        (rc = h->d_tcount.alloc((size_t)ntiles, false)) != AISX_OK || (rc = h->d_toff.alloc((size_t)ntiles, false)) != AISX_OK ||
        (rc = h->d_meta.alloc(NP_M_N)) != AISX_OK || (rc = h->d_cidx.alloc(nl, false)) != AISX_OK ||
        (rc = h->d_aux.alloc(np, false)) != AISX_OK || (rc = h->d_count.alloc(NP_NCNT)) != AISX_OK ||
        (rc = h->d_lend.alloc(nl, false)) != AISX_OK || (rc = h->d_pos.alloc(nl, false)) != AISX_OK ||
        (rc = h->d_tm.alloc(nl, false)) != AISX_OK || (rc = h->d_times.alloc(np, false)) != AISX_OK ||
        (rc = h->d_key.alloc(nl, false)) != AISX_OK || (rc = h->d_rec.alloc(np, false)) != AISX_OK ||
        (rc = h->d_next.alloc(1)) != AISX_OK || (rc = h->d_mlen.alloc(nl + NP_GMAX, false)) != AISX_OK ||
        (rc = h->d_tl.alloc(nlt, false)) != AISX_OK || (rc = h->d_tlb.alloc(nlt, false)) != AISX_OK ||
        (rc = h->d_bstat.alloc((size_t)NP_MAX_GROUPS * 8)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_desig, desig.data(), desig.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_dlen, dlen.data(), dlen.size(), hipMemcpyHostToDevice) != hipSuccess) {
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
    AISX_HIPCHK(hipMemset(h->d_st, 0, 2 * sizeof(NmpState)));
    AISX_HIPCHK(hipMemset(h->d_meta, 0, NP_M_N * sizeof(int)));
    AISX_HIPCHK(hipMemset(h->d_count, 0, NP_NCNT * sizeof(int)));
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
    NmpParams p;
    p.text = (const unsigned char*)d_text;
    p.nbytes = d_nbytes;
    p.max_bytes = h->max_bytes;
    p.max_lines = h->max_lines;
    p.max_pdus = h->max_pdus;
    p.max_len = h->lmax - 1;
    p.max_line = h->max_line;
    p.flags = h->flags;
    p.nchan = h->nchan;
    p.desig = h->d_desig;
    p.dlen = h->d_dlen;
    p.st = h->d_st;
    p.lcarry = h->d_lcarry;
    p.gcarry = h->d_gcarry;
    p.tcount = h->d_tcount;
    p.toff = h->d_toff;
    p.meta = h->d_meta;
    p.lend = h->d_lend;
    p.key = h->d_key;
    p.pos = h->d_pos;
    p.tm = h->d_tm;
    p.cidx = h->d_cidx;
    p.mlen = h->d_mlen;
    p.tl = h->d_tl;
    p.tlb = h->d_tlb;
    p.bstat = h->d_bstat;
    p.rec = h->d_rec;
    p.aux = h->d_aux;
    p.times = h->d_times;
    p.bytes = h->d_bytes;
    p.count = h->d_count;
    p.next = h->d_next;
    p.ngroups = h->tile_groups;
    p.nwaves = h->line_groups * (NP_T / 64);
    hipLaunchKernelGGL(k_nmp_count, dim3(h->tile_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_scan, dim3(1), dim3(NP_SCAN_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_index, dim3(h->tile_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_parse, dim3(h->line_groups), dim3(NP_T), 0, st, p);
    p.ngroups = h->ltile_groups;
    hipLaunchKernelGGL(k_nmp_gcount, dim3(h->ltile_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_gscan1, dim3(1), dim3(NP_SCAN_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_gcompact, dim3(h->ltile_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_gmsg, dim3(h->ltile_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_gscan2, dim3(1), dim3(NP_SCAN_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_gplace, dim3(h->ltile_groups), dim3(NP_T), 0, st, p);
    AISX_HIPCHK(hipGetLastError());
    p.nwaves = h->pdu_groups * (NP_T / 64);
    hipLaunchKernelGGL(k_nmp_write, dim3(h->pdu_groups), dim3(NP_T), 0, st, p);
    hipLaunchKernelGGL(k_nmp_carry, dim3(1), dim3(64), 0, st, p);
    AISX_HIPCHK(hipGetLastError());
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
                "line ends: it was refused and advanced nothing", h->max_bytes, h->max_lines);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[AISX_NMEAP_FOUND]) {
        set_err("aisx_nmea_parse_batch_read: %d messages found, %d records kept", cnt[AISX_NMEAP_FOUND], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
