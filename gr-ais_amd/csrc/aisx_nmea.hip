// aisx_nmea.hip -- C ABI of the batched NMEA armouring (include/aisx.h, aisx_nmea_batch_*): per call, one workgroup
// sizes and places every record's text (k_nmea.h: nmea_scan_body) and one wave per record writes it
// (nmea_write_body).  Everything is queued on the caller's stream; the record count is read on the device.
#include <string.h>

#include <vector>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_nmea.h"

using namespace aisx;

static_assert(sizeof(HdlcRec) == sizeof(aisx_pdu), "pdu record layout");

__global__ __launch_bounds__(NM_SCAN_T) void k_nmea_scan(NmeaScanParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[(2 * (NM_SCAN_T / 64) + 2) * 4];
    DevCtx cx{ smem };
    nmea_scan_body(cx, p);
}

__global__ __launch_bounds__(NM_W_T) void k_nmea_write(NmeaWriteParams p)
{
    DevCtx cx{ nullptr };
    nmea_write_body(cx, p);
}

struct aisx_nmea_batch {
    int dev = 0;
    int nchan = 0, max_pdus = 0, lmax = 0, write_groups = 0;
    long long text_cap = 0;
    DevBuf<char> d_desig;         // [nchan][NM_DESIG]
    DevBuf<unsigned char> d_dlen; // [nchan]
    DevBuf<HdlcRec> d_out;        // [max_pdus]
    DevBuf<char> d_text;          // [text_cap]
    DevBuf<int> d_count;          // [0] found, [1] records written, [2] bad-input flag
};

extern "C" int aisx_nmea_batch_destroy(aisx_nmea_batch* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    delete h;
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_create(aisx_nmea_batch** out, const char* const* designators, int nchan, int max_pdus,
                                      int length_max, long text_cap)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (!designators || nchan < 1 || max_pdus < 1 || length_max < 2 || length_max > NM_MAX_OCTETS || text_cap < 0) {
        set_err("aisx_nmea_batch_create: need designators, nchan >= 1, max_pdus >= 1, 2 <= length_max <= %d, "
                "text_cap >= 0", NM_MAX_OCTETS);
        return AISX_ERR_INVALID;
    }
    int max_dlen = 0;
    for (int c = 0; c < nchan; c++) {
        const size_t n = designators[c] ? strnlen(designators[c], NM_DESIG + 1) : NM_DESIG + 1;
        if (n > (size_t)NM_DESIG) {
            set_err("aisx_nmea_batch_create: designator %d is missing or longer than %d bytes", c, NM_DESIG);
            return AISX_ERR_INVALID;
        }
        max_dlen = (int)n > max_dlen ? (int)n : max_dlen;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_nmea_batch, aisx_nmea_batch_destroy> h(new aisx_nmea_batch());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->nchan = nchan;
    h->max_pdus = max_pdus;
    h->lmax = length_max;
    // the worst case: every record as long as a payload can be, on the channel with the longest designator
    const long long worst = (long long)max_pdus * (nm_text_len(length_max - 1, max_dlen) + 1);
    h->text_cap = text_cap == 0 || text_cap > worst ? worst : text_cap;
    const long long groups = ((long long)max_pdus + NM_W_T / 64 - 1) / (NM_W_T / 64);
    h->write_groups = (int)(groups < NM_W_MAX_GROUPS ? groups : NM_W_MAX_GROUPS);
    std::vector<char> desig((size_t)nchan * NM_DESIG, 0);
    std::vector<unsigned char> dlen(nchan);
    for (int c = 0; c < nchan; c++) {
        dlen[c] = (unsigned char)strlen(designators[c]);
        memcpy(desig.data() + (size_t)c * NM_DESIG, designators[c], dlen[c]);
    }
    if ((rc = h->d_desig.alloc((size_t)nchan * NM_DESIG, false)) != AISX_OK || (rc = h->d_dlen.alloc((size_t)nchan, false)) != AISX_OK ||
        (rc = h->d_out.alloc((size_t)max_pdus, false)) != AISX_OK || (rc = h->d_text.alloc((size_t)h->text_cap, false)) != AISX_OK ||
        (rc = h->d_count.alloc(4)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_desig, desig.data(), desig.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_dlen, dlen.data(), dlen.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_nmea_batch_create: copying the designators failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_process(aisx_nmea_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes,
                                       const int* d_npdus, const int* d_nfound, void* stream)
{
    if (!h || !d_pdus || !d_bytes || !d_npdus) {
        set_err("aisx_nmea_batch_process: a handle, records, bytes and a record count are needed");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    NmeaScanParams s;
    s.in = (const HdlcRec*)d_pdus;
    s.npdus = d_npdus;
    s.nfound = d_nfound;
    s.dlen = h->d_dlen;
    s.nchan = h->nchan;
    s.max_pdus = h->max_pdus;
    s.max_len = h->lmax - 1;
    s.text_cap = h->text_cap;
    s.out = h->d_out;
    s.count = h->d_count;
    hipLaunchKernelGGL(k_nmea_scan, dim3(1), dim3(NM_SCAN_T), 0, st, s);
    AISX_HIPCHK(hipGetLastError());
    NmeaWriteParams w;
    w.in = s.in;
    w.bytes = d_bytes;
    w.out = h->d_out;
    w.count = h->d_count;
    w.desig = h->d_desig;
    w.dlen = h->d_dlen;
    w.text = h->d_text;
    w.nwaves = h->write_groups * (NM_W_T / 64);
    hipLaunchKernelGGL(k_nmea_write, dim3(h->write_groups), dim3(NM_W_T), 0, st, w);
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_results_device(const aisx_nmea_batch* h, const aisx_pdu** d_recs, const char** d_text,
                                              const int** d_count)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (d_recs)
        *d_recs = (const aisx_pdu*)h->d_out.get();
    if (d_text)
        *d_text = h->d_text;
    if (d_count)
        *d_count = h->d_count;
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_read(aisx_nmea_batch* h, aisx_pdu* recs, int rec_cap, char* text, long text_cap,
                                    int* nrecs, int* nfound, void* stream)
{
    if (!h || !nrecs || rec_cap < 0 || text_cap < 0 || (rec_cap > 0 && !recs) || (text_cap > 0 && !text))
        return AISX_ERR_INVALID;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    int cnt[3] = { 0, 0, 0 };
    AISX_HIPCHK(hipMemcpyAsync(cnt, h->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    int k = cnt[1] < rec_cap ? cnt[1] : rec_cap;
    if (k > 0)
        AISX_HIPCHK(hipMemcpyAsync(recs, h->d_out, sizeof(aisx_pdu) * k, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    // (records are in text order: the ones whose text and newline fit text_cap are a prefix again)
    auto text_end = [](const aisx_pdu& r) { return r.offset + r.len + (r.len > 0 ? 1 : 0); };
    while (k > 0 && text_end(recs[k - 1]) > text_cap)
        k--;
    const long long nt = k > 0 ? text_end(recs[k - 1]) : 0;
    if (nt > 0)
        AISX_HIPCHK(hipMemcpyAsync(text, h->d_text, (size_t)nt, hipMemcpyDeviceToHost, st));
    if (cnt[2])
        AISX_HIPCHK(hipMemsetAsync(h->d_count + 2, 0, sizeof(int), st));
    AISX_HIPCHK(hipStreamSynchronize(st));
    *nrecs = k;
    if (nfound)
        *nfound = cnt[0];
    if (cnt[2]) {
        set_err("aisx_nmea_batch_read: a call since the last read met a record count outside [0, %d], a channel "
                "outside [0, %d) or a payload longer than %d octets: those gave no text", h->max_pdus, h->nchan, h->lmax - 1);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[0]) {
        set_err("aisx_nmea_batch_read: %d PDUs found, %d armoured", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
