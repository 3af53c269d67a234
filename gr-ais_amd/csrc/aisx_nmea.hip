// aisx_nmea.hip -- C ABI of the batched NMEA armouring (include/aisx.h, aisx_nmea_batch_*): per call, one workgroup
// sizes and places every record's text (k_nmea.h: nmea_scan_body) and one wave per record writes it
// (nmea_write_body).  Everything is queued on the caller's stream; the record count is read on the device.  A handle made
// by aisx_nmea_batch_create_std runs the standard form's two kernels (k_nmea_std.h) in their place.
#include <memory>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_nmea_std.h"

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

__global__ __launch_bounds__(NM_SCAN_T) void k_nmea_std_scan(NmeaStdScanParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[(4 * (NM_SCAN_T / 64) + 4) * 4];
    DevCtx cx{ smem };
    nmea_std_scan_body(cx, p);
}

__global__ __launch_bounds__(NM_W_T) void k_nmea_std_write(NmeaStdWriteParams p)
{
    DevCtx cx{ nullptr };
    nmea_std_write_body(cx, p);
}

struct aisx_nmea_batch {
    explicit aisx_nmea_batch(NmeaPlan&& plan) : pl(std::move(plan)) {}
    explicit aisx_nmea_batch(NmeaStdPlan&& plan) : pl(plan), sp(new NmeaStdPlan(std::move(plan))) {}
    int dev = 0;
    const NmeaPlan pl;            // the arguments, the sizes derived from them and the per-call sequence (k_nmea.h)
    DevBuf<char> d_desig;         // [nchan][NM_DESIG]
    DevBuf<unsigned char> d_dlen; // [nchan]
    DevBuf<HdlcRec> d_out;        // [max_pdus]
    DevBuf<char> d_text;          // [text_cap]
    DevBuf<int> d_count;          // [0] found, [1] records written, [2] bad-input flag, [3] the message-id counter
    // the standard form only (sp: its plan, of which pl is the part every form shares)
    const std::unique_ptr<const NmeaStdPlan> sp;
    DevBuf<char> d_station;       // [nchan][NMS_STRIDE]
    DevBuf<unsigned char> d_slen; // [nchan]
    DevBuf<unsigned char> d_ids;  // [max_pdus]
    Event done;                   // behind the last call's work (reset waits for it)
    long long time = -1;          // the c: value of the next calls
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
    if (const char* why = NmeaPlan::check(designators, nchan, max_pdus, length_max, text_cap)) {
        set_err("aisx_nmea_batch_create: %s", why);
        return AISX_ERR_INVALID;
    }
    if (const int c = nm_bad_designator(designators, nchan); c >= 0) {
        set_err("aisx_nmea_batch_create: designator %d is missing or longer than %d bytes", c, NM_DESIG);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_nmea_batch, aisx_nmea_batch_destroy> h(new aisx_nmea_batch(NmeaPlan(designators, nchan, max_pdus, length_max, text_cap)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const NmeaPlan& pl = h->pl;
    if ((rc = h->d_desig.alloc(pl.desig)) != AISX_OK || (rc = h->d_dlen.alloc(pl.dlen)) != AISX_OK ||
        (rc = h->d_out.alloc(pl.out)) != AISX_OK || (rc = h->d_text.alloc(pl.text)) != AISX_OK ||
        (rc = h->d_count.alloc(pl.count)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_desig, pl.desig_host.data(), pl.desig.n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_dlen, pl.dlen_host.data(), pl.dlen.n, hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_nmea_batch_create: copying the designators failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_create_std(aisx_nmea_batch** out, const char* const* designators, const char* const* stations,
                                          int nchan, int max_pdus, int length_max, long text_cap)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (const char* why = NmeaStdPlan::check(designators, nchan, max_pdus, length_max, text_cap)) {
        set_err("aisx_nmea_batch_create_std: %s", why);
        return AISX_ERR_INVALID;
    }
    if (const int c = nm_bad_designator(designators, nchan); c >= 0) {
        set_err("aisx_nmea_batch_create_std: designator %d is missing or longer than %d bytes", c, NM_DESIG);
        return AISX_ERR_INVALID;
    }
    if (const int c = nms_bad_station(stations, nchan); c >= 0) {
        set_err("aisx_nmea_batch_create_std: station %d is missing or not 0..%d bytes of A-Z a-z 0-9 _ -", c, NMS_STATION);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_nmea_batch, aisx_nmea_batch_destroy> h(
        new aisx_nmea_batch(NmeaStdPlan(designators, stations, nchan, max_pdus, length_max, text_cap)));
    AISX_HIPCHK(hipGetDevice(&h->dev));
    const NmeaStdPlan& pl = *h->sp;
    if ((rc = h->d_desig.alloc(pl.desig)) != AISX_OK || (rc = h->d_dlen.alloc(pl.dlen)) != AISX_OK ||
        (rc = h->d_out.alloc(pl.out)) != AISX_OK || (rc = h->d_text.alloc(pl.text)) != AISX_OK ||
        (rc = h->d_count.alloc(pl.count)) != AISX_OK || (rc = h->d_station.alloc(pl.station)) != AISX_OK ||
        (rc = h->d_slen.alloc(pl.slen)) != AISX_OK || (rc = h->d_ids.alloc(pl.ids)) != AISX_OK ||
        (rc = h->done.create(hipEventDisableTiming)) != AISX_OK)
        return rc;
    if (hipMemcpy(h->d_desig, pl.desig_host.data(), pl.desig.n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_dlen, pl.dlen_host.data(), pl.dlen.n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_station, pl.station_host.data(), pl.station.n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_slen, pl.slen_host.data(), pl.slen.n, hipMemcpyHostToDevice) != hipSuccess) {
        set_err("aisx_nmea_batch_create_std: copying the designators and stations failed");
        return AISX_ERR_HIP;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_set_time(aisx_nmea_batch* h, int64_t time)
{
    if (!h || !h->sp || !nms_time_ok(time)) {
        set_err("aisx_nmea_batch_set_time: needs a handle in the standard form and a time of -1 or 0 .. 10^18 - 1");
        return AISX_ERR_INVALID;
    }
    h->time = time;
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_reset(aisx_nmea_batch* h)
{
    if (!h || !h->sp) {
        set_err("aisx_nmea_batch_reset: needs a handle in the standard form");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    AISX_HIPCHK(hipEventSynchronize(h->done)); // (the last call's kernels; nothing else on the device)
    AISX_HIPCHK(hipMemsetAsync(h->d_count + 3, 0, sizeof(int), nullptr));
    AISX_HIPCHK(hipStreamSynchronize(nullptr)); // (done before the next call, whatever stream that is queued on)
    h->time = -1;
    return AISX_OK;
}

extern "C" int aisx_nmea_batch_next_id(aisx_nmea_batch* h, int* id, void* stream)
{
    if (!h || !h->sp || !id) {
        set_err("aisx_nmea_batch_next_id: needs a handle in the standard form");
        return AISX_ERR_INVALID;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const hipStream_t st = (hipStream_t)stream;
    AISX_HIPCHK(hipMemcpyAsync(id, h->d_count + 3, sizeof(int), hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipStreamSynchronize(st));
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
    const NmeaBufs b = { h->d_desig, h->d_dlen, h->d_out, h->d_text, h->d_count };
    hipError_t err = hipSuccess;
    if (h->sp) {
        const NmeaStdBufs sb = { b, h->d_station, h->d_slen, h->d_ids };
        h->sp->process(sb, (const HdlcRec*)d_pdus, d_bytes, d_npdus, d_nfound, h->time, [&](const PlanLaunch& l, const NmeaStdCall& c) {
            if (l.kernel == NM_K_STD_SCAN)
                hipLaunchKernelGGL(k_nmea_std_scan, dim3(l.gx), dim3(l.threads), 0, st, c.s);
            else
                hipLaunchKernelGGL(k_nmea_std_write, dim3(l.gx), dim3(l.threads), 0, st, c.w);
            return (err = hipGetLastError()) == hipSuccess;
        });
        AISX_LAUNCHCHK(err);
        AISX_HIPCHK(hipEventRecord(h->done, st));
        return AISX_OK;
    }
    h->pl.process(b, (const HdlcRec*)d_pdus, d_bytes, d_npdus, d_nfound, [&](const PlanLaunch& l, const NmeaCall& c) {
        if (l.kernel == NM_K_SCAN)
            hipLaunchKernelGGL(k_nmea_scan, dim3(l.gx), dim3(l.threads), 0, st, c.s);
        else
            hipLaunchKernelGGL(k_nmea_write, dim3(l.gx), dim3(l.threads), 0, st, c.w);
        return (err = hipGetLastError()) == hipSuccess;
    });
    AISX_LAUNCHCHK(err);
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
                "outside [0, %d) or a payload longer than %d octets: those gave no text", h->pl.max_pdus, h->pl.nchan, h->pl.lmax - 1);
        return AISX_ERR_INVALID;
    }
    if (k < cnt[0]) {
        set_err("aisx_nmea_batch_read: %d PDUs found, %d armoured", cnt[0], k);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}
