// aisx_rx.hip -- C ABI of the host-fed receiver (include/aisx.h, aisx_rx_*): python/radio.py's ais_rx as one handle
// for nstreams sources, fed from pinned host memory in the source's own sample format.  Nothing here computes: the
// handle owns the filter (aisx_xlate), the four stage handles and their chain, the tail behind the chain step (RxTail:
// the deframer and the NMEA stage and, where the aisx_rx_enable_* calls asked for them, the sequence detector before the
// deframer, the duplicate suppression behind it, the field decoder behind the NMEA stage and the vessel table behind the
// decoder), and the rings, streams and events that order them (INTEGRATION.md states the rules; this file is their one
// home).
//
//   block b, submitted:   copy stream    pinned slot b % NPIN -> raw buffer b % NRAW      (after filter b - NRAW)
//                         filter stream  raw buffer -> row buffer b % NROW                (after wait_input(b - NROW))
//                         chain          step b - 1 with d_in_next = row buffer b % NROW  (after tail b - 1 - DEPTH)
//                         tail stream    wait(step b - 1), [detector,] deframer, [dedup,] NMEA, status, results -> pinned result slot
//
// so the copy of block b + 1 runs beside the compute of block b, and the host never waits for the device in submit.
#include <string.h>

#include <string>
#include <vector>

#include "aisx_devctx.h"
#include "aisx_host.h"
#include "k_mlse.h"
#include "k_nmea_std.h"
#include "k_xlate.h"

using namespace aisx;

namespace {

constexpr int RX_NPIN = 3;                     // pinned host input slots
constexpr int RX_NRAW = 2;                     // raw-input buffers on the device
constexpr int RX_NROW = AISX_CHAIN_DEPTH + 1;  // row buffers (the filter's outputs, the chain's inputs)
constexpr int RX_NOUT = AISX_CHAIN_DEPTH;      // sets of bits / produced (aisx_chain_step: one per step in flight)
constexpr int RX_NRES = 8;                     // pinned result slots
constexpr int RX_FFTLEN = 1024, RX_LMIN = 11, RX_LMAX = 64;
constexpr int RX_META = 16;                    // ints: msk status, deframer count[3], NMEA count[3], spare, the dedup stage's counts
static_assert(8 + AISX_DEDUP_NCNT <= RX_META && RX_META % 2 == 0, "the counts fit, and the records behind stay 8-byte aligned");

// filter.firdes.low_pass(gain 1, fs, cutoff, transition) with the Hamming window (radio.py:51)
std::vector<float> low_pass(double fs, double cutoff, double transition)
{
    int ntaps = (int)(53.0 * fs / (22.0 * transition));
    if ((ntaps & 1) == 0)
        ntaps++;
    const int m = (ntaps - 1) / 2;
    const double pi = 3.14159265358979323846, fwt0 = 2 * pi * cutoff / fs;
    std::vector<float> t((size_t)ntaps);
    for (int i = 0; i < ntaps; i++) {
        const int n = i - m;
        const double w = 0.54 - 0.46 * cos(2 * pi * i / (ntaps - 1));
        t[i] = (float)((n == 0 ? fwt0 / pi : sin(n * fwt0) / (n * pi)) * w);
    }
    double fmax = t[m];
    for (int i = m + 1; i < ntaps; i++)
        fmax += 2 * (double)t[i];
    for (float& v : t)
        v = (float)((double)v * (1.0 / fmax));
    return t;
}

} // namespace

// one workgroup: the recovery's status words or-ed over the channels, and the deframer's and the NMEA stage's counts,
// gathered into one record for the copy back
// (ml_flag: the detector's bad-count word or nullptr; it counts as the deframer's, and so does the flag of dd_count, the
// duplicate suppression's count words or nullptr)
__global__ __launch_bounds__(256) void k_rx_meta(const int* __restrict__ msk_status, int nchan, const int* __restrict__ hd_count,
                                                 const int* __restrict__ nm_count, const int* __restrict__ ml_flag, const int* __restrict__ dd_count,
                                                 int* __restrict__ meta)
{
    __shared__ int acc;
    if (threadIdx.x == 0)
        acc = 0;
    __syncthreads();
    int v = 0;
    for (int c = threadIdx.x; c < nchan; c += blockDim.x)
        v |= msk_status[c];
    if (v)
        atomicOr(&acc, v);
    __syncthreads();
    if (threadIdx.x == 0) {
        meta[0] = acc;
        for (int i = 0; i < 3; i++) {
            meta[1 + i] = hd_count[i];
            meta[4 + i] = nm_count[i];
        }
        if (ml_flag)
            meta[3] |= *ml_flag;
        meta[7] = 0;
        for (int i = 0; i < AISX_DEDUP_NCNT; i++)
            meta[8 + i] = dd_count ? dd_count[3 + i] : 0;
        if (dd_count)
            meta[3] |= dd_count[2];
    }
}

// what the aisx_rx_enable_* calls have asked for; a new receiver has the default record
struct RxOptions {
    bool messages = false;              // the field decoder behind the NMEA stage
    bool tracks = false;                // the vessel table behind the decoder,
    int capacity = 0;                   // of so many vessels (the table's create judges the number)
    std::vector<aisx_hdlc_rule> rules;  // the deframer's repair: on with at least one rule,
    int events = AISX_HDLC_EV_SINGLE;   // and the error events to look for
    bool detector = false;              // the sequence detector between the chain step and the deframer,
    double bt = 0.0;                    // of this BT
    bool std_nmea = false;              // the NMEA stage writes the standard form, with
    std::vector<std::string> stations;  // these stations, one per stream,
    long long t0 = -1;                  // and its tag blocks' time counted from here (-1: none)
    bool dedup = false;                 // the duplicate suppression between the deframer and the NMEA stage,
    int window = 0;                     // remembering so many blocks
};

// a pinned result slot: byte offsets of its areas in this order, the optional ones 16-byte aligned, and its size
struct RxLayout {
    size_t recs = 0; // aisx_pdu recs[max_pdus], behind int meta[RX_META] at 0
    size_t text = 0; // char text[text_cap]
    size_t cols = 0; // with messages: int32 cols[AISX_MSG_NCOL][max_pdus],
    size_t strs = 0; // char strs[max_pdus][AISX_MSG_STR]
    size_t fix = 0;  // with repair: int32 fix_bits[max_pdus]
    size_t bytes = 0;
};

static RxLayout rx_layout(int max_pdus, long long text_cap, bool messages, bool repair)
{
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t n = (size_t)max_pdus;
    RxLayout l;
    l.recs = sizeof(int) * RX_META;
    l.text = l.recs + sizeof(aisx_pdu) * n;
    l.bytes = l.text + (size_t)text_cap;
    if (messages) {
        l.cols = up16(l.bytes);
        l.strs = l.cols + sizeof(int32_t) * AISX_MSG_NCOL * n;
        l.bytes = l.strs + (size_t)AISX_MSG_STR * n;
    }
    if (repair) {
        l.fix = up16(l.bytes);
        l.bytes = l.fix + sizeof(int32_t) * n;
    }
    return l;
}

// everything behind the chain step, made whole from one RxOptions by rx_make_tail.  What an option does not ask for stays
// empty: nothing is allocated, queued or copied for it.  (The stage handles stand last: destroyed before the buffers.)
struct RxTail {
    long long text_cap = 0;
    RxLayout lay;
    PinnedBuf<char> h_res[RX_NRES];
    int mstride = 0;                 // row stride of d_mbits: cap + what the detector carries
    DevBuf<cf> d_syms[RX_NOUT];      // [ns * nch][cap], only with the detector
    DevBuf<uint8_t> d_mbits;         // [ns * nch][mstride] the detector's bits (read by the deframer behind it on the tail stream)
    DevBuf<int> d_mnb;
    const int* d_ml_flag = nullptr;
    const aisx_pdu *d_hd_pdus = nullptr, *d_nm_recs = nullptr;
    const uint8_t* d_hd_bytes = nullptr;
    const char* d_nm_text = nullptr;
    const int *d_hd_count = nullptr, *d_nm_count = nullptr, *d_mg_count = nullptr;
    const int32_t* d_fix = nullptr;  // the deframer's marks, only with repair
    const aisx_pdu* d_ls_pdus = nullptr; // the list NMEA stage, decoder and table read: the deframer's, or the kept records
    const int* d_ls_count = nullptr;     // of the duplicate suppression, with that list's count words
    const int32_t* d_ls_fix = nullptr;   // and that list's marks
    const int32_t* d_mg_cols = nullptr;
    const char* d_mg_strs = nullptr;
    HandlePtr<aisx_mlse_batch, aisx_mlse_batch_destroy> ml;
    HandlePtr<aisx_hdlc_batch, aisx_hdlc_batch_destroy> hd;
    HandlePtr<aisx_dedup_batch, aisx_dedup_batch_destroy> dd;
    HandlePtr<aisx_nmea_batch, aisx_nmea_batch_destroy> nm;
    HandlePtr<aisx_msg_batch, aisx_msg_batch_destroy> mg;
    HandlePtr<aisx_track_batch, aisx_track_batch_destroy> tk;
};

struct aisx_rx {
    int dev = 0;
    int fmt = 0, item_bytes = 0, ns = 0, nch = 0, D = 0, T = 0, block_items = 0, max_pdus = 0, cap = 0;
    float scale = 1.f, bias = 0.f;
    size_t raw_bytes = 0;
    aisx_xlate* xl = nullptr;
    aisx_freqsync* fs = nullptr;
    aisx_agc* agc = nullptr;
    aisx_corr* corr = nullptr;
    aisx_msk* msk = nullptr;
    aisx_chain* chain = nullptr;
    double rate = 0.0;
    std::vector<std::string> des;      // the designators, one per centre
    int max_dlen = 0;
    RxOptions opt;
    std::vector<int32_t> popped_fix;   // the repair marks of the block popped last
    int popped_dd[AISX_DEDUP_NCNT] = {}; // and the duplicate suppression's counts of that block
    Stream s_copy, s_filt, s_tail;     // (before the buffers and events used on them: destroyed after those)
    PinnedBuf<char> h_in[RX_NPIN];     // pinned [ns][block_items] items
    DevBuf<char> d_raw[RX_NRAW];
    DevBuf<cf> d_row[RX_NROW];         // [ns * nch][T]
    DevBuf<uint8_t> d_bits[RX_NOUT];   // [ns * nch][cap]
    DevBuf<int> d_prod[RX_NOUT];
    DevBuf<int> d_meta;
    Event ev_copy[RX_NPIN];            // the slot's copy to the device has finished
    Event ev_filt[RX_NRAW];            // the raw buffer's filter call has finished
    Event ev_tail[RX_NOUT];            // the deframer has read this set of bits / produced
    Event ev_res[RX_NRES];             // the result slot is complete
    RxTail tail;                       // what opt asks for (behind every other owner: its stage handles are the first to go)
    const int* d_msk_status = nullptr;
    long long submitted = 0, issued = 0, popped = 0; // blocks copied and filtered; steps issued; results taken
    bool acquired = false;
    int failed = AISX_OK;
    char failed_msg[512] = {};
};

static int rx_fail(aisx_rx* h, int rc)
{
    h->failed = rc;
    snprintf(h->failed_msg, sizeof h->failed_msg, "%s", aisx_last_error());
    return rc;
}

static int rx_failed(const aisx_rx* h, const char* who)
{
    set_err("%s: an earlier block failed (%s): destroy the handle", who, h->failed_msg);
    return h->failed;
}

extern "C" int aisx_rx_destroy(aisx_rx* h)
{
    if (!h)
        return AISX_OK;
    OnDevice on(h->dev);
    for (const Stream* s : { &h->s_copy, &h->s_filt, &h->s_tail })
        if (*s)
            (void)hipStreamSynchronize(*s);
    if (h->chain) {
        (void)aisx_chain_synchronize(h->chain);
        (void)aisx_chain_destroy(h->chain); // (before the stage handles it borrows)
    }
    if (h->s_tail)
        (void)hipStreamSynchronize(h->s_tail);
    (void)aisx_msk_destroy(h->msk);
    (void)aisx_corr_destroy(h->corr);
    (void)aisx_agc_destroy(h->agc);
    (void)aisx_freqsync_destroy(h->fs);
    (void)aisx_xlate_destroy(h->xl);
    // (the tail's stage handles go first in here: every sub-handle is gone before the receiver's own buffers, events
    // and, last, streams)
    delete h;
    return AISX_OK;
}

// a stage's create into the owner of its handle
template <class H, int (*Destroy)(H*), class... A, class... B>
static int rx_make(HandlePtr<H, Destroy>& p, int (*create)(H**, A...), B... args)
{
    H* made = nullptr;
    const int rc = create(&made, args...);
    p.reset(made);
    return rc;
}

// The tail `o` asks for, whole, into the empty *t: the one place that knows what an option needs of the stages and of a
// result slot.  The stages refuse what they cannot take (a BT, a capacity, rules, a mask) with their own message.
static int rx_make_tail(const aisx_rx* h, const RxOptions& o, const char* who, RxTail* t)
{
    int rc;
    const int rows = h->ns * h->nch, cap = h->cap;
    std::vector<const char*> des((size_t)rows), sta((size_t)rows);
    int max_slen = 0;
    for (int r = 0; r < rows; r++) {
        des[r] = h->des[r % h->nch].c_str();
        sta[r] = o.std_nmea ? o.stations[r / h->nch].c_str() : "";
        max_slen = std::max(max_slen, (int)strlen(sta[r]));
    }
    if (o.detector) { // the step's symbols -> the detector's bits and counts, a step's and the carried ones
        t->mstride = cap + MLSE_EXTRA;
        if ((rc = rx_make(t->ml, aisx_mlse_batch_create, o.bt, rows, cap)) != AISX_OK ||
            (rc = aisx_mlse_batch_status_device(t->ml.get(), &t->d_ml_flag)) != AISX_OK ||
            (rc = t->d_mbits.alloc((size_t)rows * t->mstride, false)) != AISX_OK || (rc = t->d_mnb.alloc((size_t)rows)) != AISX_OK)
            return rc;
        for (auto& b : t->d_syms)
            if ((rc = b.alloc((size_t)rows * cap, false)) != AISX_OK)
                return rc;
    }
    if ((rc = rx_make(t->hd, aisx_hdlc_batch_create, RX_LMIN, RX_LMAX, rows, o.detector ? t->mstride : cap, h->max_pdus)) != AISX_OK ||
        (rc = aisx_hdlc_batch_results_device(t->hd.get(), &t->d_hd_pdus, &t->d_hd_bytes, &t->d_hd_count)) != AISX_OK)
        return rc;
    if (!o.rules.empty() && ((rc = aisx_hdlc_batch_set_repair_events(t->hd.get(), o.rules.data(), (int)o.rules.size(), o.events)) != AISX_OK ||
                             (rc = aisx_hdlc_batch_repairs_device(t->hd.get(), &t->d_fix)) != AISX_OK))
        return rc;
    t->d_ls_pdus = t->d_hd_pdus;
    t->d_ls_count = t->d_hd_count;
    t->d_ls_fix = t->d_fix;
    if (o.dedup) { // the stages behind read the kept records, their count words and their marks
        const int32_t* marks = nullptr;
        if ((rc = rx_make(t->dd, aisx_dedup_batch_create, o.window, h->max_pdus, RX_LMAX)) != AISX_OK ||
            (rc = aisx_dedup_batch_results_device(t->dd.get(), &t->d_ls_pdus, nullptr, &t->d_ls_count, nullptr, nullptr, &marks)) != AISX_OK)
            return rc;
        if (t->d_fix)
            t->d_ls_fix = marks;
    }
    const int sentence = o.std_nmea ? nms_text_len(RX_LMAX - 1, h->max_dlen, nms_tag_len(max_slen, NMS_TIME_DIGITS))
                                    : nm_text_len(RX_LMAX - 1, h->max_dlen);
    t->text_cap = (long long)h->max_pdus * (sentence + 1);
    rc = o.std_nmea ? rx_make(t->nm, aisx_nmea_batch_create_std, des.data(), sta.data(), rows, h->max_pdus, RX_LMAX, (long)t->text_cap)
                    : rx_make(t->nm, aisx_nmea_batch_create, des.data(), rows, h->max_pdus, RX_LMAX, (long)t->text_cap);
    if (rc != AISX_OK || (rc = aisx_nmea_batch_results_device(t->nm.get(), &t->d_nm_recs, &t->d_nm_text, &t->d_nm_count)) != AISX_OK)
        return rc;
    if (o.messages && ((rc = rx_make(t->mg, aisx_msg_batch_create, rows, h->max_pdus, RX_LMAX)) != AISX_OK ||
                       (rc = aisx_msg_batch_results_device(t->mg.get(), &t->d_mg_cols, nullptr, &t->d_mg_strs, &t->d_mg_count)) != AISX_OK))
        return rc;
    if (o.tracks && (rc = rx_make(t->tk, aisx_track_batch_create, o.capacity, h->max_pdus)) != AISX_OK)
        return rc;
    t->lay = rx_layout(h->max_pdus, t->text_cap, o.messages, !o.rules.empty());
    for (int i = 0; i < RX_NRES; i++)
        if ((rc = t->h_res[i].alloc(t->lay.bytes)) != AISX_OK) {
            set_err("%s: %zu bytes of pinned memory for result slot %d could not be had", who, t->lay.bytes, i);
            return rc;
        }
    AISX_HIPCHK(hipDeviceSynchronize()); // (the buffers were zeroed on the null stream, which the handle's streams do not follow)
    return AISX_OK;
}

static int rx_build(aisx_rx* h, double rate, const double* center_freqs, const char* const* designators, const float* taps,
                    int ntaps, const aisx_cf32* tmpl, int ntmpl, int max_dlen)
{
    int rc;
    const int rows = h->ns * h->nch, T = h->T;
    const double sps = rate / h->D / 9600.0;
    if ((rc = aisx_xlate_create(&h->xl, h->D, taps, ntaps, center_freqs, h->nch, rate, h->ns, h->block_items)) != AISX_OK ||
        (rc = aisx_freqsync_create(&h->fs, sps * 9600.0, 9600.0, RX_FFTLEN, rows, T)) != AISX_OK ||
        (rc = aisx_agc_create(&h->agc, 512, 2.f, rows, T + RX_FFTLEN)) != AISX_OK)
        return rc;
    const int tag_cap = 4 * ((T + RX_FFTLEN) / 256) > 64 ? 4 * ((T + RX_FFTLEN) / 256) : 64;
    if ((rc = aisx_corr_create(&h->corr, tmpl, ntmpl, (float)sps, 1, 0.9f, rows, T + RX_FFTLEN, tag_cap)) != AISX_OK ||
        (rc = aisx_msk_create(&h->msk, (float)sps, 0.04f, 0.01f, 1, rows, T + RX_FFTLEN)) != AISX_OK ||
        (rc = aisx_chain_create(&h->chain, h->fs, h->agc, h->corr, h->msk, rows, T, RX_FFTLEN)) != AISX_OK)
        return rc;
    h->cap = aisx_msk_out_capacity(h->msk);
    h->rate = rate;
    h->des.assign(designators, designators + h->nch);
    h->max_dlen = max_dlen;
    if ((rc = aisx_msk_status_device(h->msk, &h->d_msk_status)) != AISX_OK)
        return rc;
    h->raw_bytes = (size_t)h->ns * h->block_items * h->item_bytes;
    for (auto& b : h->d_raw)
        if ((rc = b.alloc(h->raw_bytes, false)) != AISX_OK)
            return rc;
    for (auto& b : h->d_row)
        if ((rc = b.alloc((size_t)rows * T, false)) != AISX_OK)
            return rc;
    for (int i = 0; i < RX_NOUT; i++)
        if ((rc = h->d_bits[i].alloc((size_t)rows * h->cap, false)) != AISX_OK || (rc = h->d_prod[i].alloc((size_t)rows)) != AISX_OK)
            return rc;
    if ((rc = h->d_meta.alloc(RX_META)) != AISX_OK)
        return rc;
    for (auto& b : h->h_in)
        if ((rc = b.alloc(h->raw_bytes)) != AISX_OK)
            return rc;
    for (Stream* s : { &h->s_copy, &h->s_filt, &h->s_tail })
        if ((rc = s->create_nonblocking()) != AISX_OK)
            return rc;
    auto make = [](Event* e, int n) {
        int rc = AISX_OK;
        for (int i = 0; i < n && rc == AISX_OK; i++)
            rc = e[i].create(hipEventDisableTiming);
        return rc;
    };
    if ((rc = make(h->ev_copy, RX_NPIN)) != AISX_OK || (rc = make(h->ev_filt, RX_NRAW)) != AISX_OK ||
        (rc = make(h->ev_tail, RX_NOUT)) != AISX_OK || (rc = make(h->ev_res, RX_NRES)) != AISX_OK)
        return rc;
    return rx_make_tail(h, h->opt, "aisx_rx_create", &h->tail); // (last: it waits for the zero fills of the buffers above too)
}

extern "C" int aisx_rx_create(aisx_rx** out, double rate, int nstreams, int nchan_per_stream, const double* center_freqs,
                              const char* const* designators, int fmt, float scale, float bias, int block_items,
                              const float* taps, int ntaps, const aisx_cf32* tmpl, int ntmpl, int max_pdus_per_block)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (!(rate >= 48000.0) || !isfinite(rate) || rate / 48000.0 > XL_MAX_DECIM) {
        set_err("aisx_rx_create: the decimation is int(rate / 48000): need 48000 <= rate <= 48000 * %d", XL_MAX_DECIM);
        return AISX_ERR_INVALID;
    }
    const int D = (int)(rate / 48000.0);
    if (!xlate_fmt_ok(fmt, scale, bias)) {
        set_err("aisx_rx_create: need a format 0 .. 3 (cf32, cs16, cs8, cu8) and a finite scale and bias");
        return AISX_ERR_INVALID;
    }
    if (nstreams < 1 || nchan_per_stream < 1 || !center_freqs || !designators || !tmpl || ntmpl < 1 || max_pdus_per_block < 1 ||
        (taps && ntaps < 1) || (long long)nstreams * nchan_per_stream > (1 << 20)) {
        set_err("aisx_rx_create: need nstreams >= 1, nchan_per_stream >= 1 (at most 2^20 channels in all), centre "
                "frequencies, designators, a template and max_pdus_per_block >= 1");
        return AISX_ERR_INVALID;
    }
    if (block_items < D || block_items % D != 0) {
        set_err("aisx_rx_create: block_items (%d) must be a positive multiple of the decimation (%d)", block_items, D);
        return AISX_ERR_INVALID;
    }
    int max_dlen = 0;
    if (const int c = nm_bad_designator(designators, nchan_per_stream, &max_dlen); c >= 0) {
        set_err("aisx_rx_create: designator %d is missing or longer than %d bytes", c, NM_DESIG);
        return AISX_ERR_INVALID;
    }
    std::vector<float> own;
    if (!taps) {
        own = low_pass(rate, 11e3, 1e3);
        taps = own.data();
        ntaps = (int)own.size();
    }
    if (const char* why = XlateHost::check(D, taps, ntaps, center_freqs, nchan_per_stream, rate, nstreams, block_items)) {
        set_err("aisx_rx_create: the filter: %s", why);
        return AISX_ERR_INVALID;
    }
    int rc = require_device();
    if (rc != AISX_OK)
        return rc;
    HandlePtr<aisx_rx, aisx_rx_destroy> h(new aisx_rx());
    AISX_HIPCHK(hipGetDevice(&h->dev));
    h->fmt = fmt;
    h->item_bytes = xlate_item_bytes(fmt);
    h->scale = scale;
    h->bias = bias;
    h->ns = nstreams;
    h->nch = nchan_per_stream;
    h->D = D;
    h->block_items = block_items;
    h->T = block_items / D;
    h->max_pdus = max_pdus_per_block;
    if ((rc = rx_build(h.get(), rate, center_freqs, designators, taps, ntaps, tmpl, ntmpl, max_dlen)) != AISX_OK) {
        const std::string msg = aisx_last_error();
        h.reset(); // (destroying the stages may leave a message of its own)
        set_err("%s", msg.c_str());
        return rc;
    }
    *out = h.release();
    return AISX_OK;
}

extern "C" int aisx_rx_geometry(const aisx_rx* h, int* decim, int* items_per_block, int* nchan, int* input_slots,
                                int* result_slots, long* text_cap)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (decim)
        *decim = h->D;
    if (items_per_block)
        *items_per_block = h->T;
    if (nchan)
        *nchan = h->ns * h->nch;
    if (input_slots)
        *input_slots = RX_NPIN;
    if (result_slots)
        *result_slots = RX_NRES;
    if (text_cap)
        *text_cap = (long)h->tail.text_cap;
    return AISX_OK;
}

extern "C" int aisx_rx_acquire(aisx_rx* h, void** slot, long* stride_items)
{
    if (!h || !slot) {
        set_err("aisx_rx_acquire: need a handle and somewhere to put the slot");
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, "aisx_rx_acquire");
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const int pin = (int)(h->submitted % RX_NPIN);
    if (!h->acquired && h->submitted >= RX_NPIN)
        AISX_HIPCHK(hipEventSynchronize(h->ev_copy[pin])); // (block submitted - NPIN was copied from it)
    h->acquired = true;
    *slot = h->h_in[pin];
    if (stride_items)
        *stride_items = h->block_items;
    return AISX_OK;
}

// chain step, deframer, NMEA stage and the copy back of block k; next = block k + 1's rows or nullptr
static int rx_issue(aisx_rx* h, long long k, const cf* next)
{
    int rc;
    const RxTail& t = h->tail;
    const RxLayout& lay = t.lay;
    const int set = (int)(k % RX_NOUT), res = (int)(k % RX_NRES), rows = h->ns * h->nch, T = h->T;
    if (k >= RX_NOUT) // the deframer has read this set's bits of step k - NOUT
        AISX_HIPCHK(hipStreamWaitEvent(h->s_filt, h->ev_tail[set], 0));
    long long step = -1;
    if ((rc = aisx_chain_step(h->chain, (const aisx_cf32*)h->d_row[k % RX_NROW].get(), T, T, (const aisx_cf32*)next, T, next ? T : 0,
                              t.ml ? (aisx_cf32*)t.d_syms[set].get() : nullptr, h->d_bits[set], h->cap, h->d_prod[set], h->s_filt, &step)) != AISX_OK)
        return rc;
    if (step != k) {
        set_err("aisx_rx: the chain numbered block %lld as step %lld", k, step);
        return AISX_ERR_RUNTIME;
    }
    hipStream_t st = h->s_tail;
    if ((rc = aisx_chain_wait(h->chain, k, st, 0)) != AISX_OK)
        return rc;
    if (t.ml) { // the step's symbols -> the detector's bits and counts -> the deframer
        if ((rc = aisx_mlse_batch_process(t.ml.get(), (const aisx_cf32*)t.d_syms[set].get(), h->cap, h->d_prod[set], t.d_mbits, t.mstride,
                                          t.d_mnb, st)) != AISX_OK ||
            (rc = aisx_hdlc_batch_process(t.hd.get(), t.d_mbits, t.mstride, t.d_mnb, st)) != AISX_OK)
            return rc;
    } else if ((rc = aisx_hdlc_batch_process(t.hd.get(), h->d_bits[set], h->cap, h->d_prod[set], st)) != AISX_OK)
        return rc;
    AISX_HIPCHK(hipEventRecord(h->ev_tail[set], st));
    if (t.dd && (rc = aisx_dedup_batch_process(t.dd.get(), t.d_hd_pdus, t.d_hd_bytes, t.d_hd_count + 1, t.d_hd_count, t.d_fix, (int32_t)k, st)) != AISX_OK)
        return rc;
    if (h->opt.std_nmea && h->opt.t0 >= 0 && // the block's first item's second (a launch parameter of the stage: nothing waits)
        (rc = aisx_nmea_batch_set_time(t.nm.get(), h->opt.t0 + (long long)floor((double)k * h->block_items / h->rate))) != AISX_OK)
        return rc;
    if ((rc = aisx_nmea_batch_process(t.nm.get(), t.d_ls_pdus, t.d_hd_bytes, t.d_ls_count + 1, t.d_ls_count, st)) != AISX_OK)
        return rc;
    hipLaunchKernelGGL(k_rx_meta, dim3(1), dim3(256), 0, st, h->d_msk_status, rows, t.d_hd_count, t.d_nm_count, t.d_ml_flag,
                       t.dd ? t.d_ls_count : nullptr, h->d_meta);
    AISX_HIPCHK(hipGetLastError());
    // (the bad-input flags are this block's: cleared behind the record that took them)
    AISX_HIPCHK(hipMemsetAsync((void*)(t.d_hd_count + 2), 0, sizeof(int), st));
    AISX_HIPCHK(hipMemsetAsync((void*)(t.d_nm_count + 2), 0, sizeof(int), st));
    if (t.d_ml_flag)
        AISX_HIPCHK(hipMemsetAsync((void*)t.d_ml_flag, 0, sizeof(int), st));
    if (t.dd)
        AISX_HIPCHK(hipMemsetAsync((void*)(t.d_ls_count + 2), 0, sizeof(int), st));
    char* r = t.h_res[res];
    if (t.mg) { // the rows of the records the NMEA stage kept; its bad-input flag goes into the record's spare word
        if ((rc = aisx_msg_batch_process(t.mg.get(), t.d_ls_pdus, t.d_hd_bytes, t.d_nm_count + 1, t.d_ls_count, st)) != AISX_OK)
            return rc;
        if (t.tk && (rc = aisx_track_batch_process(t.tk.get(), t.d_mg_cols, h->max_pdus, t.d_mg_strs, t.d_ls_pdus, t.d_mg_count + 1,
                                                   (int32_t)k, st)) != AISX_OK)
            return rc;
        AISX_HIPCHK(hipMemcpyAsync(h->d_meta + 7, t.d_mg_count + 2, sizeof(int), hipMemcpyDeviceToDevice, st));
        AISX_HIPCHK(hipMemsetAsync((void*)(t.d_mg_count + 2), 0, sizeof(int), st));
        AISX_HIPCHK(hipMemcpyAsync(r + lay.cols, t.d_mg_cols, lay.strs - lay.cols, hipMemcpyDeviceToHost, st));
        AISX_HIPCHK(hipMemcpyAsync(r + lay.strs, t.d_mg_strs, (size_t)AISX_MSG_STR * h->max_pdus, hipMemcpyDeviceToHost, st));
    }
    if (t.d_ls_fix)
        AISX_HIPCHK(hipMemcpyAsync(r + lay.fix, t.d_ls_fix, sizeof(int32_t) * (size_t)h->max_pdus, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipMemcpyAsync(r, h->d_meta, sizeof(int) * RX_META, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipMemcpyAsync(r + lay.recs, t.d_nm_recs, lay.text - lay.recs, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipMemcpyAsync(r + lay.text, t.d_nm_text, (size_t)t.text_cap, hipMemcpyDeviceToHost, st));
    AISX_HIPCHK(hipEventRecord(h->ev_res[res], st));
    h->issued = k + 1;
    return AISX_OK;
}

static bool rx_results_full(const aisx_rx* h) { return h->issued - h->popped >= RX_NRES; }

extern "C" int aisx_rx_submit(aisx_rx* h, long long* block)
{
    if (!h) {
        set_err("aisx_rx_submit: need a handle");
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, "aisx_rx_submit");
    if (!h->acquired) {
        set_err("aisx_rx_submit: no slot has been acquired");
        return AISX_ERR_INVALID;
    }
    const long long b = h->submitted;
    const bool step_due = b >= 1 && h->issued < b; // block b - 1 waits for this one
    if (step_due && rx_results_full(h)) {
        set_err("aisx_rx_submit: all %d result slots wait to be popped; nothing was queued", RX_NRES);
        return AISX_ERR_OVERFLOW;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const int pin = (int)(b % RX_NPIN), raw = (int)(b % RX_NRAW), row = (int)(b % RX_NROW);
    auto queue = [&]() -> int {
        int rc;
        if (b >= RX_NRAW) // the filter call of block b - NRAW has read the raw buffer
            AISX_HIPCHK(hipStreamWaitEvent(h->s_copy, h->ev_filt[raw], 0));
        AISX_HIPCHK(hipMemcpyAsync(h->d_raw[raw], h->h_in[pin], h->raw_bytes, hipMemcpyHostToDevice, h->s_copy));
        AISX_HIPCHK(hipEventRecord(h->ev_copy[pin], h->s_copy));
        AISX_HIPCHK(hipStreamWaitEvent(h->s_filt, h->ev_copy[pin], 0));
        if (b >= RX_NROW && (rc = aisx_chain_wait_input(h->chain, b - RX_NROW, h->s_filt, 0)) != AISX_OK)
            return rc; // (the row buffer was last read by step b - NROW)
        int nout = 0;
        if ((rc = aisx_xlate_process_fmt(h->xl, h->d_raw[raw], h->fmt, h->scale, h->bias, h->block_items, h->block_items,
                                         (aisx_cf32*)h->d_row[row].get(), h->T, &nout, h->s_filt)) != AISX_OK)
            return rc;
        AISX_HIPCHK(hipEventRecord(h->ev_filt[raw], h->s_filt));
        if (nout != h->T) {
            set_err("aisx_rx: the filter gave %d items for a block of %d", nout, h->T);
            return AISX_ERR_RUNTIME;
        }
        h->submitted = b + 1;
        h->acquired = false;
        return step_due ? rx_issue(h, b - 1, h->d_row[row]) : AISX_OK;
    };
    const int rc = queue();
    if (rc != AISX_OK)
        return rx_fail(h, rc);
    if (block)
        *block = b;
    return AISX_OK;
}

extern "C" int aisx_rx_push(aisx_rx* h, const void* host_iq, long stride_items, long long* block)
{
    if (!h || !host_iq || stride_items < h->block_items) {
        set_err("aisx_rx_push: need a handle, the block and a row stride of at least block_items");
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, "aisx_rx_push");
    if (h->submitted >= 1 && h->issued < h->submitted && rx_results_full(h)) {
        set_err("aisx_rx_push: all %d result slots wait to be popped; nothing was queued", RX_NRES);
        return AISX_ERR_OVERFLOW;
    }
    void* slot = nullptr;
    int rc = aisx_rx_acquire(h, &slot, nullptr);
    if (rc != AISX_OK)
        return rc;
    const size_t row = (size_t)h->block_items * h->item_bytes;
    for (int s = 0; s < h->ns; s++)
        memcpy((char*)slot + s * row, (const char*)host_iq + (size_t)s * stride_items * h->item_bytes, row);
    return aisx_rx_submit(h, block);
}

extern "C" int aisx_rx_flush(aisx_rx* h)
{
    if (!h) {
        set_err("aisx_rx_flush: need a handle");
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, "aisx_rx_flush");
    if (h->issued >= h->submitted)
        return AISX_OK;
    if (rx_results_full(h)) {
        set_err("aisx_rx_flush: all %d result slots wait to be popped; nothing was queued", RX_NRES);
        return AISX_ERR_OVERFLOW;
    }
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const int rc = rx_issue(h, h->submitted - 1, nullptr);
    return rc != AISX_OK ? rx_fail(h, rc) : AISX_OK;
}

// aisx_rx_pop, and with cols / strs aisx_rx_pop_messages; `extra_ok`: what the caller needs beyond the shared argument rule
static int rx_pop(aisx_rx* h, const char* who, const char* need, bool extra_ok, int wait, long long* block, char* text, long text_cap,
                  long* text_len, aisx_pdu* recs, int rec_cap, int* nrecs, int32_t* cols, long col_stride, char* strs, int* status)
{
    if (!h || !block || !text_len || !nrecs || text_cap < 0 || rec_cap < 0 || (text_cap > 0 && !text) || (rec_cap > 0 && !recs) || !extra_ok) {
        set_err("%s: need a handle, outputs for the block number and the counts, %s", who, need);
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, who);
    *block = -1;
    *text_len = 0;
    *nrecs = 0;
    if (status)
        *status = 0;
    if (h->popped >= h->issued)
        return AISX_OK;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    const int res = (int)(h->popped % RX_NRES);
    if (!wait) {
        const hipError_t e = hipEventQuery(h->ev_res[res]);
        if (e == hipErrorNotReady)
            return AISX_OK;
        AISX_HIPCHK(e);
    } else {
        const hipError_t e = hipEventSynchronize(h->ev_res[res]);
        if (e != hipSuccess) {
            set_err("%s: waiting for block %lld failed: %s", who, h->popped, hipGetErrorString(e));
            return rx_fail(h, AISX_ERR_HIP);
        }
    }
    const RxLayout& lay = h->tail.lay;
    const char* r = h->tail.h_res[res];
    const int* meta = (const int*)r;
    const aisx_pdu* rr = (const aisx_pdu*)(r + lay.recs);
    int k = meta[5]; // records the NMEA stage wrote
    if (k < 0 || k > h->max_pdus)
        k = 0;
    const long long nt = k > 0 ? rr[k - 1].offset + rr[k - 1].len + (rr[k - 1].len > 0 ? 1 : 0) : 0;
    *nrecs = k;
    *text_len = (long)nt;
    if (k > rec_cap || nt > text_cap) {
        set_err("%s: block %lld has %d records and %lld bytes of text; the buffers hold %d and %ld", who, h->popped, k, nt,
                rec_cap, text_cap);
        return AISX_ERR_OVERFLOW;
    }
    if (k > 0)
        memcpy(recs, rr, sizeof(aisx_pdu) * (size_t)k);
    if (nt > 0)
        memcpy(text, r + lay.text, (size_t)nt);
    if (cols && k > 0) {
        const int32_t* cc = (const int32_t*)(r + lay.cols);
        for (int c = 0; c < AISX_MSG_NCOL; c++)
            memcpy(cols + (size_t)c * col_stride, cc + (size_t)c * h->max_pdus, sizeof(int32_t) * (size_t)k);
        memcpy(strs, r + lay.strs, (size_t)AISX_MSG_STR * k);
    }
    if (h->tail.d_fix) // (the NMEA stage's records are the first k of the list it read: the deframer's, or the kept ones)
        h->popped_fix.assign((const int32_t*)(r + lay.fix), (const int32_t*)(r + lay.fix) + k);
    if (status)
        *status = meta[0] | (meta[1] > meta[2] ? AISX_RX_ST_HDLC_OVERFLOW : 0) | (meta[5] < (h->tail.dd ? meta[8 + AISX_DEDUP_CNT_KEPT] : meta[2]) ? AISX_RX_ST_NMEA_OVERFLOW : 0) |
                  ((meta[3] || meta[6] || meta[7]) ? AISX_RX_ST_BAD_COUNT : 0);
    memcpy(h->popped_dd, meta + 8, sizeof h->popped_dd);
    *block = h->popped++;
    return AISX_OK;
}

extern "C" int aisx_rx_pop(aisx_rx* h, int wait, long long* block, char* text, long text_cap, long* text_len, aisx_pdu* recs,
                           int rec_cap, int* nrecs, int* status)
{
    return rx_pop(h, "aisx_rx_pop", "and buffers for their capacities", true, wait, block, text, text_cap, text_len, recs, rec_cap, nrecs,
                  nullptr, 0, nullptr, status);
}

extern "C" int aisx_rx_pop_messages(aisx_rx* h, int wait, long long* block, char* text, long text_cap, long* text_len, aisx_pdu* recs,
                                    int rec_cap, int* nrecs, int32_t* cols, long col_stride, char* strs, int* status)
{
    if (h && !h->tail.mg) {
        set_err("aisx_rx_pop_messages: aisx_rx_enable_messages was not called on this handle");
        return AISX_ERR_INVALID;
    }
    return rx_pop(h, "aisx_rx_pop_messages", "buffers for their capacities and a table of rec_cap rows (col_stride >= rec_cap)",
                  (rec_cap <= 0 || (cols && strs)) && col_stride >= rec_cap, wait, block, text, text_cap, text_len, recs, rec_cap, nrecs,
                  rec_cap > 0 ? cols : nullptr, col_stride, strs, status);
}

// What every aisx_rx_enable_* is: `change` puts the call's wish into a copy of the options (or refuses its arguments
// with a message), and the tail those ask for is made beside the one in use, which it replaces only when all of it
// exists.  Until then the handle stays as it was.  `refused`: the call's own rule says no; `rule` words that rule.
template <class Change>
static int rx_reconfigure(aisx_rx* h, const char* who, bool refused, const char* rule, Change change)
{
    if (!h) {
        set_err("%s: need a handle", who);
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, who);
    if (refused || h->acquired || h->submitted > 0) {
        set_err("%s: %sonly before the first acquire, submit or push", who, rule);
        return AISX_ERR_INVALID;
    }
    RxOptions opt = h->opt;
    int rc = change(opt);
    if (rc != AISX_OK)
        return rc;
    OnDevice on(h->dev);
    AISX_HIPCHK(on.err);
    RxTail tail;
    if ((rc = rx_make_tail(h, opt, who, &tail)) != AISX_OK) { // (what is released on the way out must not replace the message)
        const std::string msg = aisx_last_error();
        tail = RxTail();
        set_err("%s", msg.c_str());
        return rc;
    }
    h->tail = std::move(tail);
    h->opt = std::move(opt);
    return AISX_OK;
}

extern "C" int aisx_rx_enable_messages(aisx_rx* h)
{
    if (h && h->failed == AISX_OK && h->opt.messages)
        return AISX_OK;
    return rx_reconfigure(h, "aisx_rx_enable_messages", false, "", [](RxOptions& o) {
        o.messages = true;
        return AISX_OK;
    });
}

extern "C" int aisx_rx_enable_standard_nmea(aisx_rx* h, const char* const* stations, int64_t t0)
{
    return rx_reconfigure(h, "aisx_rx_enable_standard_nmea", h && h->opt.std_nmea, "once, and ", [&](RxOptions& o) {
        o.t0 = t0 < 0 ? -1 : t0;
        if (const int s = nms_bad_station(stations, h->ns); s >= 0 || !nms_time_ok(o.t0)) {
            set_err("aisx_rx_enable_standard_nmea: stations of 0..%d bytes of A-Z a-z 0-9 _ - (station %d is none) and t0 < 10^18", NMS_STATION, s);
            return AISX_ERR_INVALID;
        }
        o.std_nmea = true;
        o.stations.assign((size_t)h->ns, std::string());
        for (int s = 0; stations && s < h->ns; s++)
            o.stations[s] = stations[s];
        return AISX_OK;
    });
}

extern "C" int aisx_rx_enable_repair(aisx_rx* h, const aisx_hdlc_rule* rules, int nrules)
{
    return aisx_rx_enable_repair_events(h, rules, nrules, AISX_HDLC_EV_SINGLE);
}

extern "C" int aisx_rx_enable_repair_events(aisx_rx* h, const aisx_hdlc_rule* rules, int nrules, int events)
{
    return rx_reconfigure(h, "aisx_rx_enable_repair", nrules < 1 || !rules, "at least one rule, and ", [&](RxOptions& o) {
        // (at most one rule more than a deframer takes: it is the deframer that judges rules and mask)
        o.rules.assign(rules, rules + std::min(nrules, AISX_HDLC_MAX_RULES + 1));
        o.events = events;
        return AISX_OK;
    });
}

extern "C" int aisx_rx_enable_mlse(aisx_rx* h, double bt)
{
    return rx_reconfigure(h, "aisx_rx_enable_mlse", h && h->opt.detector, "once, and ", [&](RxOptions& o) {
        o.detector = true;
        o.bt = bt;
        return AISX_OK;
    });
}

extern "C" int aisx_rx_enable_tracks(aisx_rx* h, int capacity)
{
    return rx_reconfigure(h, "aisx_rx_enable_tracks", h && h->opt.tracks, "once, and ", [&](RxOptions& o) {
        o.tracks = o.messages = true;
        o.capacity = capacity;
        return AISX_OK;
    });
}

extern "C" int aisx_rx_enable_dedup(aisx_rx* h, int window)
{
    return rx_reconfigure(h, "aisx_rx_enable_dedup", h && h->opt.dedup, "once, and ", [&](RxOptions& o) {
        o.dedup = true;
        o.window = window;
        return AISX_OK;
    });
}

extern "C" int aisx_rx_popped_dedup(aisx_rx* h, int* counts)
{
    if (!h || !h->tail.dd || !counts) {
        set_err("aisx_rx_popped_dedup: need a handle on which aisx_rx_enable_dedup was called and somewhere to put the counts");
        return AISX_ERR_INVALID;
    }
    memcpy(counts, h->popped_dd, sizeof h->popped_dd);
    return AISX_OK;
}

extern "C" int aisx_rx_popped_repairs(aisx_rx* h, int32_t* fix_bits, int cap, int* n)
{
    if (!h || !h->tail.d_fix || !n || cap < 0 || (cap > 0 && !fix_bits)) {
        set_err("aisx_rx_popped_repairs: need a handle on which aisx_rx_enable_repair was called, a count and a buffer for its capacity");
        return AISX_ERR_INVALID;
    }
    const int have = (int)h->popped_fix.size(), k = have < cap ? have : cap;
    *n = have;
    if (k > 0)
        memcpy(fix_bits, h->popped_fix.data(), sizeof(int32_t) * (size_t)k);
    if (k < have) {
        set_err("aisx_rx_popped_repairs: the block has %d records, the buffer holds %d", have, cap);
        return AISX_ERR_OVERFLOW;
    }
    return AISX_OK;
}

// the two reads of the table, on the tail stream: behind the update of every block issued so far
static int rx_tracks_ready(aisx_rx* h, const char* who, long long* block)
{
    if (!h || !h->tail.tk) {
        set_err("%s: need a handle on which aisx_rx_enable_tracks was called", who);
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, who);
    if (block)
        *block = h->issued - 1;
    return AISX_OK;
}

extern "C" int aisx_rx_read_tracks(aisx_rx* h, int first, int n, int32_t* cols, long col_stride, char* strs, int* nvessels,
                                   long long* block)
{
    const int rc = rx_tracks_ready(h, "aisx_rx_read_tracks", block);
    return rc != AISX_OK ? rc : aisx_track_batch_read(h->tail.tk.get(), first, n, cols, col_stride, strs, nvessels, (hipStream_t)h->s_tail);
}

extern "C" int aisx_rx_read_changed_tracks(aisx_rx* h, int* idx, int32_t* cols, long col_stride, char* strs, int cap, int* nchanged,
                                           long long* block)
{
    const int rc = rx_tracks_ready(h, "aisx_rx_read_changed_tracks", block);
    return rc != AISX_OK ? rc : aisx_track_batch_read_changed(h->tail.tk.get(), idx, cols, col_stride, strs, cap, nchanged, (hipStream_t)h->s_tail);
}

extern "C" int aisx_rx_set_center_freq(aisx_rx* h, int stream, int chan, double center_freq)
{
    if (!h) {
        set_err("aisx_rx_set_center_freq: need a handle");
        return AISX_ERR_INVALID;
    }
    if (h->failed != AISX_OK)
        return rx_failed(h, "aisx_rx_set_center_freq");
    return aisx_xlate_set_center_freq(h->xl, stream, chan, center_freq);
}
