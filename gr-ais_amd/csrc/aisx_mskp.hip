// aisx_mskp.hip -- the time-parallel timing recovery (k_mskp.h; aisx_msk_set_time_parallel): its __global__ wrappers,
// what it keeps in the handle, and the prepass / units / join / gather of a stream call, which aisx_msk.hip's
// msk_process_stream queues around its own steps.  Off unless asked for; the join build of the serial kernel
// (k_msk_ff) stays with k_msk in aisx_msk.hip and is reached through msk_launch.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "aisx_devctx.h"
#include "aisx_msk_impl.h"
#include "k_mskp.h"

using namespace aisx;

__global__ __launch_bounds__(64) void k_mskp_prep(MskpPrepParams p)
{
    __shared__ __attribute__((aligned(16))) char smem[MSKP_PREP_LDS_TAGS * 8];
    DevCtx cx{ smem };
    mskp_prep_body(cx, p);
}
__global__ __launch_bounds__(64) void k_mskp_units(MskpParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DevCtx cx{ smem };
    mskp_body<DevCtx, false>(cx, p);
}
__global__ __launch_bounds__(64) void k_mskp_join(MskpParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DevCtx cx{ smem };
    // one lane per channel, a recurrence: its waves go first on their SIMDs
    __builtin_amdgcn_s_setprio(3);
    mskp_body<DevCtx, true>(cx, p);
}
__global__ __launch_bounds__(256) void k_mskp_gather(MskpGatherParams p)
{
    DevCtx cx{ nullptr };
    mskp_gather_body(cx, p);
}

// The tunables, and everything the path allocates on its first call (and nothing before): set up = s_units exists;
// without it the handle is as if the path had never run.
struct aisx::MskTp {
    struct Knobs {
        int smax = 0;        // restart points per channel at most; 0 = off, the serial kernel alone
        int min_gap = 64;    // items between restart points at least
        int jw = 16;         // channels per wave of the join kernel
        int join = 1;        // the join: 1 = the serial kernel with fast-forward (k_msk.h, MskParams::ff), 0 = k_mskp_join
        int max_span = 4096; // no unit from a restart point further than this from the next one (join = 1: the serial kernel is faster there)
        bool one_stream = false, unsorted = false; // (experiments: units on the call's stream; unsorted unit list)
    } k;
    // the units run on a stream of their own, one call ahead of the join (which needs the previous call's
    // state): everything the prepass and the units leave for the join exists twice, by the call's parity
    Stream s_units;
    Event ev_entry, ev_units[2], ev_join[2];
    bool ev_join_set[2] = { false, false };
    DevBuf<msk_ctag> d_ctl; // 2 x nchan x ctl_cap
    int ctl_cap = 0;
    DevBuf<int> d_ctl_n, d_nrst;
    DevBuf<mskp_rst> d_rst;
    DevBuf<mskp_res> d_res;
    DevBuf<int> d_ct_nc;
    DevBuf<cf> d_stage[2];
    long stage_stride = 0;
    DevBuf<int> d_ucount; // units per length class
    DevBuf<int> d_ulist;  // ... and which
    DevBuf<mskp_piece> d_pieces[2];
    DevBuf<int> d_npieces[2];
    long tp_calls = 0;
    // parity `par`'s copies of what the prepass and the units leave for the join
    size_t nc = 0; // channels
    msk_ctag* ctl(int par) const { return d_ctl + (size_t)par * nc * (size_t)ctl_cap; }
    int* ctl_n(int par) const { return d_ctl_n + par * nc; }
    int* nrst(int par) const { return d_nrst + par * nc; }
    mskp_rst* rst(int par) const { return d_rst + par * nc * MSKP_SMAX; }
    mskp_res* res(int par) const { return d_res + par * nc * MSKP_SMAX; }
    int* ucount(int par) const { return d_ucount + par * 8; }
    int* ulist(int par) const { return d_ulist + par * nc * MSKP_SMAX * MSKP_NCLS; }
    ~MskTp()
    {
        if (s_units) // the units' stream comes to rest before anything it uses is released
            (void)hipStreamSynchronize(s_units);
    }
};
void aisx::MskTpDelete::operator()(MskTp* t) const { delete t; }

void aisx::msk_tp_create(aisx_msk* h)
{
    h->tp.reset(new MskTp());
    MskTp::Knobs& k = h->tp->k;
    if (const char* e = exp_env("AISX_MSK_TIME_PARALLEL")) // (experiments; the API is aisx_msk_set_time_parallel)
        k.smax = atoi(e) != 0 ? MSKP_SMAX : 0;
    if (const char* e = exp_env("AISX_MSK_TP_SMAX")) // restart points per channel (0: the serial kernel)
        k.smax = std::max(0, std::min(atoi(e), (int)MSKP_SMAX));
    if (const char* e = exp_env("AISX_MSK_TP_GAP"))
        k.min_gap = std::max(0, atoi(e));
    if (const char* e = exp_env("AISX_MSK_TP_JOIN"))
        k.join = atoi(e) != 0;
    if (const char* e = exp_env("AISX_MSK_TP_MAXSPAN"))
        k.max_span = std::max(64, atoi(e));
    if (const char* e = exp_env("AISX_MSK_JW"))
        k.jw = std::max(1, std::min(64, atoi(e)));
    k.one_stream = exp_env("AISX_MSK_TP_ONE_STREAM") != nullptr;
    k.unsorted = exp_env("AISX_MSK_TP_UNSORTED") != nullptr;
}

extern "C" int aisx_msk_set_time_parallel(aisx_msk* h, int restart_points_per_channel, int join_kernel, int max_unit_items)
{
    if (!h || restart_points_per_channel < 0)
        return AISX_ERR_INVALID;
    MskTp::Knobs& k = h->tp->k;
    k.smax = std::min(restart_points_per_channel, (int)MSKP_SMAX);
    if (join_kernel >= 0)
        k.join = join_kernel != 0;
    if (max_unit_items > 0)
        k.max_span = std::max(64, max_unit_items);
    return AISX_OK;
}

bool aisx::msk_tp_applies(const aisx_msk* h, const float* d_err, const float* d_mu)
{
    // (osps = 2 and the err / mu ports stay with the serial kernel: after a restart the first err
    // of a unit would need the previous unit's last nlin_out)
    return h->tp->k.smax > 0 && h->osps == 1 && !d_err && !d_mu &&
           mskp_geometry_ok(h->d_sps, h->gain, h->limit, h->max_items + aisx_msk::carry_cap);
}

static int msk_tp_buffers(aisx_msk* h, int tag_cap, hipStream_t st)
{
    int rc;
    const size_t nc = (size_t)h->nchan;
    const int need = MSKP_TPRE + tag_cap + 1;
    const bool set_up = (bool)h->tp->s_units;
    if (set_up && need <= h->tp->ctl_cap)
        return AISX_OK;
    AISX_HIPCHK(hipStreamSynchronize(st));
    if (!set_up) {
        // (all or nothing: a failed allocation half way leaves a handle on which the path never ran)
        std::unique_ptr<MskTp, MskTpDelete> t(new MskTp());
        t->k = h->tp->k;
        t->nc = nc;
        t->stage_stride = mskp_stage_stride(h->max_items + aisx_msk::carry_cap, h->d_sps, h->gain, h->limit);
        if ((rc = t->d_ctl.alloc(2 * nc * (size_t)need)) != AISX_OK || (rc = t->d_ctl_n.alloc(2 * nc)) != AISX_OK ||
            (rc = t->d_nrst.alloc(2 * nc)) != AISX_OK || (rc = t->d_rst.alloc(2 * nc * MSKP_SMAX)) != AISX_OK ||
            (rc = t->d_res.alloc(2 * nc * MSKP_SMAX)) != AISX_OK || (rc = t->d_ucount.alloc(16)) != AISX_OK ||
            (rc = t->d_ct_nc.alloc(nc)) != AISX_OK || (rc = t->d_ulist.alloc(2 * nc * MSKP_SMAX * MSKP_NCLS)) != AISX_OK ||
            (rc = t->s_units.create_nonblocking()) != AISX_OK || (rc = t->ev_entry.create(hipEventDisableTiming)) != AISX_OK)
            return rc;
        for (int k = 0; k < 2; k++)
            if ((rc = t->ev_units[k].create(hipEventDisableTiming)) != AISX_OK || (rc = t->ev_join[k].create(hipEventDisableTiming)) != AISX_OK ||
                (rc = t->d_stage[k].alloc(nc * (size_t)t->stage_stride)) != AISX_OK ||
                (rc = t->d_pieces[k].alloc(nc * MSKP_SMAX)) != AISX_OK || (rc = t->d_npieces[k].alloc(nc)) != AISX_OK)
                return rc;
        t->ctl_cap = need;
        h->tp = std::move(t);
    } else {
        AISX_HIPCHK(hipStreamSynchronize(h->tp->s_units));
        h->tp->ctl_cap = 0; // (until the new list exists)
        if ((rc = h->tp->d_ctl.alloc(2 * nc * (size_t)need)) != AISX_OK)
            return rc;
        h->tp->ctl_cap = need;
    }
    // dev_alloc's zero fill runs on the null stream: it must not trail into the kernels on `st`
    AISX_HIPCHK(hipDeviceSynchronize());
    return AISX_OK;
}

// where the prepass and the units of a call on `st` run
static hipStream_t tp_units_stream(const MskTp* T, hipStream_t st) { return T->k.one_stream ? st : (hipStream_t)T->s_units; }
// units sorted by length need every row within 4 GiB of the first (32-bit buffer offsets)
static bool tp_sorted(const aisx_msk* h, long in_stride)
{
    return (double)h->nchan * (double)in_stride * 8.0 < 4294000000.0 && !h->tp->k.unsorted;
}
// (units run blind to the general_work calls: with a max_noutput_items the call boundaries must
// leave an un-blocked loop alone, which needs d_sps >= 2 -- see mskp_body's walk)
static int tp_prep_smax(const aisx_msk* h) { return (h->max_noutput > 0 && h->d_sps < 2.0f) ? 0 : h->tp->k.smax; }

int aisx::msk_tp_prepass(aisx_msk* h, const MskCall& c, hipStream_t* ran_on)
{
    int rc;
    if ((rc = msk_tp_buffers(h, c.tags ? c.tag_cap : 0, c.st)) != AISX_OK)
        return rc;
    MskTp* T = h->tp.get();
    // The units need the samples and the tags of this call, nothing of the call before: they run
    // on their own stream, beside the join of the previous call.  They start when the caller says
    // the inputs are there (ready_event; without one: when `stream` gets here), when the join of
    // two calls ago has let go of this parity's records and the bit tail of its staging rows.
    const hipStream_t su = *ran_on = tp_units_stream(T, c.st);
    if (su != c.st) {
        if (c.ready_event) {
            AISX_HIPCHK(hipStreamWaitEvent(su, (hipEvent_t)c.ready_event, 0));
        } else {
            AISX_HIPCHK(hipEventRecord(T->ev_entry, c.st));
            AISX_HIPCHK(hipStreamWaitEvent(su, T->ev_entry, 0));
        }
        if (T->ev_join_set[c.par])
            AISX_HIPCHK(hipStreamWaitEvent(su, T->ev_join[c.par], 0));
    }
    if (h->tail_on && h->ev_tail_set[c.par])
        AISX_HIPCHK(hipStreamWaitEvent(su, h->ev_tail[c.par], 0));
    MskpPrepParams t;
    t.nchan = h->nchan;
    t.tags = c.tags;
    t.tag_count = c.tag_counts;
    t.tag_cap = c.tag_cap;
    t.W = h->total_in;
    t.n = c.n;
    t.d_sps = h->d_sps;
    t.gain = h->gain;
    t.limit = h->limit;
    t.ctl = T->ctl(c.par);
    t.ctl_n = T->ctl_n(c.par);
    t.ctl_cap = T->ctl_cap;
    t.smax = tp_prep_smax(h);
    t.nrst = T->nrst(c.par);
    t.rst = T->rst(c.par);
    t.stage_stride = T->stage_stride;
    t.tail = mskp_tail(h->d_sps);
    t.min_gap = T->k.min_gap;
    t.max_span = T->k.join ? T->k.max_span : 0x3fffffff;
    const bool sorted = tp_sorted(h, c.in_stride);
    t.ucount = sorted ? T->ucount(c.par) : nullptr;
    t.ulist = T->ulist(c.par);
    t.ucap = (long)h->nchan * MSKP_SMAX;
    if (sorted)
        AISX_HIPCHK(hipMemsetAsync(T->ucount(c.par), 0, sizeof(int) * 8, su));
    hipLaunchKernelGGL(k_mskp_prep, dim3(h->nchan), dim3(64), 0, su, t);
    AISX_HIPCHK(hipGetLastError());
    return AISX_OK;
}

// the serial kernel as the join: the loop from the carried state, fast-forwarded through the units;
// its tag list = the tags the scheduler still held + this call's, as the prepass compacted them
static int tp_join_serial(aisx_msk* h, const MskCall& c)
{
    MskTp* T = h->tp.get();
    int rc;
    if ((rc = msk_launch_tagprep(h, nullptr, nullptr, 0, c.st, T->d_ct_nc, T->ctl(c.par), T->ctl_n(c.par), T->ctl_cap, MSKP_TPRE)) != AISX_OK)
        return rc;
    MskParams m;
    msk_fill_common(h, m);
    msk_fill_call(c, m);
    m.err = nullptr;
    m.mu_out = nullptr;
    m.sym_al16 = 0; // (behind a fast-forward a channel's symbol count may be odd)
    m.inline_tags = 0; // (every tag reset through the general step, where the junctions are looked at)
    m.ff = 1;
    m.nrst = T->nrst(c.par);
    m.rst = T->rst(c.par);
    m.res = T->res(c.par);
    m.pieces = T->d_pieces[c.par];
    m.npieces = T->d_npieces[c.par];
    m.ct_nc = T->d_ct_nc;
    return msk_launch(m, (h->nchan + msk_wg_channels(h->lpw) - 1) / msk_wg_channels(h->lpw), c.st);
}

int aisx::msk_tp_units_join(aisx_msk* h, const MskCall& c)
{
    MskTp* T = h->tp.get();
    const hipStream_t su = tp_units_stream(T, c.st);
    const bool sorted = tp_sorted(h, c.in_stride);
    int rc;
    MskpParams p;
    msk_fill_state(h, p);
    msk_fill_call(c, p);
    p.ctag_in = h->d_ctag[h->cur];
    p.ctag_n_in = h->d_ctag_n[h->cur];
    p.ctl = T->ctl(c.par);
    p.ctl_n = T->ctl_n(c.par);
    p.ctl_cap = T->ctl_cap;
    p.smax = T->k.smax;
    p.nrst = T->nrst(c.par);
    p.rst = T->rst(c.par);
    p.res = T->res(c.par);
    p.stage = T->d_stage[c.par];
    p.stage_stride = T->stage_stride;
    p.pieces = T->d_pieces[c.par];
    p.npieces = T->d_npieces[c.par];
    p.W = h->total_in;
    p.look = mskp_look(h->d_sps, h->limit);
    p.padv = mskp_padv(h->d_sps, h->gain, h->limit);
    p.padv_inv = mskp_padv_inv(h->d_sps, h->gain, h->limit);
    p.jw = T->k.jw;
    p.ucount = sorted ? T->ucount(c.par) : nullptr;
    p.ulist = T->ulist(c.par);
    p.ucap = (long)h->nchan * MSKP_SMAX;
    p.tail = mskp_tail(h->d_sps);
    if ((rc = ensure_dyn_lds((const void*)k_mskp_units, MSKP_LDS_BYTES, "msk_timing_recovery_cc: the restart units")) != AISX_OK ||
        (rc = ensure_dyn_lds((const void*)k_mskp_join, MSKP_LDS_BYTES, "msk_timing_recovery_cc: the join")) != AISX_OK)
        return rc;
    if (tp_prep_smax(h) > 0) {
        const long units = (long)h->nchan * T->k.smax;
        hipLaunchKernelGGL(k_mskp_units, dim3((unsigned)((units + 63) / 64 + (sorted ? MSKP_NCLS : 0))), dim3(64), MSKP_LDS_BYTES, su, p);
        AISX_HIPCHK(hipGetLastError());
    }
    if (su != c.st) { // the join, on the caller's stream, behind the units
        AISX_HIPCHK(hipEventRecord(T->ev_units[c.par], su));
        AISX_HIPCHK(hipStreamWaitEvent(c.st, T->ev_units[c.par], 0));
    }
    if (T->k.join) {
        if ((rc = tp_join_serial(h, c)) != AISX_OK)
            return rc;
    } else {
        hipLaunchKernelGGL(k_mskp_join, dim3((h->nchan + T->k.jw - 1) / T->k.jw), dim3(64), MSKP_LDS_BYTES, c.st, p);
        AISX_HIPCHK(hipGetLastError());
    }
    if (su != c.st) {
        AISX_HIPCHK(hipEventRecord(T->ev_join[c.par], c.st));
        T->ev_join_set[c.par] = true;
    }
    T->tp_calls++;
    return AISX_OK;
}

int aisx::msk_tp_gather(aisx_msk* h, const MskCall& c, bool on_tail)
{
    MskTp* T = h->tp.get();
    MskpGatherParams g;
    g.nchan = h->nchan;
    g.pieces = T->d_pieces[c.par];
    g.npieces = T->d_npieces[c.par];
    g.stage = T->d_stage[c.par];
    g.stage_stride = T->stage_stride;
    g.syms = c.syms;
    g.out_stride = c.out_stride;
    hipLaunchKernelGGL(k_mskp_gather, dim3(MSKP_GATHER_X, h->nchan), dim3(256), 0, on_tail ? h->tail_stream : c.st, g);
    AISX_HIPCHK(hipGetLastError());
    // On the call's stream the gather reads d_stage[par] / d_res[par], which the units of the call after next
    // overwrite on their own stream: they wait for ev_join[par], so it has to stand BEHIND the gather (without a
    // bit tail on another stream nothing else orders the two)
    if (!on_tail && T->ev_join_set[c.par])
        AISX_HIPCHK(hipEventRecord(T->ev_join[c.par], c.st));
    return AISX_OK;
}

// what the time-parallel path made of the last call (diagnostics; waits for `stream`)
extern "C" int aisx_msk_restart_stats(aisx_msk* h, long long* out10, void* stream)
{
    if (!h || !out10)
        return AISX_ERR_INVALID;
    for (int i = 0; i < 10; i++) // (ten entries: include/aisx.h)
        out10[i] = 0;
    const MskTp* T = h->tp.get();
    if (T->tp_calls == 0) // (the path never ran on this handle)
        return AISX_OK;
    out10[5] = T->tp_calls;
    const int par = h->callpar ^ 1; // the call before this one
    const size_t nc = (size_t)h->nchan;
    std::vector<int> nrst(nc), np(nc);
    std::vector<mskp_piece> pc(nc * MSKP_SMAX);
    std::vector<mskp_res> rs(nc * MSKP_SMAX);
    std::vector<mskp_rst> rp(nc * MSKP_SMAX);
    AISX_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    // (a pipelined caller's join runs on a stream of its own: its records are complete behind ev_join)
    if (T->ev_join_set[par])
        AISX_HIPCHK(hipEventSynchronize(T->ev_join[par]));
    AISX_HIPCHK(hipMemcpy(nrst.data(), T->nrst(par), sizeof(int) * nc, hipMemcpyDeviceToHost));
    AISX_HIPCHK(hipMemcpy(np.data(), T->d_npieces[par], sizeof(int) * nc, hipMemcpyDeviceToHost));
    AISX_HIPCHK(hipMemcpy(pc.data(), T->d_pieces[par], sizeof(mskp_piece) * pc.size(), hipMemcpyDeviceToHost));
    AISX_HIPCHK(hipMemcpy(rs.data(), T->res(par), sizeof(mskp_res) * rs.size(), hipMemcpyDeviceToHost));
    AISX_HIPCHK(hipMemcpy(rp.data(), T->rst(par), sizeof(mskp_rst) * rp.size(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < nc; c++) {
        out10[0] += nrst[c];                     // restart points chosen
        out10[1] += np[c];                       // units whose run was taken over
        for (int i = 0; i < np[c]; i++)
            out10[2] += pc[c * MSKP_SMAX + i].cnt; // symbols that came from units
        for (int i = 0; i < nrst[c]; i++) {
            out10[3] += rs[c * MSKP_SMAX + i].kind == MSKP_KIND_NEXT;    // units that ended at the next restart point
            out10[4] += rs[c * MSKP_SMAX + i].kind == MSKP_KIND_HANDOFF; // ... somewhere else (stale tag, end of the row)
            const long long span = rs[c * MSKP_SMAX + i].end.a - rp[c * MSKP_SMAX + i].relA;
            out10[8] = std::max(out10[8], span); // longest unit, items
            out10[9] += span;
            // links: a unit that ended at the next restart point with exactly the delay registers that one assumed
            if (i + 1 < nrst[c] && rs[c * MSKP_SMAX + i].kind == MSKP_KIND_NEXT) {
                const mskp_res &a = rs[c * MSKP_SMAX + i], &b = rs[c * MSKP_SMAX + i + 1];
                out10[6] += mskp_same_bits(a.end.y, b.ay) && mskp_same_bits(a.end.nl, b.anl);
                out10[7] += 1;
            }
        }
    }
    return AISX_OK;
}
