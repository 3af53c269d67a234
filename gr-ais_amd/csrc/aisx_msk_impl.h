// aisx_msk_impl.h -- the msk_timing_recovery_cc handle and what its two translation units share: aisx_msk.hip (the
// serial kernel, the bit tail, the C ABI) and aisx_mskp.hip (the time-parallel recovery).  Needs k_msk.h alone.
#pragma once
#include <memory>
#include <vector>

#include "aisx_host.h"
#include "k_msk.h"

#pragma GCC visibility push(hidden)
namespace aisx {
struct MskTp; // the time-parallel recovery's tunables and, from its first call on, its resources (aisx_mskp.hip)
struct MskTpDelete {
    void operator()(MskTp* t) const;
};
} // namespace aisx

struct aisx_msk {
    int nchan = 0, max_items = 0, out_cap = 0, osps = 1;
    // measurement hook (aisx_msk_set_profiling): hipEvents around the recovery kernel of every stream call
    aisx::EventRing prof;
    int lpw = 64; // channels per wave of the timing-recovery kernel
    int inline_tags = 1; // (AISX_MSK_INLINE_TAGS=0: every tag reset through the general steps, for A/B runs)
    float d_sps = 0, gain = 0, gain_omega = 0, limit = 0;
    static constexpr int carry_cap = aisx::MSK_CARRY_MAX, ctag_cap = 64;
    aisx::DevBuf<float> d_mu, d_omega;
    aisx::DevBuf<int> d_div;
    aisx::DevBuf<aisx::cf> d_dly1, d_dly2, d_diff1;
    // bit tail state (previous symbol, previous sliced bit): read from [tcur], written to [tcur ^ 1]
    aisx::DevBuf<aisx::cf> d_tprev[2];
    aisx::DevBuf<unsigned char> d_tbit[2];
    int tcur = 0;
    // symbols for the bit tail when the caller takes bits only; two, alternating, so that the
    // bit tail of call k may still read one while call k+1 writes the other (tail stream)
    aisx::DevBuf<aisx::cf> d_symscratch[2];
    int callpar = 0;
    // optional: the bit tail on a stream of its own (aisx_msk_set_tail_stream)
    bool tail_on = false;
    hipStream_t tail_stream = nullptr; // the caller's
    aisx::Event ev_msk, ev_tail[2];
    unsigned head_start_ticks = 0; // aisx_msk_set_head_start
    aisx::Event ev_prep; // behind the tag prepass of the last aisx_msk_process_stream (aisx_msk_wait_prepass)
    bool ev_prep_set = false;
    bool ev_tail_set[2] = { false, false };
    // The bit tail inside the recovery kernel's symbol flush (aisx_msk_set_fused_tail; k_msk.h, MskParams::bits) where the
    // call allows it: no second kernel, no symbol scratch, nothing on the tail stream.  last_fused / last_st: whether the
    // last call with d_bits took that path, and its stream (where its bits are complete); tail_pend[par]: a bit tail is
    // queued on the tail stream that no later call on the recovery's stream has waited for yet.
    bool fused_tail = true, last_fused = false;
    int pair_core = 1; // aisx_msk_set_pair_core: 1 = the hand-scheduled lock-step pair where a build has it, 0 = the compiler's
    hipStream_t last_st = nullptr;
    bool tail_pend[2] = { false, false };
    aisx::DevBuf<int> d_produced2; // second internal `produced` array (alternates with d_produced)
    aisx::DevBuf<unsigned long long> d_nread;
    aisx::DevBuf<aisx::cf> d_carry[2];
    aisx::DevBuf<int> d_carry_len[2];
    aisx::DevBuf<aisx::tag_rec> d_ctag[2];
    aisx::DevBuf<int> d_ctag_n[2];
    aisx::DevBuf<aisx::msk_ctag> d_ct; // this call's time_est tags, compacted (k_msk_tagprep): nchan x ct_cap()
    aisx::DevBuf<int> d_ct_n;
    int ct_cap() const { return (int)(d_ct.cap() / (size_t)nchan); }
    int cur = 0;
    aisx::DevBuf<int> d_produced, d_consumed, d_status;
    aisx::DevBuf<float> d_mmse, d_atan;
    int max_noutput = 0;   // set_max_noutput_items(): output items one general_work call is offered at most (0: what fits)
    unsigned long long total_in = 0; // items handed to the block so far = absolute offset of the next row's item 0
    // GNU Radio path staging
    aisx::DevBuf<aisx::cf> d_st_in, d_st_blk;
    aisx::cf* d_st_sym = nullptr; // (= d_st_blk + 2: the symbols behind their 16-byte header)
    std::vector<aisx::cf> st_host; // where header + symbols land on the host
    aisx::DevBuf<float> d_st_err, d_st_mu;
    aisx::DevBuf<unsigned char> d_st_bits;
    aisx::DevBuf<aisx::tag_rec> d_st_tags;
    aisx::DevBuf<int> d_st_tagn;
    // the time-parallel recovery (msk_tp_create); last, so that its stream has come to rest before any buffer above goes
    std::unique_ptr<aisx::MskTp, aisx::MskTpDelete> tp;
};

namespace aisx {

// one stream call's arguments as msk_process_stream resolved them
struct MskCall {
    const cf* in; long in_stride; int n;
    const tag_rec* tags; const int* tag_counts; int tag_cap; // (tags nullptr: none)
    cf* syms; int* produced; long out_stride; int out_cap;   // (syms: the caller's rows or the handle's scratch)
    int par; hipStream_t st;                                 // the call's parity and stream
    void* ready_event;
    unsigned char* fused_bits = nullptr; // the serial kernel writes the bits itself (fused bit tail): their rows, else null
};

// the loop's state and constants, and the call's arguments, under the names MskParams (k_msk.h) and MskpParams (k_mskp.h) share
template <class P>
inline void msk_fill_state(const aisx_msk* h, P& p)
{
    p.nchan = h->nchan;
    p.d_sps = h->d_sps;
    p.gain = h->gain;
    p.gain_omega = h->gain_omega;
    p.limit = h->limit;
    p.mu = h->d_mu;
    p.omega = h->d_omega;
    p.div = h->d_div;
    p.dly1 = h->d_dly1;
    p.dly2 = h->d_dly2;
    p.diff1 = h->d_diff1;
    p.nread = h->d_nread;
    p.carry_in = h->d_carry[h->cur];
    p.carry_out = h->d_carry[h->cur ^ 1];
    p.carry_len_in = h->d_carry_len[h->cur];
    p.carry_len_out = h->d_carry_len[h->cur ^ 1];
    p.carry_cap = aisx_msk::carry_cap;
    p.ctag_out = h->d_ctag[h->cur ^ 1];
    p.ctag_n_out = h->d_ctag_n[h->cur ^ 1];
    p.ctag_cap = aisx_msk::ctag_cap;
    p.consumed = h->d_consumed;
    p.status = h->d_status;
    p.mmse = h->d_mmse;
    p.max_noutput = h->max_noutput;
}
template <class P>
inline void msk_fill_call(const MskCall& c, P& p)
{
    p.in = c.in;
    p.in_stride = c.in_stride;
    p.n = c.n;
    p.syms = c.syms;
    p.out_stride = c.out_stride;
    p.out_cap = c.out_cap;
    p.produced = c.produced;
}

// ---- aisx_msk.hip
int msk_launch(const MskParams& p, int nwg, hipStream_t st);
void msk_fill_common(aisx_msk* h, MskParams& p); // (the stream contract; the GNU Radio path sets its own)
// compacts (carried tags + this call's tags [+ the prepass's list `ctl_new`, whose first `ctl_new_pre` places of every
// channel are room for the carried ones: time-parallel join]) into h->d_ct for the kernel launch that follows
int msk_launch_tagprep(aisx_msk* h, const tag_rec* d_tags, const int* d_tag_counts, int tag_cap, hipStream_t st,
                       int* d_ct_nc = nullptr, const msk_ctag* ctl_new = nullptr, const int* ctl_new_n = nullptr,
                       int ctl_new_cap = 0, int ctl_new_pre = 0);

// ---- aisx_mskp.hip: the time-parallel recovery
void msk_tp_create(aisx_msk* h); // h->tp with its defaults (experiments: and what the AISX_MSK_TP_* knobs say)
bool msk_tp_applies(const aisx_msk* h, const float* d_err, const float* d_mu);
// The three stages of a call, in the order msk_process_stream queues them.  The prepass (c.syms, c.produced and
// c.out_cap not looked at yet) says in *ran_on where it ran: the caller's tag records have been read behind it there.
int msk_tp_prepass(aisx_msk* h, const MskCall& c, hipStream_t* ran_on);
int msk_tp_units_join(aisx_msk* h, const MskCall& c);
// the units' symbols into c.syms, on the call's stream or on the handle's tail stream
int msk_tp_gather(aisx_msk* h, const MskCall& c, bool on_tail);

} // namespace aisx
#pragma GCC visibility pop
