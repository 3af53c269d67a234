/*
 * aisx.h -- C ABI of libaisx.so: the MI355X (gfx950) implementation of the gr-ais
 * per-sample demod hot path.  This is the drop-in boundary: every entry point is
 * `extern "C"`, takes plain pointers / sizes / an opaque handle, returns an int
 * status (no exceptions cross the ABI) and corresponds to one method of the
 * reference's block classes, cited below (paths under bistromath/gr-ais).
 *
 * Two ways to drive each block:
 *   *_process / *_step   batched device path: device pointers, `nchan`
 *                        independent channels laid out channel-major
 *                        (`ptr[c * stride + k]`, stride in items), work queued
 *                        on a hipStream_t passed as void* (NULL = default);
 *   *_work_host          the GNU Radio path: nchan == 1, HOST pointers exactly
 *                        as the scheduler hands them to work()/general_work();
 *                        the call stages, launches and synchronises itself.
 *
 * Per-channel carry state (correlator history, timing-loop registers, NCO
 * phase, AGC window) lives in device memory inside the handle, so a stream is
 * processed by successive calls.
 */
#ifndef AISX_H
#define AISX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AISX_VERSION 300

/* gr_complex = std::complex<float>: interleaved re, im */
typedef struct aisx_cf32 { float re, im; } aisx_cf32;

/* stream tag (gr::tag_t with a PMT double value); keys of
 * lib/corr_est_cc_impl.cc:213-256.  Tags the reference adds on output port 1
 * (:258-266) carry AISX_KEY_PORT1 or-ed into `key`. */
enum {
    AISX_KEY_CORR_START = 0,
    AISX_KEY_PHASE_EST = 1,
    AISX_KEY_TIME_EST = 2,
    AISX_KEY_CORR_EST = 3,
    AISX_KEY_PORT1 = 0x100
};
typedef struct aisx_tag {
    uint64_t offset; /* absolute item offset (nitems_written(0) + i [+ mark_delay]) */
    double value;    /* pmt::from_double payload */
    int32_t key;     /* AISX_KEY_* */
    int32_t chan;    /* channel index (0 for the GNU Radio path) */
} aisx_tag;

enum {
    AISX_OK = 0,
    AISX_ERR_INVALID = -1,      /* bad argument */
    AISX_ERR_OUT_OF_RANGE = -2, /* the reference throws std::out_of_range here */
    AISX_ERR_HIP = -3,          /* HIP runtime error, see aisx_last_error() */
    AISX_ERR_NO_DEVICE = -4,    /* no gfx950 device: there is no CPU fallback */
    AISX_ERR_OVERFLOW = -5,     /* a tag / carry buffer was too small; results truncated */
    AISX_ERR_RUNTIME = -6       /* the reference throws std::runtime_error here */
};

int aisx_version(void);
const char* aisx_last_error(void);
int aisx_device_count(int* count);
int aisx_set_device(int device);
/* measurement hook (bench.py's "copy_ceiling"): the rate, in GB/s of bytes read + bytes written,
 * a plain 16-bytes-per-lane device copy of `bytes` bytes sustains over `iters` launches, timed
 * with hipEvents and no profiler attached: what "HBM-bound" can mean on this chip next to the
 * 8 TB/s spec peak */
int aisx_util_copy_GBs(size_t bytes, int iters, float* GBs);
/* test hook: the streaming AGC kernel (k_agcw.h) forms the gain reference / max_env as a refined
 * hardware reciprocal when the reference is a power of two (the stock 2): this sweeps EVERY float
 * max_env in [2^-100, 2^100] on the device and counts those for which that differs from the
 * correctly rounded float division (*count must come back 0; *example = the largest such value) */
int aisx_util_agc_rcp_mismatches(float reference, unsigned long long* count, float* example);
/* ------------------------------------------------------------------------ */
/* corr_est_cc  (include/ais/corr_est_cc.h:85-106, lib/corr_est_cc_impl.cc)  */
/* ------------------------------------------------------------------------ */
typedef struct aisx_corr aisx_corr;

/* corr_est_cc::make(symbols, sps, mark_delay, threshold) (corr_est_cc.h:102-103,
 * ctor lib/corr_est_cc_impl.cc:48-117).  max_items bounds `n` of one call;
 * max_tags_per_chan bounds the tags one call can return per channel. */
int aisx_corr_create(aisx_corr** h, const aisx_cf32* symbols, int nsym, float sps, unsigned mark_delay,
                     float threshold, int nchan, int max_items, int max_tags_per_chan);
int aisx_corr_destroy(aisx_corr* h);
/* symbols() (corr_est_cc.h:105): d_symbols as stored (reversed conjugate) */
int aisx_corr_symbols(const aisx_corr* h, aisx_cf32* out, int cap);
/* set_symbols() (corr_est_cc.h:106, impl :132-162); keeps the reference's quirks:
 * taps stored as given (no conjugate/reverse), threshold not recomputed, the FFT
 * filter restarts from a zeroed tail.  A different length re-sizes history, output
 * multiple and mark_delay as :143-161 do (up to 2048 samples).  Must not be called
 * while a call on this handle is in flight (the reference holds d_setlock, :135). */
int aisx_corr_set_symbols(aisx_corr* h, const aisx_cf32* symbols, int nsym);
int aisx_corr_geometry(const aisx_corr* h, int* nchan, int* max_items); /* what aisx_corr_create was given */
int aisx_corr_history(const aisx_corr* h);         /* history() = nsym + 1   (:95)  */
int aisx_corr_output_multiple(const aisx_corr* h); /* fft_filter nsamples    (:84-85) */
int aisx_corr_max_noutput_items(const aisx_corr* h); /* 24*1024              (:111-112) */
float aisx_corr_threshold(const aisx_corr* h);     /* d_thresh               (:71-74) */
unsigned aisx_corr_mark_delay(const aisx_corr* h); /* d_mark_delay           (:65-66) */
uint64_t aisx_corr_nitems_written(const aisx_corr* h);
int aisx_corr_reset(aisx_corr* h); /* zero history, nitems_written = 0 */

/* One work() call of n items on every channel (lib/corr_est_cc_impl.cc:164-279).
 * d_in  : n NEW items per channel (the handle supplies the N history items);
 * d_out : n items, the input delayed by N (:184);
 * d_corr: optional port-1 output, the correlator output (:174-177, :188), or NULL.
 * Semantics of one call = one work(noutput_items = n): the peak search restarts
 * at i = 0 and the climb / centre of mass stop at the call's edge.  n need not
 * be a multiple of output_multiple().  Tags stay in device memory (feed them to
 * aisx_msk_process_stream via aisx_corr_tags_device, or fetch them with
 * aisx_corr_read_tags). */
int aisx_corr_process(aisx_corr* h, const aisx_cf32* d_in, long in_stride, aisx_cf32* d_out, long out_stride,
                      aisx_cf32* d_corr, long corr_stride, int n, void* stream);
/* Placement knob (as aisx_agc_set_lds_claim): LDS a workgroup of the F = 4096 build (templates of 513 .. 2048 items) claims
 * beyond what it uses (aisx_corr_get_lds_claim: 49 KB at 513 items to 74 KB at 2048).  The rule: a claim with used + claim
 * greater than what a timing-recovery workgroup leaves on a CU (LDS per CU - aisx_msk_placement's bytes) keeps the
 * correlator's workgroups off the CUs that hold one; two still fit a free CU while 2 x (used + claim) <= LDS per CU.  At 896
 * items (55 KB used) 17 408 bytes do that: in the 4096-channel chain the recovery then runs up to 0.25 ms shorter and the step
 * up to 3 % (5.31 against 5.49 ms on one box, nothing on another), the correlator itself a third longer (1.98 against
 * 1.50 ms) -- a caller's choice between the step and this kernel's own rate; aisx_chain_create leaves it alone (bench.py:
 * config.side.corr_off_recovery_cus).  Results do not depend on it; default 0.  A call whose used + claim exceeds the
 * device's LDS per CU is refused by aisx_corr_process (AISX_ERR_INVALID, nothing launched, the handle unchanged).  Not part
 * of the GNU Radio API. */
int aisx_corr_set_lds_claim(aisx_corr* h, int bytes);
/* the claim in force, and the LDS a workgroup of the F = 4096 build uses itself for this template length (0: the F = 2048
 * build serves it, and takes no claim); either pointer may be NULL */
int aisx_corr_get_lds_claim(const aisx_corr* h, int* bytes, int* used_bytes);
/* measurement hook: when on, aisx_corr_process brackets the main correlator
 * kernel with hipEvents on the launch stream; aisx_corr_last_kernel_ms waits for
 * the last bracket and returns its duration. */
int aisx_corr_set_profiling(aisx_corr* h, int on);
int aisx_corr_last_kernel_ms(aisx_corr* h, float* ms);
/* durations of the main kernel in the calls made since profiling was switched on
 * (the most recent 64 at most), oldest first */
int aisx_corr_kernel_ms_history(aisx_corr* h, float* ms, int cap, int* n);
/* device tag buffers of the last call: tags[c * cap + k], k < min(counts[c], cap).  The
 * handle rotates through three sets: the pointers of call k stay valid (for a consumer on
 * another stream) until call k+3 is launched. */
int aisx_corr_tags_device(const aisx_corr* h, const aisx_tag** d_tags, const int** d_counts, int* cap);
/* copy the last call's tags to the host, channel by channel in emission order;
 * synchronises the stream.  Returns AISX_ERR_OVERFLOW if a channel overflowed
 * max_tags_per_chan or host_cap was too small (what fits is still returned). */
int aisx_corr_read_tags(aisx_corr* h, aisx_tag* host_tags, int host_cap, int* ntags, void* stream);
/* the same for the call `back` calls before the last one (0 = the last; up to 2: the handle keeps
 * three sets) -- what a pipelined caller reads once several steps have been issued */
int aisx_corr_read_tags_back(aisx_corr* h, int back, aisx_tag* host_tags, int host_cap, int* ntags, void* stream);
/* GNU Radio path (nchan == 1): `in` = input_items[0] as the scheduler passes it
 * (history()-1 old items, then noutput_items new ones), out = output_items[0],
 * corr = output_items[1] or NULL, nitems_written = nitems_written(0). */
int aisx_corr_work_host(aisx_corr* h, const aisx_cf32* in, aisx_cf32* out, aisx_cf32* corr, int noutput_items,
                        uint64_t nitems_written, aisx_tag* tags, int tag_cap, int* ntags);

/* ------------------------------------------------------------------------ */
/* msk_timing_recovery_cc (include/ais/msk_timing_recovery_cc.h:46-69,        */
/* lib/msk_timing_recovery_cc_impl.cc) + fused NRZI bit tail                  */
/* (python/ais_demod.py:48-52, lib/invert_impl.cc:62-64)                      */
/* ------------------------------------------------------------------------ */
typedef struct aisx_msk aisx_msk;

/* make(sps, gain, limit, osps) (msk_timing_recovery_cc.h:60, ctor impl :45-62).
 * AISX_ERR_OUT_OF_RANGE if gain <= 0 or osps not in {1,2} (impl :61,:82). */
int aisx_msk_create(aisx_msk** h, float sps, float gain, float limit, int osps, int nchan, int max_items);
int aisx_msk_destroy(aisx_msk* h);
int aisx_msk_geometry(const aisx_msk* h, int* nchan, int* max_items); /* what aisx_msk_create was given */
/* what the recovery kernel's launch occupies: its workgroups (one per CU at most: each takes more than half of a CU's LDS)
 * and the LDS of one -- aisx_chain_create places the front-end kernel's workgroups by these.  Not part of the GNU Radio API. */
int aisx_msk_placement(const aisx_msk* h, int* workgroups, int* lds_bytes_per_workgroup);
int aisx_msk_set_gain(aisx_msk* h, float gain); /* :80-84, AISX_ERR_OUT_OF_RANGE if gain <= 0 */
float aisx_msk_get_gain(const aisx_msk* h);     /* :86-88 */
int aisx_msk_set_limit(aisx_msk* h, float limit); /* :90-92 */
float aisx_msk_get_limit(const aisx_msk* h);      /* :94-96 */
int aisx_msk_set_sps(aisx_msk* h, float sps);     /* :69-74 (d_sps = sps/2, omega reset) */
/* set_sps / set_limit / set_gain return AISX_ERR_INVALID for values outside what the kernel's
 * rings are sized for (sps/2 - |limit| >= 0.5, sps <= ~47, 2 (sps/2 + |limit|) + 3 |gain| <= 32);
 * after set_sps / set_limit ask aisx_msk_out_capacity() again. */
float aisx_msk_get_sps(const aisx_msk* h);        /* :76-78 returns d_sps */
int aisx_msk_forecast(const aisx_msk* h, int noutput_items); /* :98-105 */
/* items per channel the output arrays must hold: ceil((max_items + 128) / (2 (sps/2 - |limit|)))
 * outputs a call can produce without tags, plus room for the extra outputs of max_items / 64
 * time_est tags (each reset restarts the even/odd cadence, :159), times osps.  A call that would
 * need more stops there and reports AISX_MSK_ST_OUT_FULL. */
int aisx_msk_out_capacity(const aisx_msk* h);
int aisx_msk_reset(aisx_msk* h);

/* One general_work() call per channel under the stream contract:
 * the n new items are appended to the unconsumed items kept in the handle,
 * ninput_items = all of them minus one look-ahead item, noutput_items = the
 * largest count whose forecast() fits; unconsumed items and still-live
 * time_est tags are carried to the next call.  d_tags/d_tag_counts/tag_cap: this
 * call's tags as laid out by aisx_corr_tags_device (only key time_est is read,
 * impl :125-130), or NULL.  Outputs (any may be NULL): d_syms = port 0,
 * d_err = port 1, d_mu = port 2 (impl :186-191), d_bits = the unpacked NRZI
 * decoded bit per symbol; all [nchan][out_stride].  d_produced[c] = items
 * written for channel c. */
int aisx_msk_process_stream(aisx_msk* h, const aisx_cf32* d_in, long in_stride, int n, const aisx_tag* d_tags,
                            const int* d_tag_counts, int tag_cap, aisx_cf32* d_syms, float* d_err, float* d_mu,
                            uint8_t* d_bits, long out_stride, int* d_produced, void* stream);
/* The same call for a pipelined caller.  With the time-parallel recovery (k_mskp.h; osps 1, err / mu
 * ports open) the units of a call need its samples and tags but nothing of the call before: they run
 * on a stream of the handle's own, beside the previous call's join on `stream`.  `ready_event` (a
 * hipEvent_t, may be null) is what that stream waits for before it reads d_in / d_tags; without it it
 * waits for `stream` to reach this call, and nothing overlaps.  Results are identical. */
int aisx_msk_process_stream_after(aisx_msk* h, const aisx_cf32* d_in, long in_stride, int n, const aisx_tag* d_tags,
                                  const int* d_tag_counts, int tag_cap, aisx_cf32* d_syms, float* d_err, float* d_mu,
                                  uint8_t* d_bits, long out_stride, int* d_produced, void* stream, void* ready_event);
/* status word per channel of the last call, or-ed over channels (0 = clean):
 * 1 interpolator index out of range (upstream throws), 2 carry buffer overflow,
 * 4 carried-tag buffer overflow, 8 output rows full (results truncated),
 * 16 the tag list handed over was truncated by its producer (corr_est ran out of
 * max_tags_per_chan): tags are missing */
enum {
    AISX_MSK_ST_INTERP_RANGE = 1,
    AISX_MSK_ST_CARRY_OVERFLOW = 2,
    AISX_MSK_ST_TAGCARRY_OVERFLOW = 4,
    AISX_MSK_ST_OUT_FULL = 8,
    AISX_MSK_ST_TAGS_TRUNCATED = 16
};
/* gr::block::set_max_noutput_items(): under the stream contract every general_work call is offered
 * at most that many output items (0, the default: as many as the pending input allows).  With
 * GNU Radio's default buffers the scheduler never offers msk_timing_recovery_cc more than ~2000-4000;
 * a stale time_est tag blocks the later ones until the call ends (reference :140-142), so the value
 * bounds how long.  Takes effect with the next aisx_msk_process_stream. */
int aisx_msk_set_max_noutput_items(aisx_msk* h, int max_noutput_items);
/* The time-parallel recovery (gr-ais_amd/csrc/k_mskp.h), off by default.  The reference loop (:138-202) is a
 * recurrence, but two time_est tags one symbol apart reset it to a state that follows from the tags and
 * the samples alone: the loop is entered at up to `restart_points_per_channel` such pairs per call
 * (<= 64; 0 = off) by one lane each ("units"), and a join pass runs the serial loop from the carried
 * state, compares the two delay registers bit for bit at every restart point it reaches and takes over
 * the unit's symbols and end state where they agree.  Results are identical to the serial kernel's;
 * which is faster depends on the traffic.  join_kernel: 1 = the serial kernel
 * with fast-forward (default), 0 = one lane per channel, -1 = leave; max_unit_items: no unit is started
 * at a restart point further than this from the next one (0 = leave).  Applies to stream calls with
 * osps 1 and the err / mu ports open; everything else takes the serial kernel. */
int aisx_msk_set_time_parallel(aisx_msk* h, int restart_points_per_channel, int join_kernel, int max_unit_items);
int aisx_msk_get_max_noutput_items(const aisx_msk* h);
int aisx_msk_last_status(aisx_msk* h, int* status, void* stream);
/* the per-channel status words [nchan] in device memory (what aisx_msk_last_status copies and or-s) */
int aisx_msk_status_device(const aisx_msk* h, const int** d_status);
/* Diagnostics of the time-parallel recovery (k_mskp.h) for the last aisx_msk_process_stream call,
 * summed over the channels: out10 (ten entries) = { restart points chosen, units whose run was taken over,
 * symbols that came from units, units that ended at the next restart point, units that ended
 * elsewhere (stale tag, end of the row), calls that took the time-parallel path, units whose end
 * state equals what the next unit assumed, out of this many, items of the longest unit, items of all
 * units }.  Waits for `stream`. */
int aisx_msk_restart_stats(aisx_msk* h, long long* out10, void* stream);
/* measurement hook, as aisx_corr_set_profiling: when on, every aisx_msk_process_stream call (serial
 * kernel) brackets the recovery kernel with hipEvents on its stream; aisx_msk_kernel_ms_history returns
 * the durations of the calls made since it was switched on (the most recent 64 at most), oldest first */
int aisx_msk_set_profiling(aisx_msk* h, int on);
int aisx_msk_kernel_ms_history(aisx_msk* h, float* ms, int cap, int* n);
/* The NRZI bit tail (quadrature demod .. invert, python/ais_demod.py:48-52) has no part in
 * the timing recurrence.  With a tail stream set (enable != 0) aisx_msk_process_stream
 * launches it there, ordered after the call's recovery kernel, so that the next call need
 * not wait for it: d_bits of a call is complete on THAT stream (aisx_msk_wait_tail makes
 * another stream wait for it); the caller must then alternate between two d_bits / d_syms /
 * d_produced buffers from call to call.  Default: off, everything on the call's stream. */
int aisx_msk_set_tail_stream(aisx_msk* h, void* tail_stream, int enable);
int aisx_msk_wait_tail(aisx_msk* h, void* stream);
/* The bit tail inside the recovery kernel (default: on).  Where a call allows it -- d_bits given, osps 1, d_err and d_mu
 * NULL, the serial kernel (not the time-parallel recovery) -- the lanes that flush a channel's symbols to memory slice
 * them there and write the bits: no second kernel, no pass over the symbols, and with d_syms NULL the symbols never
 * reach memory at all.  Results are identical, bit for bit, state included: fused and unfused calls may alternate on
 * one handle.  d_bits of a fused call is complete on the call's own `stream`, also when a tail stream is set (nothing
 * of the call runs there); aisx_msk_wait_tail covers both cases.  aisx_msk_last_tail_fused: 1 if the last call that
 * took d_bits was fused, 0 if its bit tail was a kernel of its own.  on = 0: always the separate kernel (twin tests,
 * A/B runs).  The fused flush costs the recovery kernel about 2 %: it pays wherever the bit-tail kernel would delay
 * something.  aisx_chain_create clears the switch for a chain without front end (there the step is the recovery
 * kernel and the bit tail hides beside the next one) and gives it back at aisx_chain_destroy. */
int aisx_msk_set_fused_tail(aisx_msk* h, int on);
int aisx_msk_get_fused_tail(const aisx_msk* h);
int aisx_msk_last_tail_fused(const aisx_msk* h);
/* The schedule of the recovery kernel's lock-step iteration pair.  mode 1 (default): the build that the stream contract
 * launches with osps 1 and d_err / d_mu NULL runs its plain pair loop as a hand-scheduled instruction sequence (operands
 * used where the LDS reads leave them, two waits, the symbol staged while the next pair's reads are in flight).  mode 0:
 * the same statements as the compiler schedules them.  The builds with err / mu ports, osps 2, the GNU Radio path and the
 * join of the time-parallel recovery have the compiler's schedule in either mode.  Every float operation, its operands and
 * its rounding are the same: results are identical bit for bit, state included, and calls of either mode may alternate on
 * one handle.  The switch exists for twin tests and for A/B runs inside one library; it is not a tuning knob. */
int aisx_msk_set_pair_core(aisx_msk* h, int mode);
int aisx_msk_get_pair_core(const aisx_msk* h);
/* Makes `stream` wait until the tag prepass of the last aisx_msk_process_stream call has run, i.e.
 * until that call's recovery kernel stands at the head of its queue.  The recovery kernel is 128
 * workgroups of 90 KB of LDS each: when it becomes ready at the same moment as a kernel with
 * thousands of small workgroups on another stream (both waiting for the same predecessor), those
 * fill every CU first and the recovery waits for a contiguous 90 KB until they drain (measured:
 * 1.6 ms of a 6 ms step, every other step).  A caller that pipelines the next step's sample passes
 * beside the recovery calls this on their stream right after aisx_msk_process_stream.  The first
 * call only arms the event (returns at once).  An event wait and nothing else, unless
 * aisx_msk_set_head_start has been called on the handle. */
int aisx_msk_wait_prepass(aisx_msk* h, void* stream);
/* The event of aisx_msk_wait_prepass fires for both queues at the same instant: which of them the
 * dispatcher serves first is a race (0.3 ms per 5.6 ms step when the recovery kernel loses it).  With
 * microseconds > 0, aisx_msk_wait_prepass also queues a one-wave kernel that sleeps that long on `stream`
 * behind the wait (ticks of the constant-rate wall clock, hipDeviceAttributeWallClockRate), so that the
 * recovery kernel gets there first.  Default 0: off.  aisx_chain_create switches it on for its own
 * streams (20 us; environment AISX_MSK_HEADSTART_US, 0 = off). */
int aisx_msk_set_head_start(aisx_msk* h, int microseconds);
/* GNU Radio path (nchan == 1), host pointers as general_work() receives them
 * (impl :107-206): tags = the time_est tags get_tags_in_range would return or
 * any superset, nitems_read = nitems_read(0).  *consumed is what to pass to
 * consume_each(), *produced the return value.  The reference's loop bound
 * (impl :119,:138) lets the 8-tap interpolator read in[ninput_items], one item
 * past what the scheduler announced; in_has_lookahead = 1 says that item is
 * readable (always true inside a GNU Radio circular buffer), 0 substitutes 0.
 * out_err / out_mu / out_bits may be NULL (ports not connected).  The NRZI bit tail runs only in calls
 * that pass out_bits; its state (previous symbol, previous sliced bit) carries on from the last call
 * that did, so a caller takes bits in every call or in none (the gr::ais block takes none: the tail
 * is four GNU Radio blocks of its own there, python/ais_demod.py:48-52). */
int aisx_msk_general_work_host(aisx_msk* h, int noutput_items, int ninput_items, const aisx_cf32* in, aisx_cf32* out,
                               float* out_err, float* out_mu, uint8_t* out_bits, const aisx_tag* tags, int ntags,
                               uint64_t nitems_read, int in_has_lookahead, int* consumed, int* produced);

/* ------------------------------------------------------------------------ */
/* freqest (include/ais/freqest.h:36-49, lib/freqest_impl.cc) and            */
/* square_and_fft_sync_cc (python/gmsk_sync.py:14-37)                        */
/* ------------------------------------------------------------------------ */
typedef struct aisx_freqsync aisx_freqsync;
/* square_and_fft_sync_cc(samplerate, bits_per_sec, fftlen) (gmsk_sync.py:15);
 * builds freqest::make(int(samplerate), int(bits_per_sec), fftlen) (:25). */
int aisx_freqsync_create(aisx_freqsync** h, double samplerate, double bits_per_sec, int fftlen, int nchan,
                         int max_items);
int aisx_freqsync_destroy(aisx_freqsync* h);
int aisx_freqsync_geometry(const aisx_freqsync* h, int* nchan, int* max_items, int* fftlen);
/* forget what aisx_freqsync_estimate_ahead has queued (nothing of it is committed before the pass it was
 * made for); `stream`: where the next pass will run -- it waits for what the dropped preparations still
 * have in flight */
int aisx_freqsync_drop_ahead(aisx_freqsync* h, void* stream);
/* Placement knob (as aisx_agc_set_lds_claim): LDS a one-wave workgroup of the NCO phase walk (aisx_freqsync_estimate_ahead /
 * aisx_freqsync_agc_process) claims beyond the 3 KB it uses.  aisx_chain_create sets it while the recovery leaves half of the
 * CUs free, so that no walk workgroup lands on a CU that holds a recovery workgroup -- where it also shuts the correlator's
 * workgroup out (4096 channels: the step 0.8 % shorter, the correlator 1.46 instead of 1.53 ms) -- and gives the handle its
 * previous claim back when it is destroyed.  Results do not depend on it; default 0.  Not part of the GNU Radio API. */
int aisx_freqsync_set_walk_lds_claim(aisx_freqsync* h, int bytes);
int aisx_freqsync_get_walk_lds_claim(const aisx_freqsync* h, int* bytes, int* used_bytes);
/* freqest::make(sample_rate, data_rate, fftlen) (include/ais/freqest.h:46) for the block on its own
 * (nchan == 1, aisx_freqest_work / aisx_freqest_work_host): d_offset and d_binsize from the FLOAT sample
 * rate as lib/freqest_impl.cc:46-47 compute them (aisx_freqsync_create truncates it to an int first, as
 * python/gmsk_sync.py:25 does).  max_vectors bounds noutput_items of one work() call. */
int aisx_freqest_create(aisx_freqsync** h, float sample_rate, int data_rate, int fftlen, int max_vectors);
/* ... for nchan rows of vectors, and any fftlen >= 2: freqest::work (lib/freqest_impl.cc:57-88) searches fftlen - offset
 * bins of spectra its caller transformed and needs no transform of its own.  A handle made with a vector length other
 * than 1024 serves aisx_freqest_work / aisx_freqest_work_host only: the square_and_fft_sync_cc entry points
 * (aisx_freqsync_process, _work_host, _agc_process, _estimate_ahead, aisx_chain_create) refuse it with AISX_ERR_INVALID. */
int aisx_freqest_create_n(aisx_freqsync** h, float sample_rate, int data_rate, int fftlen, int nchan, int max_vectors);
int aisx_freqsync_is_estimator_only(const aisx_freqsync* h); /* 1 for such a handle, 0 otherwise */
int aisx_freqsync_reset(aisx_freqsync* h);
/* n new items per channel; every complete fftlen-vector is processed (one
 * freqest work() call per channel); *n_out = items written per channel (a
 * multiple of fftlen); d_fhat (optional) = one estimate per vector,
 * [nchan][fhat_stride]. */
int aisx_freqsync_process(aisx_freqsync* h, const aisx_cf32* d_in, long in_stride, int n, aisx_cf32* d_out,
                          long out_stride, float* d_fhat, long fhat_stride, int* n_out, void* stream);
/* The hier block as ONE GNU Radio block (nchan == 1, HOST pointers): in = n new items, out
 * receives every complete fftlen-vector's worth of mixed items (pending ones stay in the
 * handle, as stream_to_vector keeps them), fhat (optional) one estimate per vector.  Returns the
 * items written (a multiple of fftlen) or a negative status. */
int aisx_freqsync_work_host(aisx_freqsync* h, const aisx_cf32* in, int n, aisx_cf32* out, int out_cap, float* fhat,
                            int fhat_cap);
/* freqest::work on already transformed vectors (lib/freqest_impl.cc:57-88):
 * d_vecs [nchan][nvec*fftlen] (fft-shifted spectra), d_out [nchan][nvec]. */
int aisx_freqest_work(aisx_freqsync* h, const aisx_cf32* d_vecs, long vec_stride, float* d_out, long out_stride,
                      int nvec, void* stream);
/* GNU Radio path (nchan == 1), HOST pointers exactly as the scheduler hands them to
 * freqest_impl::work (include/ais/freqest.h:36-49, lib/freqest_impl.h:39-41,
 * lib/freqest_impl.cc:57-88): in = input_items[0], noutput_items vectors of fftlen
 * gr_complex (item size 8*fftlen, :43); out = output_items[0], one float per vector.
 * maxpos is initialised once per call, as the reference's local is (:68 vs :74).
 * Returns noutput_items (:87) or a negative status. */
int aisx_freqest_work_host(aisx_freqsync* h, int noutput_items, const aisx_cf32* in, float* out);

/* ------------------------------------------------------------------------ */
/* analog.feedforward_agc_cc(nsamples, reference) (python/ais_demod.py:35)   */
/* ------------------------------------------------------------------------ */
typedef struct aisx_agc aisx_agc;
int aisx_agc_create(aisx_agc** h, int nsamples, float reference, int nchan, int max_items);
int aisx_agc_destroy(aisx_agc* h);
/* what aisx_agc_create was given; *fused_ok: the window is one aisx_freqsync_agc_process serves */
int aisx_agc_geometry(const aisx_agc* h, int* nchan, int* max_items, int* nsamples, int* fused_ok);
int aisx_agc_reset(aisx_agc* h);
/* the initial max_env of [GR] feedforward_agc_cc_impl::work: 1e-4 (default; GNU Radio 3.7/3.8
 * "float max_env = 1e-4; // avoid divide by zero, indirectly set max gain") or the 1e-12 of the
 * line upstream has commented out.  Not part of the GNU Radio API. */
int aisx_agc_set_floor(aisx_agc* h, float floor_env);
/* Which kernel serves a call is an implementation detail with one switch: calls with the stock
 * window (512) and a whole number of 512-item blocks run the streaming kernel (k_agcw.h: every
 * wave walks its own run of blocks, nothing but registers between loads and stores), all others
 * the tile kernels (k_agc.h).  Same results bit for bit; on = 0 keeps the tile kernels for every
 * call (A/B measurements, twin tests).  Default on.  Not part of the GNU Radio API. */
int aisx_agc_set_streaming(aisx_agc* h, int on);
/* Placement of the streaming kernel's workgroups when it runs BESIDE the timing recovery (the pipelined
 * chain): a workgroup uses 8 KB of LDS; claiming `bytes` more decides how many of them the dispatcher
 * puts on the 128 CUs that hold a recovery workgroup (92 160 of 163 840 B taken, 71 680 left) and on the
 * other CUs.  The recovery is a recurrence that every co-resident wave delays, and this kernel is the
 * densest arithmetic of the chain.  Measured (round 5, 4096 channels x 65536 samples, interleaved runs on
 * one box): no claim 5.65-5.86 ms per step with the recovery kernel at 5.45-5.66 ms and the correlator at
 * 2.50-2.59; 72 KB (none beside the recovery, two per free CU) 5.44-5.49 with the recovery at 5.05-5.09 and
 * the correlator at 1.89-1.94; 100 KB (one per free CU) 5.71-5.74.  aisx_chain_create sets 73 728 while the
 * recovery's workgroups (32 channels each) leave at least half of the CUs free, 49 152 otherwise (one front-end
 * workgroup beside each recovery workgroup: 8192 channels 9.40-9.42 against 9.47-9.60 ms); default 0.
 * Results do not depend on it.  Environment AISX_AGCW_LDS_PAD overrides (experiments). */
int aisx_agc_set_lds_claim(aisx_agc* h, int bytes);
/* the claim in force, and the LDS a streaming workgroup uses itself (either pointer may be NULL) */
int aisx_agc_get_lds_claim(const aisx_agc* h, int* bytes, int* used_bytes);
int aisx_agc_process(aisx_agc* h, const aisx_cf32* d_in, long in_stride, aisx_cf32* d_out, long out_stride, int n,
                     void* stream);
/* square_and_fft_sync_cc -> feedforward_agc_cc, the first two blocks of python/ais_demod.py:56, in
 * ONE pass over the samples (batched device path): the mixing with the NCO is done where the AGC
 * reads its input, the hier block's output is never stored.  Same results, bit for bit, as
 * aisx_freqsync_process followed by aisx_agc_process on its output; both handles advance as if
 * those had been called.  AGC windows that are a multiple of 8 (the stock 512). */
int aisx_freqsync_agc_process(aisx_freqsync* fs, aisx_agc* agc, const aisx_cf32* d_in, long in_stride, int n,
                              aisx_cf32* d_out, long out_stride, float* d_fhat, long fhat_stride, int* n_out, void* stream);
/* Prepares the frequency estimates (on `stream`) and the NCO phase walk (on `walk_stream`, NULL =
 * the same stream, behind the estimates) of the NEXT aisx_freqsync_agc_process call, which must
 * come with the same d_in / in_stride / n (it then waits for this preparation instead of
 * estimating itself; with other arguments the preparation is dropped).  The walk is a strict
 * recurrence per channel (one lane each, ~2 ms for 65536 samples whatever the channel count):
 * prepared one call ahead and on a stream of its own it runs beside the sample passes of the call
 * before.  A second estimate may be prepared while the first still waits for its call, provided
 * that call leaves no pending items (nothing pending now, its n a multiple of fftlen): issuing
 * estimate_ahead(call k + 1) BEFORE agc_process(call k) gives the walk all of step k to hide in
 * (what bench.py does).  Preparations are consumed in order; a call with other arguments drops all
 * of them.  d_in must stay valid and unchanged until its call. */
int aisx_freqsync_estimate_ahead(aisx_freqsync* fs, const aisx_cf32* d_in, long in_stride, int n, void* stream,
                                 void* walk_stream);
/* GNU Radio path (nchan == 1, HOST pointers): in = input_items[0] as the scheduler passes it to
 * a sync_block with set_history(nsamples): nsamples - 1 old items, then noutput_items new ones.
 * Returns noutput_items or a negative status. */
int aisx_agc_work_host(aisx_agc* h, int noutput_items, const aisx_cf32* in, aisx_cf32* out);

/* ------------------------------------------------------------------------ */
/* ais_demod (python/ais_demod.py:21-56): the demod chain as ONE pipelined    */
/* step per batch of new samples, over the stage handles above                */
/* ------------------------------------------------------------------------ */
typedef struct aisx_chain aisx_chain;
#define AISX_CHAIN_DEPTH 3 /* steps in flight: buffers and events rotate through this many sets */
/* The connect order of python/ais_demod.py:56 -- freq_sync -> agc -> (preamble_detect, 0) ->
 * clockrec -> demod -> slicer -> diff -> invert -- over handles the caller has built with that
 * file's constants (:28-47): fs = aisx_freqsync_create(sps * bits_per_sec, bits_per_sec, fftlen),
 * agc = aisx_agc_create(512, 2), corr = aisx_corr_create(template, sps, 1, 0.9), msk =
 * aisx_msk_create(sps, clockrec_gain, omega_relative_limit, 1), the last three sized for
 * max_items + fftlen items per call.  fs = agc = NULL gives the chain BASELINE.json's metric
 * names (corr_est -> msk timing recovery only).  The handles stay the caller's (tags, status,
 * setters, profiling go through them) and must outlive the chain; they must be fresh or reset
 * when the chain is created (it keeps count of the items stream_to_vector holds back), and while
 * a chain drives them they must not be called directly.  One thread at a time per chain.
 * aisx_chain_create checks the handles against its own arguments (same nchan; corr / msk / agc sized for
 * max_items + fftlen, freq_sync for max_items and the same fftlen; an AGC window the fused front end
 * serves) and returns AISX_ERR_INVALID otherwise.
 * The chain owns four streams, AISX_CHAIN_DEPTH sets of inter-stage buffers and the events that
 * order them: the sample passes of step k + 1 (one stream) run beside the timing recovery of step
 * k (a strict recurrence per channel, on its own stream), its bit tail and the NCO phase walk of
 * step k + 2 (two more).  Results are those of the stages called one after the other, bit for
 * bit.  The HIP runtime shares hardware queues between streams unless GPU_MAX_HW_QUEUES >= 8 is
 * in the environment before the first HIP call (the Python package sets it on import). */
int aisx_chain_create(aisx_chain** h, aisx_freqsync* fs, aisx_agc* agc, aisx_corr* corr, aisx_msk* msk, int nchan,
                      int max_items, int fftlen);
int aisx_chain_destroy(aisx_chain* h); /* waits for the steps in flight; the stage handles are not destroyed */
int aisx_chain_depth(void);            /* AISX_CHAIN_DEPTH */
/* One step: d_in [nchan][in_stride] holds n new items per channel, ready on `stream` (the chain's
 * streams wait for what `stream` has queued so far).  Outputs as in aisx_msk_process_stream:
 * d_syms (optional), d_bits (optional) [nchan][out_stride], d_produced [nchan]; they are complete
 * when aisx_chain_wait(step) says so, and every step in flight needs its own set (rotate through
 * AISX_CHAIN_DEPTH of them).  *step (optional) receives the step's number, counted from 0.
 * d_in_next / next_stride / n_next (optional): the input of the NEXT step, if it is already in
 * device memory: its frequency estimates and NCO phase walk are then prepared during this step
 * (aisx_freqsync_estimate_ahead).  The next call must come with exactly that pointer, stride and
 * count, and the samples must not change in between -- a live source therefore runs one buffer
 * ahead: step k is issued when block k + 1 has arrived.  Without it (NULL) every step estimates
 * for itself: same results, the phase walk (~2 ms at 65536 items) no longer hidden.
 * d_in may be reused once aisx_chain_wait_input(step) has passed (d_in_next: its own step's).
 * A step is NOT transactional: when it fails after its first stage call (a HIP error, a handle
 * misused behind the chain's back), stages already issued have advanced their histories.  The chain
 * then drops what was prepared ahead and refuses every further step (AISX_ERR_INVALID): reset the
 * stage handles and create a new chain.  Argument errors are reported before anything is issued and
 * leave the chain usable. */
int aisx_chain_step(aisx_chain* h, const aisx_cf32* d_in, long in_stride, int n, const aisx_cf32* d_in_next,
                    long next_stride, int n_next, aisx_cf32* d_syms, uint8_t* d_bits, long out_stride, int* d_produced,
                    void* stream, long long* step);
/* `stream` (host_blocks == 0) or the calling thread (host_blocks != 0) waits until the outputs of
 * `step` are complete / until its input buffer has been read for the last time */
int aisx_chain_wait(aisx_chain* h, long long step, void* stream, int host_blocks);
int aisx_chain_wait_input(aisx_chain* h, long long step, void* stream, int host_blocks);
int aisx_chain_synchronize(aisx_chain* h); /* everything issued so far has run */
/* corr_est's port-0 output of `step` (the conditioned samples delayed by the template length,
 * lib/corr_est_cc_impl.cc:184, which the timing recovery consumed): rows chan0 .. chan0 + nch - 1
 * are copied to d_dst[..][dst_stride] on `stream`, *n = items per row.  Valid for the last
 * AISX_CHAIN_DEPTH steps. */
int aisx_chain_read_corr_output(aisx_chain* h, long long step, int chan0, int nch, aisx_cf32* d_dst, long dst_stride, int* n,
                                void* stream);
/* corr_est's tags of `step` on the host (as aisx_corr_read_tags_back, but by step number: steps whose
 * front end emitted no whole vector made no corr_est call and have no tags).  Valid for the last
 * AISX_CHAIN_DEPTH steps; synchronises `stream`. */
int aisx_chain_read_tags(aisx_chain* h, long long step, aisx_tag* host_tags, int host_cap, int* ntags, void* stream);
/* the chain's streams (0 sample passes, 1 timing recovery, 2 bit tail, 3 phase walk), e.g. to
 * read a stage handle's results in order with the step that produced them */
void* aisx_chain_stream(aisx_chain* h, int which);

/* ------------------------------------------------------------------------ */
/* wideband front end (BASELINE config 5; reference analogue: one             */
/* freq_xlating_fir_filter_ccf(decim, low_pass(1, rate, 11e3, 1e3), f_off,    */
/* rate) per channel, python/radio.py:49-54): a polyphase channelizer that    */
/* computes all nlanes uniformly spaced channels f_m = m*fs/nlanes at once    */
/* ------------------------------------------------------------------------ */
typedef struct aisx_pfb aisx_pfb;
/* nlanes = 1024; decim = 1024 (critically sampled) or 512 (2x oversampled);
 * taps = the prototype low-pass (what firdes.low_pass returns), ntaps of them */
int aisx_pfb_create(aisx_pfb** h, int nlanes, int decim, const float* taps, int ntaps, int nstreams, int max_frames);
int aisx_pfb_destroy(aisx_pfb* h);
/* d_in [nstreams][n] new wideband samples (n a multiple of decim); writes
 * n/decim output items per lane: lane m of stream s is row s*nlanes + m of
 * d_out[..][out_stride] (channel-major, ready for the demod stages) */
int aisx_pfb_process(aisx_pfb* h, const aisx_cf32* d_in, long in_stride, int n, aisx_cf32* d_out, long out_stride,
                     int* nframes, void* stream);

/* ------------------------------------------------------------------------ */
/* freq_xlating_fir_filter_ccf(decim, taps, center_freq, samp_rate) for any  */
/* decimation, real prototype and centre frequency (python/radio.py:49-54),  */
/* batched: nstreams input streams, nchan_per_stream output channels each    */
/* ------------------------------------------------------------------------ */
typedef struct aisx_xlate aisx_xlate;
/* 1 <= decim <= 4096, 1 <= ntaps <= 131072, 1 <= nchan_per_stream <= 1024, 1 <= nstreams <= 65535,
 * 1 <= max_items <= 2^30 inputs per call; center_freqs [nstreams][nchan_per_stream] in Hz, |f| <= samp_rate / 2.
 * Output row s * nchan_per_stream + c is stream s filtered at centre c, as the float64 filter
 *   y[k] = e^{-j w D k} sum_n h[n] e^{+j w n} x[kD - n],  w = 2 pi f_c / samp_rate,  x[m] = 0 for m < 0
 * (GNU Radio 3.8's block; the first output uses input 0).  The handle belongs to the device current here. */
int aisx_xlate_create(aisx_xlate** h, int decim, const float* taps, int ntaps, const double* center_freqs,
                      int nchan_per_stream, double samp_rate, int nstreams, int max_items);
int aisx_xlate_destroy(aisx_xlate* h);
/* zero history, input index 0, rotators back to 1 (the centre frequencies stay); waits for the handle's own work */
int aisx_xlate_reset(aisx_xlate* h);
int aisx_xlate_geometry(const aisx_xlate* h, int* nstreams, int* nchan_per_stream, int* decim, int* ntaps, int* max_items);
/* from the next call on; the output rotator goes on from its phase with the new increment (GNU Radio 3.8
 * build_composite_fir): outputs after a retune at output k_r are the filter at the new frequency times
 * e^{-j (w_old - w_new) D k_r} */
int aisx_xlate_set_center_freq(aisx_xlate* h, int stream, int chan, double center_freq);
int aisx_xlate_center_freq(const aisx_xlate* h, int stream, int chan, double* center_freq);
/* outputs the next call with n inputs produces (the same for every row) */
int aisx_xlate_output_count(const aisx_xlate* h, int n);
/* d_in [nstreams][in_stride]: n new inputs per stream (1 <= n <= max_items); writes *nout outputs to columns
 * 0 .. *nout - 1 of every row of d_out[..][out_stride].  Queued on `stream`; calls of one handle must be ordered.
 * Any split of an input into calls gives the same outputs, bit for bit. */
int aisx_xlate_process(aisx_xlate* h, const aisx_cf32* d_in, long in_stride, int n, aisx_cf32* d_out, long out_stride,
                       int* nout, void* stream);
/* The item formats SDR sources deliver.  An integer item's value is ((float)raw - bias) * scale on re and im alike:
 * two float32 operations, each rounded once, so numpy's (raw.astype(float32) - float32(bias)) * float32(scale) gives
 * the same bits (an RTL-SDR's unsigned bytes: bias 127.5 or the caller's choice).  CF32 ignores scale and bias. */
enum {
    AISX_FMT_CF32 = 0, /* float re, im */
    AISX_FMT_CS16 = 1, /* int16 re, im */
    AISX_FMT_CS8 = 2,  /* int8 re, im */
    AISX_FMT_CU8 = 3   /* uint8 re, im */
};
/* aisx_xlate_process for d_in [nstreams][in_stride] ITEMS of `fmt`, converted where the filter stages its window: the
 * same outputs, bit for bit, as aisx_xlate_process on the converted values.  The history the handle carries is the
 * converted values, so a stream may change format between calls.  scale and bias must be finite. */
int aisx_xlate_process_fmt(aisx_xlate* h, const void* d_in, int fmt, float scale, float bias, long in_stride, int n,
                           aisx_cf32* d_out, long out_stride, int* nout, void* stream);

/* ------------------------------------------------------------------------ */
/* host-side tail of the receive chain (python/radio.py:64-73): per-packet,   */
/* bytes-per-second work, plain CPU code, HOST pointers                      */
/* ------------------------------------------------------------------------ */
typedef struct aisx_hdlc aisx_hdlc;
/* digital.hdlc_deframer_bp(length_min, length_max) (python/radio.py:64): flag
 * search, bit unstuffing, bytes packed LSB first, CRC-16/X.25 check. */
int aisx_hdlc_create(aisx_hdlc** h, int length_min, int length_max);
int aisx_hdlc_destroy(aisx_hdlc* h);
/* feeds nbits unpacked bits (one per byte); every frame whose CRC checks is
 * appended to pdu_bytes, frame k = pdu_bytes[pdu_offsets[k] .. pdu_offsets[k+1]);
 * *npdus = frames found (AISX_ERR_OVERFLOW if they did not all fit). */
int aisx_hdlc_work(aisx_hdlc* h, const uint8_t* bits, int nbits, uint8_t* pdu_bytes, int pdu_cap, int* pdu_offsets,
                   int max_pdus, int* npdus);
/* Single-bit repair by CRC syndrome: opt-in, off after create.  A rule names a payload length (octets, FCS excluded)
 * and the message types allowed at that length: bit t of type_mask allows type t = pdu[0] >> 2 (aisx_msg_decode's
 * convention); all ones allows any content. */
typedef struct aisx_hdlc_rule {
    int32_t payload_octets;
    int32_t reserved; /* 0 */
    uint64_t type_mask;
} aisx_hdlc_rule;
#define AISX_HDLC_MAX_RULES 16
/* At most AISX_HDLC_MAX_RULES rules with distinct payload lengths in [length_min - 2, length_max - 2]; nrules == 0
 * turns the repair off.  AISX_ERR_INVALID for anything else, and the handle keeps the rules it had.  With rules, a
 * frame of at least length_min octets whose FCS does NOT match and whose payload length has a rule is looked up by its
 * syndrome, (CRC of the payload) xor (sent FCS): when that is the syndrome of ONE wrong bit inside the frame, the bit
 * is flipped, and when the message type after the flip is in the rule's mask the payload is delivered.  A wrong bit in
 * the FCS delivers the payload as received.  Every other frame is dropped as before; which bits form a frame does not
 * change.  Two or more wrong bits are not repaired, and about n / 65535 of such n-bit frames look like a single error
 * and come out wrong with a matching CRC (before the type check): the marks of aisx_hdlc_work_repair tell a consumer
 * which PDUs to trust less.  The rules apply to every frame that closes after the call, one under way included.
 * The same as aisx_hdlc_set_repair_events with AISX_HDLC_EV_SINGLE. */
int aisx_hdlc_set_repair(aisx_hdlc* h, const aisx_hdlc_rule* rules, int nrules);
/* Repair of one error EVENT: a short fixed pattern of wrong bits anywhere in the destuffed frame.  Both bit sources of
 * the receiver decode differentially, so one wrong decision never gives one wrong bit: a wrong symbol decision of the
 * slicer gives two adjacent wrong bits (PAIR), the sequence detector's typical error two wrong bits two apart (SKIP).
 * An event's id is its span: the distance between its first and last flipped bit. */
#define AISX_HDLC_EV_SINGLE 1 /* pattern 1,   id 0 */
#define AISX_HDLC_EV_PAIR 2   /* pattern 11,  id 1 */
#define AISX_HDLC_EV_SKIP 4   /* pattern 101, id 2 */
#define AISX_HDLC_EV_ALL 7
#define AISX_HDLC_EV_REACH 16383 /* an event is looked for with its last flipped bit less than this far from the frame's last bit */
/* aisx_hdlc_set_repair with a mask of the events to look for (rules: as there; when they apply: as there).
 * AISX_ERR_INVALID also for a mask of 0 or with unknown bits, and the handle keeps the rules and mask it had.  The
 * syndrome of an event whose LAST flipped bit is d bits before the frame's last bit is s(d) ^ s(d + span) (s(d) for
 * SINGLE), s(0) = 0x8000 and one step of the CRC's shift register per bit.  Of the enabled events that give a failed
 * frame's syndrome the one with the smallest d is taken (aisx_hdlc_event_table); when all its flipped bits lie inside
 * the frame (d + span < 8 * octets) they are flipped, and when the message type after the flips is in the length's
 * rule the payload is delivered.  Bits flipped in the FCS change nothing that is delivered.  SINGLE syndromes never
 * equal PAIR or SKIP ones; PAIR at d and SKIP at d + 7140 share theirs, so in frames below 893 octets the choice is
 * the only candidate, and in longer ones the nearer event wins. */
int aisx_hdlc_set_repair_events(aisx_hdlc* h, const aisx_hdlc_rule* rules, int nrules, int events);
/* table [65536]: for every syndrome the enabled event with the smallest d < AISX_HDLC_EV_REACH, as id << 14 | d + 1,
 * or 0 for none: what the deframers look a failed frame up in.  AISX_ERR_INVALID for a bad mask. */
int aisx_hdlc_event_table(int events, uint16_t* table);
/* aisx_hdlc_work with one more output: fix_bits [max_pdus], the frames' repair MARKS: -1 for a frame delivered as
 * received, else (index of the first flipped bit in the frame) | (event id << 16) -- payload + FCS; bit 0 = the first
 * bit received = bit 0 of octet 0; an index of 8 * payload length or more lies in the FCS; the event's other flipped
 * bit, if any, is id bits behind the first.  A single-bit repair's mark is the flipped bit's index.  aisx_hdlc_work on
 * a handle with rules returns the same PDUs without the marks. */
int aisx_hdlc_work_repair(aisx_hdlc* h, const uint8_t* bits, int nbits, uint8_t* pdu_bytes, int pdu_cap, int* pdu_offsets,
                          int32_t* fix_bits, int max_pdus, int* npdus);
/* ais.pdu_to_nmea(designator)::msg_to_sentence (lib/pdu_to_nmea_impl.cc:63-131):
 * writes the NUL-terminated !AIVDM sentence(s) (fragments separated by '\n');
 * returns the string length. */
int aisx_pdu_to_nmea(const char* designator, const uint8_t* pdu, int len, char* out, int cap);
/* The same PDU as STANDARD sentences (aisx_pdu_to_nmea keeps three defects of the reference: a wrong last payload
 * character when len % 3 != 0, the fill count on every fragment, no message id).  With P = ceil(8 len / 6) payload
 * characters, fill = 6 P - 8 len and F = ceil(P / 56) <= 9 fragments (len <= 378), sentence f of F is
 *     [tag]!AIVDM,F,f,S,designator,chars,fill_f*HH
 * character k: message bits 6k .. 6k + 5, most significant first, zero from bit 8 len on (message bit i is bit
 * 7 - i % 8 of octet i / 8), as v + 48 for v < 40, else v + 56 -- the inverse of the parser's rule below; S the one
 * digit seq (0..9) when F > 1, else empty; fill_f = fill for f == F, else 0; HH the upper-case hex XOR of the bytes
 * between '!' and '*'; fragments separated by '\n'.  tag, before every fragment, is \fields*HH\ with fields =
 * "s:" station (if not empty), ',' (if both), "c:" time in decimal (if time >= 0) and HH the XOR of the field bytes; no
 * tag block for an empty station and time < 0.  station: NULL or 0..15 bytes of A-Z a-z 0-9 _ -; time: -1 or
 * 0 .. 10^18 - 1 (the parser reads 18 digits).  Not done: talkers other than AI, VDO, g: group fields, more than nine
 * fragments.  Writes the NUL-terminated text and returns its length; AISX_ERR_INVALID for anything outside the above. */
int aisx_pdu_to_nmea_std(const char* designator, const uint8_t* pdu, int len, int seq, const char* station, int64_t time,
                         char* out, int cap);
/* the length aisx_pdu_to_nmea_std returns, from the lengths alone (len = 0 gives 0) */
int aisx_nmea_std_text_len(int len, int dlen, int slen, int64_t time);

/* ------------------------------------------------------------------------ */
/* batched HDLC deframer on the device: for every channel of a chain step,   */
/* exactly what one aisx_hdlc handle per channel returns when fed that       */
/* channel's bits in call order (the stream state carries across calls)      */
/* ------------------------------------------------------------------------ */
typedef struct aisx_pdu {
    uint64_t end_bit; /* index, in this channel's bit stream counted from create / reset, of the bit that closed the frame */
    int64_t offset;   /* first payload octet in the byte buffer */
    int32_t chan;
    int32_t len;      /* payload octets, FCS excluded */
} aisx_pdu;
typedef struct aisx_hdlc_batch aisx_hdlc_batch;
/* 2 <= length_min <= length_max <= 1024 octets (as aisx_hdlc_create's, frame = payload + FCS); nchan channels of at
 * most max_bits (<= 2^28) bits per call; max_pdus records (and max_pdus * (length_max - 1) payload bytes) per call.
 * The handle belongs to the device that was current here. */
int aisx_hdlc_batch_create(aisx_hdlc_batch** h, int length_min, int length_max, int nchan, int max_bits, int max_pdus);
int aisx_hdlc_batch_destroy(aisx_hdlc_batch* h);
int aisx_hdlc_batch_reset(aisx_hdlc_batch* h); /* back to the state after create; waits for the last process call's work */
/* d_bits [nchan][bits_stride] one bit per byte (nonzero = 1), d_nbits [nchan] on the DEVICE (the chain's
 * d_produced), bits_stride >= max_bits.  Queued on `stream`, no host synchronisation: the counts are read when the
 * work runs.  The PDUs whose CRC checks replace the previous call's results, ordered by channel, then end_bit.  A
 * channel whose count is outside [0, max_bits] is not advanced and the next aisx_hdlc_batch_read says so. */
int aisx_hdlc_batch_process(aisx_hdlc_batch* h, const uint8_t* d_bits, long bits_stride, const int* d_nbits, void* stream);
/* the last call's results in device memory: d_pdus [max_pdus] (offsets into d_bytes), d_count[0] = PDUs found,
 * d_count[1] = records kept = min(found, max_pdus) (a prefix of the ordered list), d_count[2] != 0 after a bad count */
int aisx_hdlc_batch_results_device(const aisx_hdlc_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                   const int** d_count);
/* copies the last call's results to the host (synchronises `stream`): *npdus = PDUs found; the records written are
 * the first min(*npdus, max_pdus, pdu_cap) of them (fewer only where their bytes would pass bytes_cap), their bytes
 * at the same offsets.  AISX_ERR_OVERFLOW when not all were written, AISX_ERR_INVALID when a call since the
 * previous read met a bad count (the flag is then cleared). */
int aisx_hdlc_batch_read(aisx_hdlc_batch* h, aisx_pdu* pdus, int pdu_cap, uint8_t* bytes, long bytes_cap, int* npdus,
                         void* stream);
/* aisx_hdlc_set_repair for every channel of the handle (the same rules, the same results as one host handle per
 * channel with them, marks included).  Waits for the handle's queued work; applies from the next process call on, to
 * every frame that closes in it, one opened before included.  Without rules the deframer launches the kernel it
 * launches on a handle that never had any.  The same as aisx_hdlc_batch_set_repair_events with AISX_HDLC_EV_SINGLE. */
int aisx_hdlc_batch_set_repair(aisx_hdlc_batch* h, const aisx_hdlc_rule* rules, int nrules);
/* aisx_hdlc_set_repair_events for every channel of the handle (the same results as one host handle per channel, marks
 * included); waits and applies as aisx_hdlc_batch_set_repair does.  AISX_ERR_INVALID for bad rules or a bad mask, and
 * the handle keeps what it had.  A mask of exactly AISX_HDLC_EV_SINGLE launches the single-bit kernel; any other mask
 * its own kernel, with the mask's table (aisx_hdlc_event_table) uploaded here. */
int aisx_hdlc_batch_set_repair_events(aisx_hdlc_batch* h, const aisx_hdlc_rule* rules, int nrules, int events);
/* the last call's marks in device memory: d_fix_bits [max_pdus], entry k for record k of
 * aisx_hdlc_batch_results_device (-1: delivered as received, else first flipped bit's index | event id << 16 as
 * aisx_hdlc_work_repair gives it).  On a handle without rules every entry is -1. */
int aisx_hdlc_batch_repairs_device(const aisx_hdlc_batch* h, const int32_t** d_fix_bits);
/* copies the last call's marks to the host (synchronises `stream`): *n = PDUs found, the marks written are those of
 * the first min(*n, max_pdus, cap) records.  AISX_ERR_OVERFLOW when not all were written.  The bad-count flag is
 * left for aisx_hdlc_batch_read. */
int aisx_hdlc_batch_read_repairs(aisx_hdlc_batch* h, int32_t* fix_bits, int cap, int* n, void* stream);

/* ------------------------------------------------------------------------ */
/* batched NMEA armouring on the device: for every record of a device PDU    */
/* list (aisx_hdlc_batch_results_device's), the text aisx_pdu_to_nmea        */
/* writes for it, byte for byte, queued behind the deframer                  */
/* ------------------------------------------------------------------------ */
typedef struct aisx_nmea_batch aisx_nmea_batch;
/* nchan designators (each 0..16 bytes, NUL-terminated; one per channel, as radio.py gives "A" / "B"), at most
 * max_pdus records per call of at most length_max - 1 payload octets (2 <= length_max <= 1024, as the deframer's),
 * text_cap bytes of text (0 = the worst case for these arguments, so nothing can overflow).  The handle belongs to
 * the device that was current here. */
int aisx_nmea_batch_create(aisx_nmea_batch** h, const char* const* designators, int nchan, int max_pdus, int length_max,
                           long text_cap);
int aisx_nmea_batch_destroy(aisx_nmea_batch* h);
/* d_pdus / d_bytes as aisx_hdlc_batch_results_device gives them; d_npdus: ONE int on the device = records to armour
 * (for the deframer: d_count + 1); d_nfound: optional (NULL) int on the device = PDUs the producer found
 * (d_count + 0), only used to report a producer's overflow.  Queued on `stream`; no host sync.  Output record i
 * belongs to input record i (chan and end_bit copied); its offset / len give its text in the text buffer, followed
 * by one '\n' that len does not count.  A record with an empty payload gets no text and no newline; a record whose
 * chan is outside [0, nchan) or whose len is above length_max - 1, and a count outside [0, max_pdus], give no text
 * and make the next read say so.  Records whose text does not fit text_cap are not written (a prefix is). */
int aisx_nmea_batch_process(aisx_nmea_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes, const int* d_npdus,
                            const int* d_nfound, void* stream);
/* the last call's results in device memory: d_recs [max_pdus], d_text, d_count[0] = PDUs found (the producer's count,
 * else the record count), d_count[1] = records written, d_count[2] != 0 after bad input */
int aisx_nmea_batch_results_device(const aisx_nmea_batch* h, const aisx_pdu** d_recs, const char** d_text,
                                   const int** d_count);
/* copies the last call's results to the host (synchronises `stream`): *nrecs = records copied, the first of those
 * written that fit rec_cap and (text and newline) text_cap, their text at the same offsets; *nfound (may be NULL) as
 * d_count[0].  AISX_ERR_OVERFLOW when fewer records were copied than *nfound, AISX_ERR_INVALID when a call since the
 * previous read met bad input (the flag is then cleared). */
int aisx_nmea_batch_read(aisx_nmea_batch* h, aisx_pdu* recs, int rec_cap, char* text, long text_cap, int* nrecs,
                         int* nfound, void* stream);
/* A handle in the STANDARD form: per record the text of aisx_pdu_to_nmea_std, byte for byte, with the station of the
 * record's channel (stations: [nchan], or NULL for none), the handle's time and message ids.  length_max - 1 <= 378;
 * text_cap = 0 is this form's worst case (the longest designator and station, an 18-digit time, the id digit).
 * process, results_device, read and destroy work on it as on any handle; records, text layout, counts and flag are
 * the same.  Ids: one counter per handle, in device memory, 0 after create; a written record of more than one
 * sentence gets (counter + the written multi-sentence records before it in the list) mod 10, and the call advances
 * the counter by its written multi-sentence records (records cut by text_cap, refused records and empty payloads take
 * no id, so the text never skips one). */
int aisx_nmea_batch_create_std(aisx_nmea_batch** h, const char* const* designators, const char* const* stations, int nchan,
                               int max_pdus, int length_max, long text_cap);
/* the c: value of the following process calls' tag blocks (-1, the initial value: none; else 0 .. 10^18 - 1).  A launch
 * parameter: no synchronisation, no upload.  The three calls below refuse a handle that is not in the standard form. */
int aisx_nmea_batch_set_time(aisx_nmea_batch* h, int64_t time);
/* counter = 0 and time = -1; waits for the handle's queued work */
int aisx_nmea_batch_reset(aisx_nmea_batch* h);
/* *id = the id the next multi-sentence record will get (synchronises `stream`) */
int aisx_nmea_batch_next_id(aisx_nmea_batch* h, int* id, void* stream);

/* ------------------------------------------------------------------------ */
/* !AIVDM text back into PDUs: on the host (the specification), and batched   */
/* on the device, where the record list feeds the stages behind the deframer  */
/* ------------------------------------------------------------------------ */
/* The text is a byte stream cut into calls anywhere; every result is the same for every way of cutting it.  A line
 * ends at '\n' (one '\r' directly before it is dropped); line indices count line ends from create / reset.  A line of
 * more than max_line bytes ('\r' included) is rejected once (REJ_FORMAT), where its '\n' arrives.  A sentence is a
 * line of exactly the form
 *     [\tagblock\]!TTVDM,F,f,[s],chan,payload,fill*HH
 * TT two of A-Z / 0-9; F, f one digit 1..9 each, f <= F; s empty or one digit; chan 0..16 bytes without ',' or '*';
 * payload any bytes without ','; fill one digit 0..5; HH two hex digits (either case), the line's last bytes.  A tag
 * block runs from a leading '\' to the next one (none: REJ_FORMAT); its time is the first ','-separated field, of
 * what precedes its last '*', that is "c:" and 1..18 digits, else -1 (as for a sentence without a block); the block's
 * own checksum is not looked at.  Then, the first failure naming the reject: HH is the XOR of the bytes between '!'
 * and '*' (REJ_CHECKSUM); chan equals one of the designators byte for byte, the smallest such index being the
 * record's chan (REJ_CHANNEL); every payload byte is in '0'..'W' or '`'..'w' (REJ_ARMOUR).  With
 * AISX_NMEA_PARSE_REF_TAIL the last payload character of a sentence with f == F and fill > 0 is not checked and
 * counts as six zero bits (aisx_pdu_to_nmea keeps the reference's defect in that character).
 * Messages form from accepted sentences in line order: F == 1 is a message; f == 1 with F > 1 opens a group, which
 * completes when the next F - 1 accepted sentences carry f = 2..F in order with the same F, s and chan; anything
 * else closes it (a sentence with f == 1 opens the next).  Every accepted sentence that ends up in no completed
 * message counts in REJ_FRAGMENT, in the call that decides it.  An open group and a partial line survive calls.
 * A message of P payload characters (its sentences' one behind the other) and the LAST sentence's fill has
 * nbits = 6 P - fill and len = ceil(nbits / 8) octets; nbits <= 0 or len > length_max - 1 counts REJ_LENGTH and
 * gives no record.  Character c is v = c - 48, less 8 more if that is above 40, six bits, most significant first;
 * message bit i is bit 7 - i % 8 of octet i / 8 (what aisx_msg_decode reads); bits from nbits on are zero.
 * The record: chan, len, offset (records' bytes one behind the other), end_bit = the line index of the message's
 * last sentence; times[k] = the FIRST sentence's time. */
enum { AISX_NMEA_PARSE_REF_TAIL = 1 };
/* what a call reports: int counts[AISX_NMEAP_NCNT] */
enum {
    AISX_NMEAP_FOUND = 0,    /* messages that give a record */
    AISX_NMEAP_KEPT,         /* records written: the first that fit the capacities (a prefix) */
    AISX_NMEAP_BAD_INPUT,    /* device form only: a call since the last read was refused */
    AISX_NMEAP_LINES,        /* line ends */
    AISX_NMEAP_SENTENCES,    /* lines accepted as sentences */
    AISX_NMEAP_REJ_FORMAT, AISX_NMEAP_REJ_CHECKSUM, AISX_NMEAP_REJ_CHANNEL, AISX_NMEAP_REJ_ARMOUR, /* lines rejected */
    AISX_NMEAP_REJ_FRAGMENT, /* accepted sentences that ended up in no completed message */
    AISX_NMEAP_REJ_LENGTH,   /* completed messages without a record */
    AISX_NMEAP_CARRIED,      /* bytes of text held for the next call: the partial line and the open group's lines */
    AISX_NMEAP_NCNT
};
typedef struct aisx_nmea_parse aisx_nmea_parse;
/* nchan designators of 0..16 bytes, 2 <= length_max <= 1024, 64 <= max_line <= 4096, flags 0 or
 * AISX_NMEA_PARSE_REF_TAIL.  Plain C++, no device. */
int aisx_nmea_parse_create(aisx_nmea_parse** h, const char* const* designators, int nchan, int length_max, int max_line,
                           int flags);
int aisx_nmea_parse_destroy(aisx_nmea_parse* h);
int aisx_nmea_parse_reset(aisx_nmea_parse* h); /* drops the open group and the partial line; line indices start at 0 */
/* times may be NULL.  AISX_ERR_OVERFLOW when KEPT < FOUND (pdu_cap or bytes_cap); the state advances all the same. */
int aisx_nmea_parse_work(aisx_nmea_parse* h, const char* text, long nbytes, aisx_pdu* pdus, int pdu_cap, uint8_t* bytes,
                         long bytes_cap, int64_t* times, int* counts);

typedef struct aisx_nmea_parse_batch aisx_nmea_parse_batch;
/* The device form: per call at most max_bytes (<= 2^30) bytes of text holding at most max_lines (<= 2^26) line ends,
 * at most max_pdus records (the byte buffer holds max_pdus * (length_max - 1), so only max_pdus can truncate).
 * Records, bytes, times and counts equal the host form's with pdu_cap = max_pdus, bit for bit, call by call.  The
 * handle belongs to the device that was current here. */
int aisx_nmea_parse_batch_create(aisx_nmea_parse_batch** h, const char* const* designators, int nchan, int length_max,
                                 int max_line, int flags, long max_bytes, int max_lines, int max_pdus);
int aisx_nmea_parse_batch_destroy(aisx_nmea_parse_batch* h);
int aisx_nmea_parse_batch_reset(aisx_nmea_parse_batch* h); /* waits for the handle's queued work */
/* d_text: the call's bytes in device memory; d_nbytes: ONE value on the device, read when the work runs (the armouring
 * stage's text length can be handed over as it is).  Queued on `stream`, no host synchronisation.  A call whose
 * count lies outside [0, max_bytes], or whose text holds more than max_lines line ends, advances nothing and makes
 * the next read say so.  No byte at or beyond *d_nbytes is read. */
int aisx_nmea_parse_batch_process(aisx_nmea_parse_batch* h, const char* d_text, const long long* d_nbytes, void* stream);
/* the last call's results in device memory: d_pdus [max_pdus], d_bytes, d_count [AISX_NMEAP_NCNT] (its first three
 * entries as every producer's here: found, kept, bad-input flag), d_times [max_pdus] */
int aisx_nmea_parse_batch_results_device(const aisx_nmea_parse_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                         const int** d_count, const int64_t** d_times);
/* copies the last call's results to the host (synchronises `stream`): the first records kept that fit pdu_cap and
 * bytes_cap (counts[AISX_NMEAP_KEPT] says how many), times may be NULL.  AISX_ERR_INVALID when a call since the
 * previous read was refused (the flag is then cleared), AISX_ERR_OVERFLOW when fewer records were copied than found. */
int aisx_nmea_parse_batch_read(aisx_nmea_parse_batch* h, aisx_pdu* pdus, int pdu_cap, uint8_t* bytes, long bytes_cap,
                               int64_t* times, int* counts, void* stream);

/* ------------------------------------------------------------------------ */
/* ITU-R M.1371 message fields: one PDU on the host (the specification), and  */
/* every record of a device PDU list at once, queued behind the deframer      */
/* ------------------------------------------------------------------------ */
/* Columns of a decoded message.  Values are the transmitted integers (no scaling: longitude and latitude in 1/10000
 * minute, speed in 1/10 knot, course in 1/10 degree ...; type 27's coarser position, speed and course are brought to
 * these class-A units by exact integer multiplication).  A column the message's type does not carry, or whose bits
 * the payload does not hold entirely, is AISX_MSG_NA. */
enum {
    AISX_MSG_COL_TYPE = 0, AISX_MSG_COL_REPEAT, AISX_MSG_COL_MMSI, AISX_MSG_COL_FLAGS, AISX_MSG_COL_NAV_STATUS,
    AISX_MSG_COL_ROT, AISX_MSG_COL_SOG, AISX_MSG_COL_ACCURACY, AISX_MSG_COL_LON, AISX_MSG_COL_LAT, AISX_MSG_COL_COG,
    AISX_MSG_COL_HEADING, AISX_MSG_COL_SECOND, AISX_MSG_COL_MANEUVER, AISX_MSG_COL_RAIM, AISX_MSG_COL_RADIO,
    AISX_MSG_COL_IMO, AISX_MSG_COL_AIS_VERSION, AISX_MSG_COL_SHIPTYPE, AISX_MSG_COL_TO_BOW, AISX_MSG_COL_TO_STERN,
    AISX_MSG_COL_TO_PORT, AISX_MSG_COL_TO_STARBOARD, AISX_MSG_COL_EPFD, AISX_MSG_COL_YEAR, AISX_MSG_COL_MONTH,
    AISX_MSG_COL_DAY, AISX_MSG_COL_HOUR, AISX_MSG_COL_MINUTE, AISX_MSG_COL_DRAUGHT, AISX_MSG_COL_DTE, AISX_MSG_COL_PART,
    AISX_MSG_COL_AID_TYPE, AISX_MSG_COL_OFF_POSITION, AISX_MSG_COL_VIRTUAL_AID, AISX_MSG_COL_ASSIGNED,
    AISX_MSG_COL_CS_FLAGS, /* type 18's bits 141 .. 146 as one value: cs, display, dsc, band, msg22, assigned */
    AISX_MSG_NCOL
};
#define AISX_MSG_NA (-2147483647 - 1)
/* bits of the FLAGS column, which every row carries */
enum {
    AISX_MSG_FL_COMPLETE = 1,  /* the payload holds the type's whole minimum length (38 bits for a type without a layout) */
    AISX_MSG_FL_NO_LAYOUT = 2, /* only TYPE, REPEAT and MMSI are decoded: types 6-10, 12-17, 20, 22, 23, 25, 26, 0, 28-63 */
    AISX_MSG_FL_BAD_RECORD = 4 /* device lists only: chan or len out of range; nothing was read, every other column is NA */
};
/* a row's strings, six-bit characters as bytes ('@' for 0, nothing stripped); a slot the message does not carry, or
 * does not hold entirely, is all NUL: [0, 7) call sign, [7] NUL, [8, 28) name, [28, 48) destination */
#define AISX_MSG_STR 48
/* Message bit i is bit 7 - i % 8 of pdu[i / 8] (the bits aisx_pdu_to_nmea's payload characters are made of).  Types
 * 1-3, 4, 5, 11, 18, 19, 21 (without the name extension), 24 (parts A and B, without the vendor id) and 27 are decoded
 * field by field (csrc/aisx_msgtab.h holds the layouts).  cols [AISX_MSG_NCOL], strs [AISX_MSG_STR].  Plain C++, no
 * device.  AISX_ERR_INVALID for len < 0 or a missing pointer. */
int aisx_msg_decode(const uint8_t* pdu, int len, int32_t* cols, char* strs);

typedef struct aisx_msg_batch aisx_msg_batch;
/* at most max_pdus records per call on nchan channels, of at most length_max - 1 payload octets (2 <= length_max <=
 * 1024, as the deframer's).  The handle owns int32_t cols[AISX_MSG_NCOL][max_pdus] and char strs[max_pdus][AISX_MSG_STR]
 * on the device that was current here. */
int aisx_msg_batch_create(aisx_msg_batch** h, int nchan, int max_pdus, int length_max);
int aisx_msg_batch_destroy(aisx_msg_batch* h);
/* d_pdus / d_bytes / d_npdus / d_nfound as aisx_nmea_batch_process takes them (record offsets into d_bytes need be
 * neither ordered nor contiguous).  Queued on `stream`; no host sync.  Row i of the table is aisx_msg_decode of
 * record i's payload (its chan and end_bit stay in the input list); a record whose chan is outside [0, nchan) or whose
 * len is outside [0, length_max - 1] gets FLAGS = AISX_MSG_FL_BAD_RECORD, NA columns and NUL strings without a payload
 * byte being read, and makes the next read say so; a count outside [0, max_pdus] writes no rows and does the same. */
int aisx_msg_batch_process(aisx_msg_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes, const int* d_npdus,
                           const int* d_nfound, void* stream);
/* the last call's table in device memory: column c is d_cols + c * *col_stride (*col_stride = max_pdus), row i's
 * strings d_strs + i * AISX_MSG_STR; d_count[0] = PDUs found (the producer's count, else the record count),
 * d_count[1] = rows written, d_count[2] != 0 after bad input */
int aisx_msg_batch_results_device(const aisx_msg_batch* h, const int32_t** d_cols, long* col_stride, const char** d_strs,
                                  const int** d_count);
/* copies the first min(rows written, cap) rows to the host (synchronises `stream`): cols [AISX_MSG_NCOL][col_stride]
 * with col_stride >= cap, strs [cap][AISX_MSG_STR]; *nrecs = rows copied, *nfound (may be NULL) as d_count[0].
 * AISX_ERR_OVERFLOW when fewer rows were copied than *nfound, AISX_ERR_INVALID when a call since the previous read met
 * bad input (the flag is then cleared). */
int aisx_msg_batch_read(aisx_msg_batch* h, int32_t* cols, long col_stride, char* strs, int cap, int* nrecs, int* nfound,
                        void* stream);

/* The inverse of aisx_msg_decode: a row of the column table -> the payload octets of its layout.  cols
 * [AISX_MSG_NCOL] and strs [AISX_MSG_STR] exactly as aisx_msg_decode gives them (strs NULL: all NUL).
 *   - The type is as_type when that is in 1..63, else cols[TYPE]; for type 24 the part is as_part when that is >= 0,
 *     else cols[PART] (NA: the layout without a part, PART written as 3).
 *   - *len = ceil(minimum bits / 8) octets of the layout: 21 (1-3, 4, 11, 18, 24B), 53 (5), 39 (19), 34 (21), 20 (24A
 *     and 24 with another part), 12 (27).  Every column the layout carries is written at its place; bits that no
 *     column or string covers (spares, type 24B's vendor id, type 21's name extension) are zero.
 *   - TYPE and PART are the chosen ones, FLAGS is ignored; a column that is AISX_MSG_NA takes the protocol's "not
 *     available" value (NAV_STATUS 15, ROT -128, SOG 1023, LON 181 deg, LAT 91 deg, COG 3600, HEADING 511, SECOND 60,
 *     HOUR 24, MINUTE 60, DTE 1) and 0 where there is none.  Type 27's LON / LAT / SOG / COG are converted from
 *     class-A units in integers: v / 1000 to nearest (halves away from zero); SOG 1023 -> 63, else min(62, (v + 5) /
 *     10); COG >= 3600 -> 511, else ((v + 5) / 10) % 360.
 *   - A string slot is written up to its first NUL ('@' from there on): bytes 64..95 as b - 64, 32..63 as b.
 * *status is 0 or a sum of AISX_MSG_ENC_*; with a status other than 0 the row is refused: *len = 0, nothing written.
 * Nothing is ever truncated: a value that does not fit its field (the converted value for type 27) is a range error.
 * Returns AISX_OK in both cases, AISX_ERR_INVALID for a missing pointer, AISX_ERR_OVERFLOW when cap is below the
 * length (nothing written).  Plain C++, no device. */
enum {
    AISX_MSG_ENC_NO_MMSI = 1,   /* MMSI is AISX_MSG_NA or outside [0, 2^30) (then with AISX_MSG_ENC_RANGE) */
    AISX_MSG_ENC_NO_LAYOUT = 2, /* a type without a layout (AISX_MSG_FL_NO_LAYOUT's), AISX_MSG_NA or outside 1..63 */
    AISX_MSG_ENC_RANGE = 4,     /* a column the layout carries does not fit its field */
    AISX_MSG_ENC_BAD_CHAR = 8,  /* a string byte outside 32..95 before the slot's first NUL (lower case included) */
    AISX_MSG_ENC_BAD_ROW = 16   /* device lists only: a row index outside the table or a channel outside [0, nchan) */
};
int aisx_msg_encode(const int32_t* cols, const char* strs, int as_type, int as_part, uint8_t* pdu, int cap, int* len,
                    int* status);

#define AISX_MSG_ENC_PITCH 56 /* octets between the payloads of two records of aisx_msg_enc_batch's list */
typedef struct aisx_msg_enc_batch aisx_msg_enc_batch;
/* at most max_rows records per call, made from a table of table_rows rows, on nchan channels.  The handle owns the
 * records, AISX_MSG_ENC_PITCH * max_rows payload bytes and a status per record on the device that was current here. */
int aisx_msg_enc_batch_create(aisx_msg_enc_batch** h, int nchan, int max_rows, int table_rows);
int aisx_msg_enc_batch_destroy(aisx_msg_enc_batch* h);
/* d_cols / col_stride / d_strs as aisx_msg_batch_results_device or aisx_track_batch_results_device gives them (d_strs
 * 4-byte aligned, or NULL: all NUL); d_nrows: ONE int on the device, the records to make.  d_idx (may be NULL): int32
 * [rows], record i is made from table row d_idx[i] -- the vessel table's d_changed with d_count + AISX_TRK_CNT_CHANGED,
 * say; without it record i is row i.  d_chan (may be NULL: channel 0): int32, the channel of record i at d_chan[i]
 * without d_idx and at d_chan[d_idx[i]] with it (a column of the table, then).  A row index outside [0, table_rows) or
 * a channel outside [0, nchan) gives status AISX_MSG_ENC_BAD_ROW and the table is not read for that record.
 * Record i: end_bit = i, offset = AISX_MSG_ENC_PITCH * i, len and status as aisx_msg_encode gives them (len 0 for a
 * refused row, whose channel is written as 0 when it is the bad part), the bytes of its pitch beyond len zero.
 * Queued on `stream`; no host sync.  A row count outside [0, max_rows] writes nothing and makes the next read say so. */
int aisx_msg_enc_batch_process(aisx_msg_enc_batch* h, const int32_t* d_cols, long col_stride, const char* d_strs,
                               const int32_t* d_idx, const int* d_nrows, const int32_t* d_chan, int as_type, int as_part,
                               void* stream);
/* the last call's list in device memory, in the layout every stage behind the deframer takes: d_pdus [max_rows],
 * d_bytes, d_count[0] = d_count[1] = records, d_count[2] != 0 after a bad row count, d_count[3] = rows encoded,
 * d_count[4] = rows refused; d_status int32 [max_rows] */
int aisx_msg_enc_batch_results_device(const aisx_msg_enc_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                      const int** d_count, const int32_t** d_status);
/* copies the first min(records, cap) records, their status and their AISX_MSG_ENC_PITCH bytes each to the host
 * (synchronises `stream`): pdus [cap], status [cap], bytes [bytes_cap]; *nrecs = records copied, counts (may be NULL)
 * int [5] as d_count.  AISX_ERR_OVERFLOW when fewer were copied than there are (cap, or bytes_cap below the pitch times
 * the records), AISX_ERR_INVALID when a call since the previous read met a bad row count (the flag is then cleared). */
int aisx_msg_enc_batch_read(aisx_msg_enc_batch* h, aisx_pdu* pdus, int32_t* status, int cap, uint8_t* bytes, long bytes_cap,
                            int* nrecs, int* counts, void* stream);

/* ------------------------------------------------------------------------ */
/* the vessel table: the latest state per MMSI, merged from decoded tables    */
/* call by call -- on the host (the specification), and in device memory,     */
/* queued behind the field decoder                                            */
/* ------------------------------------------------------------------------ */
/* Columns of a vessel: the message columns with their indices, then */
enum {
    AISX_TRK_COL_COUNT = AISX_MSG_NCOL, /* rows merged into the vessel (stays at INT32_MAX once there) */
    AISX_TRK_COL_STAMP,                 /* the stamp of the last update that merged a row */
    AISX_TRK_COL_POS_STAMP,             /* ... that merged a row with LON and LAT both not AISX_MSG_NA; NA until then */
    AISX_TRK_COL_CHAN,                  /* chan of the last merged row's PDU record; NA when no record list was given */
    AISX_TRK_NCOL
};
/* what an update or expire reports: int counts[AISX_TRK_NCNT] */
enum {
    AISX_TRK_CNT_VESSELS = 0, /* vessels in the table */
    AISX_TRK_CNT_MERGED,      /* the last update: rows merged, */
    AISX_TRK_CNT_SKIPPED,     /* rows with AISX_MSG_FL_BAD_RECORD or without an MMSI, */
    AISX_TRK_CNT_DROPPED,     /* rows of an unknown MMSI that met a full table, */
    AISX_TRK_CNT_CHANGED,     /* vessels that merged at least one row (0 after an expire) */
    AISX_TRK_CNT_REMOVED,     /* the last expire: vessels removed */
    AISX_TRK_CNT_FULL,        /* the last update dropped a row */
    AISX_TRK_CNT_BAD_INPUT,   /* device form only: a row count outside [0, max_rows] since the last read */
    AISX_TRK_NCNT
};
/* The table holds `capacity` vessels as a struct of arrays, int32_t cols[AISX_TRK_NCOL][capacity] and char
 * strs[capacity][AISX_MSG_STR]; vessel v is the v-th distinct MMSI ever accepted, in order of first appearance, so the
 * table is dense in [0, nvessels).  An update takes the rows of a decoded table (the layout of aisx_msg_decode /
 * aisx_msg_batch_read; recs, optional, the PDU records the rows were decoded from) in ascending row order:
 *   - a row with AISX_MSG_FL_BAD_RECORD, or whose MMSI is AISX_MSG_NA, is skipped;
 *   - a row of an unknown MMSI creates vessel nvessels++ (every column NA, strings NUL, COUNT 0), or is dropped when
 *     the table is full;
 *   - every message column of the row that is not NA replaces the vessel's (TYPE, REPEAT, MMSI and FLAGS always do),
 *     every string slot ([0, 8), [8, 28), [28, 48)) whose first byte is not NUL replaces the vessel's slot whole;
 *   - COUNT, STAMP, POS_STAMP and CHAN are set as described above.
 * Values are kept as transmitted: the protocol's own "not available" codes (longitude 181 degrees, speed 1023 ...) are
 * values like any other and replace what was known; mapping them is the caller's business.  Every int32 but
 * AISX_MSG_NA is an MMSI (0 and 2^30 - 1 included).  The changed list of an update: the vessels that merged a row,
 * ordered by the first row that touched each.  Plain C++, no device.  1 <= capacity <= 2^24. */
typedef struct aisx_track aisx_track;
int aisx_track_create(aisx_track** h, int capacity);
int aisx_track_destroy(aisx_track* h);
/* cols [AISX_MSG_NCOL][col_stride] (col_stride >= n), strs [n][AISX_MSG_STR], recs [n] or NULL, counts
 * [AISX_TRK_NCNT] or NULL */
int aisx_track_update(aisx_track* h, const int32_t* cols, long col_stride, const char* strs, const aisx_pdu* recs, int n,
                      int32_t stamp, int* counts);
/* removes every vessel whose STAMP is below min_stamp; the others keep their order and are renumbered from 0; the
 * changed list becomes empty */
int aisx_track_expire(aisx_track* h, int32_t min_stamp, int* counts);
/* the table where it is (valid until the next update or expire): column c is *cols + c * *col_stride */
int aisx_track_data(const aisx_track* h, const int32_t** cols, long* col_stride, const char** strs, int* nvessels);
int aisx_track_changed(const aisx_track* h, const int** idx, int* nchanged);

typedef struct aisx_track_batch aisx_track_batch;
/* The same table on the device that was current here, updated from at most max_rows (<= 2^24) rows per call: two
 * table buffers (expire compacts from one into the other), an open-addressing hash from MMSI to vessel of at least
 * 2 * capacity slots, and a workspace in proportion to max_rows.  Table, changed list and counts equal the host
 * form's, bit for bit, whatever order the device ran the rows in. */
int aisx_track_batch_create(aisx_track_batch** h, int capacity, int max_rows);
int aisx_track_batch_destroy(aisx_track_batch* h);
int aisx_track_batch_reset(aisx_track_batch* h); /* an empty table; waits for the work queued before */
/* d_cols / col_stride / d_strs as aisx_msg_batch_results_device gives them, d_pdus the records the rows were decoded
 * from (or NULL), d_nrows ONE int on the device (for the decoder: d_count + 1).  Queued on `stream`; no host sync.  A
 * count outside [0, max_rows] merges nothing and makes the next read say so. */
int aisx_track_batch_process(aisx_track_batch* h, const int32_t* d_cols, long col_stride, const char* d_strs,
                             const aisx_pdu* d_pdus, const int* d_nrows, int32_t stamp, void* stream);
int aisx_track_batch_expire(aisx_track_batch* h, int32_t min_stamp, void* stream);
/* the table in device memory: column c is d_cols + c * *col_stride (*col_stride = capacity), vessel v's strings
 * d_strs + v * AISX_MSG_STR, d_changed [max_rows], d_count [AISX_TRK_NCNT].  d_cols and d_strs name the buffer that
 * holds the table once the calls queued so far have run: an expire moves the table to the other one. */
int aisx_track_batch_results_device(const aisx_track_batch* h, const int32_t** d_cols, long* col_stride,
                                    const char** d_strs, const int** d_changed, const int** d_count);
/* copies vessels [first, first + n) that exist to the host (synchronises `stream`): cols [AISX_TRK_NCOL][col_stride]
 * with col_stride >= n, strs [n][AISX_MSG_STR]; *nvessels = vessels in the table.  AISX_ERR_INVALID when a call since
 * the previous read met a bad count (the flag is then cleared). */
int aisx_track_batch_read(aisx_track_batch* h, int first, int n, int32_t* cols, long col_stride, char* strs, int* nvessels,
                          void* stream);
/* d_count on the host (synchronises `stream`); the bad-input flag is reported and left as it is */
int aisx_track_batch_counts(aisx_track_batch* h, int* counts, void* stream);
/* the vessels of the last update's changed list, gathered on the device into one block and copied (synchronises
 * `stream`): idx [cap], cols [AISX_TRK_NCOL][col_stride] with col_stride >= cap, strs [cap][AISX_MSG_STR], row j for
 * vessel idx[j]; *nchanged = the list's length.  When cap is smaller than that: AISX_ERR_OVERFLOW, nothing copied.
 * AISX_ERR_INVALID after a bad count, as aisx_track_batch_read. */
int aisx_track_batch_read_changed(aisx_track_batch* h, int* idx, int32_t* cols, long col_stride, char* strs, int cap,
                                  int* nchanged, void* stream);

/* ------------------------------------------------------------------------ */
/* PDUs heard by several receivers: keep the first copy of a payload, count   */
/* the others -- on the host (the specification), and in device memory,       */
/* queued between a producer of a PDU list and every stage behind it          */
/* ------------------------------------------------------------------------ */
/* The key of a payload, 64 bits, computed in arithmetic modulo 2^64:
 *     h = 0x9E3779B97F4A7C15 ^ ((uint64_t)len * 0xFF51AFD7ED558CCD)
 *     for k = 0 .. ceil(len / 8) - 1:   w = octets 8 k .. 8 k + 7 as one little-endian word (octets at or beyond len: 0)
 *                                       h = (h ^ w) * 0x9FB21C651E98DF25;   h ^= h >> 32
 *     h ^= h >> 29;   h *= 0xBF58476D1CE4E5B9;   h ^= h >> 32;   a result of 0 is replaced by 1
 * (0 marks a free slot of the device form's hashes and is never a key.)  Every step is one-to-one in h and in w, so two
 * payloads of one length that differ in octets of exactly one word share a key only where the replacement of 0 merges
 * them; all other pairs share one with the probability of a 64-bit hash.  Two payloads are "the same" when their keys are equal: the bytes are not compared.
 * AISX_ERR_INVALID for len < 0 or a missing pointer. */
int aisx_dedup_key(const uint8_t* pdu, int len, uint64_t* key);
/* what an update reports: int counts[AISX_DEDUP_NCNT] */
enum {
    AISX_DEDUP_CNT_IN = 0,     /* records of the call */
    AISX_DEDUP_CNT_KEPT,       /* records kept (bad records included) */
    AISX_DEDUP_CNT_DUP_CALL,   /* suppressed: the key was kept earlier in this call */
    AISX_DEDUP_CNT_DUP_WINDOW, /* suppressed: the key is remembered from an earlier call inside the window */
    AISX_DEDUP_CNT_BAD_LEN,    /* records whose len is outside [0, length_max - 1]: kept, not keyed */
    AISX_DEDUP_NCNT
};
/* A handle remembers the keys it kept, each with the stamp of the call that kept it.  Calls carry a stamp that must be
 * strictly greater than the previous call's (AISX_ERR_OUT_OF_RANGE otherwise: nothing changes, the outputs are not
 * written); stamps are compared and subtracted in 64 bits, so any int32 values do.  0 <= window <= 15, 2 <= length_max
 * <= 1024.  An update takes n records (aisx_pdu layout, offsets into `bytes`) in ascending order; for record i:
 *   - len outside [0, length_max - 1]: kept as the next output record j, not keyed, counted in BAD_LEN;
 *     first[i] = j, copies[j] = 1;
 *   - else, its key is remembered from a call with stamp t in [stamp - window, stamp - 1] (there is at most one such
 *     t): suppressed, first[i] = -1 - (stamp - t), counted in DUP_WINDOW;
 *   - else, its key was kept earlier in this call as output record j: suppressed, first[i] = j, copies[j] grows by
 *     one, counted in DUP_CALL;
 *   - else kept as the next output record j: first[i] = j, copies[j] = 1, and the key is remembered with this stamp.
 * A suppressed record never refreshes what is remembered: a payload repeated in every call is delivered once every
 * window + 1 calls.  Outputs: out_pdus [n] the kept records, unchanged and in input order (their offsets still point
 * into `bytes`); first [n]; copies [n] (the first KEPT entries written); with marks [n] (may be NULL: one int32 per
 * record, carried along, for instance the deframer's repair marks) out_marks [n] the kept records' marks.  Any output
 * pointer may be NULL.  Plain C++, no device. */
typedef struct aisx_dedup aisx_dedup;
int aisx_dedup_create(aisx_dedup** h, int window, int length_max);
int aisx_dedup_destroy(aisx_dedup* h);
int aisx_dedup_reset(aisx_dedup* h); /* nothing remembered, any stamp may follow */
int aisx_dedup_update(aisx_dedup* h, const aisx_pdu* pdus, const uint8_t* bytes, int n, const int32_t* marks, int32_t stamp,
                      aisx_pdu* out_pdus, int32_t* first, int32_t* copies, int32_t* out_marks, int* counts);

typedef struct aisx_dedup_batch aisx_dedup_batch;
/* The same on the device that was current here, for at most max_pdus (<= 2^24) records per call: records, first,
 * copies, marks and counts equal the host form's, bit for bit, whatever order the device ran the records in.  The
 * handle owns a ring of window + 1 sets of remembered keys, one per stamp (open addressing, at least 2 * max_pdus slots
 * of 8 bytes each; the set being reused is cleared at the start of a call, a set whose stamp lies outside the window is
 * not looked at), a hash of the same size for the call's own keys, and a workspace in proportion to max_pdus. */
int aisx_dedup_batch_create(aisx_dedup_batch** h, int window, int max_pdus, int length_max);
int aisx_dedup_batch_destroy(aisx_dedup_batch* h);
int aisx_dedup_batch_reset(aisx_dedup_batch* h); /* as aisx_dedup_reset; waits for the work queued before */
/* d_pdus / d_bytes / d_npdus / d_nfound as aisx_nmea_batch_process takes them; d_marks: int32 [records] on the device or
 * NULL.  Queued on `stream`; no host sync, calls of one handle must be ordered.  The stamp rule is the host form's
 * (AISX_ERR_OUT_OF_RANGE: nothing queued).  A record count outside [0, max_pdus] keeps nothing, as a call of no
 * records does, and makes the next read say so. */
int aisx_dedup_batch_process(aisx_dedup_batch* h, const aisx_pdu* d_pdus, const uint8_t* d_bytes, const int* d_npdus,
                             const int* d_nfound, const int32_t* d_marks, int32_t stamp, void* stream);
/* the last call's results in device memory: d_pdus [max_pdus] the kept records; d_bytes the producer's, unchanged;
 * d_count [3 + AISX_DEDUP_NCNT]: [0] = found = records kept + what the producer found beyond the records it handed
 * over (so a deframer's overflow still shows downstream), [1] = records kept, [2] != 0 after a bad count, [3 + c] =
 * count c above; d_first [max_pdus], d_copies [max_pdus], d_marks [max_pdus] (the kept records' marks; not written by
 * a call without marks).  The first three are what every stage behind the deframer takes. */
int aisx_dedup_batch_results_device(const aisx_dedup_batch* h, const aisx_pdu** d_pdus, const uint8_t** d_bytes,
                                    const int** d_count, const int32_t** d_first, const int32_t** d_copies,
                                    const int32_t** d_marks);
/* copies the last call's results to the host (synchronises `stream`): the first min(kept, pdu_cap) records, their
 * copies and marks (either may be NULL), the first min(in, first_cap) entries of first (may be NULL with first_cap 0),
 * counts [AISX_DEDUP_NCNT]; *nfound (may be NULL) as d_count[0].  AISX_ERR_OVERFLOW when not all kept records or not
 * all of first were written, or when the producer found more than it handed over; AISX_ERR_INVALID when a call since
 * the previous read met a bad count (the flag is then cleared). */
int aisx_dedup_batch_read(aisx_dedup_batch* h, aisx_pdu* pdus, int32_t* copies, int32_t* marks, int pdu_cap, int32_t* first,
                          int first_cap, int* counts, int* nfound, void* stream);

/* ------------------------------------------------------------------------ */
/* ais_rx (python/radio.py:40-73) as ONE handle, fed from host memory in the  */
/* source's own sample format: freq_xlating_fir_filter_ccf -> ais_demod ->    */
/* hdlc_deframer_bp -> pdu_to_nmea for nstreams sources at once               */
/* ------------------------------------------------------------------------ */
typedef struct aisx_rx aisx_rx;
/* bits of aisx_rx_pop's *status above the msk status word (AISX_MSK_ST_*, or-ed over channels as the device holds it
 * when the block's tail runs) */
enum {
    AISX_RX_ST_HDLC_OVERFLOW = 0x100, /* more PDUs found than max_pdus_per_block: a prefix was kept */
    AISX_RX_ST_NMEA_OVERFLOW = 0x200, /* fewer records armoured than the deframer kept */
    AISX_RX_ST_BAD_COUNT = 0x400      /* the deframer or the NMEA stage met a count, channel or length out of range */
};
/* nstreams sources at `rate` samples per second, nchan_per_stream centres each (center_freqs [nstreams][nchan], |f| <=
 * rate / 2; designators [nchan_per_stream], 0..16 bytes each: radio.py:88-89 gives {-25e3, +25e3} and {"A", "B"}).
 * Constants as radio.py:47-65: decimation int(rate / 48000) (so rate >= 48000), taps low_pass(1, rate, 11e3, 1e3)
 * unless given (taps == NULL), samples_per_symbol = rate / decimation / 9600, clock recovery gain 0.04 and limit 0.01,
 * fftlen 1024, deframer (11, 64).  Every block is block_items raw items per stream in `fmt` (AISX_FMT_*, with scale
 * and bias as aisx_xlate_process_fmt), a multiple of the decimation, so that every block is block_items / decimation
 * items per channel.  That count need not be a multiple of fftlen: the chain holds the items short of a whole vector
 * back for the next block (stream_to_vector), so a block's text is that of the vectors completed in it, the same with
 * and without look-ahead.  tmpl / ntmpl: the preamble at the demod rate (what ais_demod builds for corr_est).  At most
 * max_pdus_per_block PDUs per block come out.  The handle owns the filter, the four stage handles and their chain,
 * the deframer, the NMEA stage, AISX_CHAIN_DEPTH + 1 row buffers, two raw-input buffers on the device, three pinned
 * host input slots, eight pinned result slots, and three streams of its own beside the chain's four (copy-in, filter,
 * tail): GPU_MAX_HW_QUEUES >= 8 in the environment before the first HIP call lets all seven run side by side.
 * Row s * nchan_per_stream + c of everything downstream (a record's chan) is stream s at centre c.
 * One thread at a time per handle.  The handle belongs to the device that was current here. */
int aisx_rx_create(aisx_rx** h, double rate, int nstreams, int nchan_per_stream, const double* center_freqs,
                   const char* const* designators, int fmt, float scale, float bias, int block_items, const float* taps,
                   int ntaps, const aisx_cf32* tmpl, int ntmpl, int max_pdus_per_block);
int aisx_rx_destroy(aisx_rx* h); /* waits for what is in flight */
/* any pointer may be NULL: the decimation, items per channel and block, channels (nstreams * nchan_per_stream), pinned
 * input slots, result slots, bytes of text a block can give at most */
int aisx_rx_geometry(const aisx_rx* h, int* decim, int* items_per_block, int* nchan, int* input_slots, int* result_slots,
                     long* text_cap);
/* a pinned host slot [nstreams][*stride_items] items for the source to write the next block into (the same slot until
 * it is submitted); blocks the calling thread only while every slot is still being copied from */
int aisx_rx_acquire(aisx_rx* h, void** slot, long* stride_items);
/* The slot acquired last is full: queues its copy to the device (copy stream), its filter call (one block ahead of
 * the chain, so that aisx_chain_step gets its d_in_next) and the chain step, deframer and NMEA stage of the block
 * BEFORE it, whose results go to a pinned result slot on the tail stream.  Returns without waiting for the device.
 * *block (optional) = this block's number, from 0.  When the block before it would need a result slot and all are
 * waiting to be popped: AISX_ERR_OVERFLOW, nothing queued, the slot stays acquired -- pop, then submit again. */
int aisx_rx_submit(aisx_rx* h, long long* block);
/* acquire + memcpy of [nstreams][block_items] items from host_iq (row stride stride_items) + submit */
int aisx_rx_push(aisx_rx* h, const void* host_iq, long stride_items, long long* block);
/* issues the block that is waiting for its successor, without look-ahead (same results); AISX_ERR_OVERFLOW as submit */
int aisx_rx_flush(aisx_rx* h);
/* The oldest finished block not yet popped, in block order: *block its number; its NMEA text, one '\n' after every
 * sentence (*text_len bytes); its records (chan, end_bit counted over the channel's whole bit stream, offset / len of
 * the record's text in `text`); *status (optional) = 0 or the bits above.  wait == 0: *block = -1 when the next block
 * has not finished (or none is issued); wait != 0 blocks the calling thread until it has (*block = -1 when none is
 * issued).  A block stays available until it is popped, whatever has been submitted since.  When the caller's
 * buffers are too small: AISX_ERR_OVERFLOW with *nrecs / *text_len = what is needed, and the block stays. */
int aisx_rx_pop(aisx_rx* h, int wait, long long* block, char* text, long text_cap, long* text_len, aisx_pdu* recs,
                int rec_cap, int* nrecs, int* status);
/* The aisx_rx_enable_* calls below are the handle's options.  They may come in any order: the handle that results is the
 * same.  A call that returns an error leaves the handle as it was, options set earlier included. */
/* Opt-in: from the first block on, the tail stream queues the field decoder (aisx_msg_batch_*) behind the NMEA stage
 * and every result slot also carries the kept records' table.  Only before the first acquire, submit or push
 * (AISX_ERR_INVALID afterwards) -- but on a handle that has messages enabled the call returns AISX_OK at any time and
 * does nothing.  A handle on which this was never called allocates, queues and copies nothing more. */
int aisx_rx_enable_messages(aisx_rx* h);
/* aisx_rx_pop plus the block's table: cols [AISX_MSG_NCOL][col_stride] (col_stride >= rec_cap), strs
 * [rec_cap][AISX_MSG_STR], row i for record i.  The same waiting and overflow rules (the table needs rec_cap rows).
 * AISX_ERR_INVALID on a handle without messages enabled. */
int aisx_rx_pop_messages(aisx_rx* h, int wait, long long* block, char* text, long text_cap, long* text_len, aisx_pdu* recs,
                         int rec_cap, int* nrecs, int32_t* cols, long col_stride, char* strs, int* status);
/* Opt-in: the handle's deframer repairs by these rules as aisx_hdlc_batch_set_repair describes, and every result slot
 * also carries the block's marks.  Only before the first acquire, submit or push (AISX_ERR_INVALID afterwards, and for
 * bad rules or none); until then it may be called again, and the rules (and events) of the last call hold.  A handle on
 * which this was never called allocates, queues and copies nothing more.  The same as aisx_rx_enable_repair_events
 * with AISX_HDLC_EV_SINGLE. */
int aisx_rx_enable_repair(aisx_rx* h, const aisx_hdlc_rule* rules, int nrules);
/* aisx_rx_enable_repair with aisx_hdlc_batch_set_repair_events' mask of error events, under the same
 * before-the-first-block rule (AISX_ERR_INVALID also for a bad mask; the handle stays as it was). */
int aisx_rx_enable_repair_events(aisx_rx* h, const aisx_hdlc_rule* rules, int nrules, int events);
/* the marks of the block popped last (by aisx_rx_pop or aisx_rx_pop_messages), one per record of that block: *n of
 * them, the first min(*n, cap) written (AISX_ERR_OVERFLOW when cap is less): -1, or first flipped bit's index |
 * event id << 16 (aisx_hdlc_work_repair).  Valid until the next pop; *n = 0 before the first.  AISX_ERR_INVALID on a
 * handle without repair enabled. */
int aisx_rx_popped_repairs(aisx_rx* h, int32_t* fix_bits, int cap, int* n);
/* Opt-in, and implies aisx_rx_enable_messages: the handle also owns a vessel table of `capacity` vessels
 * (aisx_track_batch_*, max_rows = max_pdus_per_block), and from the first block on the tail stream queues its update
 * behind the field decoder, with stamp = the block's number (its low 32 bits) and the deframer's records for CHAN.
 * Only before the first acquire, submit or push (AISX_ERR_INVALID afterwards); a handle on which this was never called
 * allocates and queues nothing more.  The result slots do not carry the changed list: it is read on request. */
int aisx_rx_enable_tracks(aisx_rx* h, int capacity);
/* aisx_track_batch_read / aisx_track_batch_read_changed of the handle's table, queued on the tail stream (so behind
 * the update of every block issued so far; the calling thread waits for them): *block (optional) = the number of the
 * last block whose update the result includes, -1 before the first.  aisx_rx_read_changed_tracks gives that block's
 * changed list.  AISX_ERR_INVALID on a handle without tracks enabled. */
int aisx_rx_read_tracks(aisx_rx* h, int first, int n, int32_t* cols, long col_stride, char* strs, int* nvessels,
                        long long* block);
int aisx_rx_read_changed_tracks(aisx_rx* h, int* idx, int32_t* cols, long col_stride, char* strs, int cap, int* nchanged,
                                long long* block);
/* Opt-in: the bits the deframer reads are decided by the 4-state sequence detector (aisx_mlse_batch_*, below) of BT = bt
 * GMSK instead of the one-symbol slicer.  From the first block on every chain step also writes its symbols (one of
 * AISX_CHAIN_DEPTH buffers of the handle's), and the tail stream queues the detector between the step and the deframer,
 * which takes the detector's longer calls (max_bits + 79).  Deframer, repair (the rules and events of
 * aisx_rx_enable_repair / _events, set before or after this call), NMEA, decoder and vessel table work behind it as they do
 * without it, and a record's end_bit counts the same
 * bits: bit n belongs to symbol n.  The detector decides a symbol once 80 to 143 later ones have arrived, so the last
 * 16 to 79 symbols of a channel stay undecided until more input follows; aisx_rx_flush does not flush the detector
 * (input may follow), and a burst that ends within them appears with the next block.  Only before the first
 * acquire, submit or push (AISX_ERR_INVALID afterwards, and for bt outside [0.1, 1]); a handle on which this was never
 * called allocates, queues and copies nothing more. */
int aisx_rx_enable_mlse(aisx_rx* h, double bt);
/* Opt-in: the NMEA stage writes the STANDARD form (aisx_nmea_batch_create_std) in place of the reference's text: rows
 * s * nchan_per_stream + c carry stations[s] (stations: [nstreams], or NULL for none) in their tag blocks, and block b's
 * time is t0 + floor((double)b * block_items / rate), evaluated in double -- or none when t0 < 0.  The message ids run
 * over the handle's blocks in order.  aisx_rx_geometry then reports the larger text capacity of this form; records,
 * decoder, repair, vessel table and detector work as before.  Once, and only before the first acquire, submit or push
 * (AISX_ERR_INVALID afterwards, and for a station that is none); a handle on which this was never called runs what it
 * ran before. */
int aisx_rx_enable_standard_nmea(aisx_rx* h, const char* const* stations, int64_t t0);
/* Opt-in: the tail stream queues the duplicate suppression (aisx_dedup_batch_*, max_pdus = max_pdus_per_block,
 * remembering `window` blocks, 0..15) between the deframer and the NMEA stage, with stamp = the block's number (its low
 * 32 bits) and, with repair enabled, the deframer's marks carried along.  NMEA stage, decoder and vessel table read the
 * kept records in place of the deframer's: popped records, text, messages and aisx_rx_popped_repairs' marks are those
 * of the kept records, and the table's COUNT counts transmissions, not receptions.  AISX_RX_ST_NMEA_OVERFLOW then means
 * fewer records armoured than kept.  Once, and only before the first acquire, submit or push (AISX_ERR_INVALID
 * afterwards, and for a window outside [0, 15]); a handle on which this was never called allocates and queues nothing
 * for it. */
int aisx_rx_enable_dedup(aisx_rx* h, int window);
/* the duplicate suppression's counts [AISX_DEDUP_NCNT] of the block popped last (all 0 before the first pop).
 * AISX_ERR_INVALID on a handle without dedup enabled. */
int aisx_rx_popped_dedup(aisx_rx* h, int* counts);
/* from the next submitted block on (aisx_xlate_set_center_freq of the handle's filter) */
int aisx_rx_set_center_freq(aisx_rx* h, int stream, int chan, double center_freq);
/* A failed block (a HIP error, the chain refusing) makes every later call but destroy return that block's error. */

/* ------------------------------------------------------------------------ */
/* the transmit side: HDLC framing (the inverse of aisx_hdlc_work) and a      */
/* GMSK burst modulator defined per output sample, on the host (the           */
/* specification, in double) and batched on the device                        */
/* ------------------------------------------------------------------------ */
/* Payload octets -> the burst's NRZ symbol levels, one 0 / 1 per byte of `levels`:
 *   ramp_syms alternating symbols 1, 0, 1, ... ;
 *   training_bits symbols 1, 1, 0, 0, 1, 1, ... (the NRZI image of 0101...; 28 is what the receiver's template holds,
 *   24 the ITU-R M.1371 value);
 *   flag 0x7E + [payload bits, LSB first per octet, + CRC-16/X.25 FCS, low octet first; a 0 stuffed behind every five
 *   1s] + flag 0x7E, NRZI-encoded (a 0 toggles the level, a 1 keeps it) starting from the training sequence's last level;
 *   tail_syms repeats of the last level.
 * 1 <= len <= 1023; 0 <= ramp_syms, tail_syms <= 64; 1 <= training_bits <= 256.  *nsyms = symbols of the burst; when
 * cap is smaller, AISX_ERR_OVERFLOW and nothing written (levels may then be NULL). */
int aisx_hdlc_frame(const uint8_t* payload, int len, int training_bits, int ramp_syms, int tail_syms, uint8_t* levels,
                    int cap, int* nsyms);

typedef struct aisx_burst {
    int64_t start;   /* row sample index at which symbol 0 begins */
    int64_t offset;  /* first payload octet in the byte buffer */
    int32_t chan, len;
    float frac;      /* extra delay in samples, [0, 1) */
    float amp;
    float cfo;       /* cycles per sample, |cfo| <= 0.5 */
    float phase;     /* radians */
} aisx_burst;

/* The waveform.  With a_k = +-1 the burst's levels (0 outside it), L = 4, d = t - start, u = (d - frac) / sps and
 * m = floor(u), sample t of a burst is
 *   x(t) = amp env(u) exp(j [ (pi/2) ( S(m - L) + sum_{k = m-L+1 .. m} a_k q(u - k) ) + 2 pi cfo d + phase ])
 * where S(i) = a_0 + ... + a_i (an integer: (pi/2) S is an exact quadrant), env(u) = min(1, u / r, (nsyms - u) / r) with
 * r = ramp_syms / 2 symbols (1 when ramp_syms = 0), and q the phase pulse of BT = bt GMSK, truncated to L symbols:
 *   beta = pi bt sqrt(2 / ln 2),   F(x) = x erf(beta x) + exp(-beta^2 x^2) / (beta sqrt(pi)),
 *   G(x) = 1/2 + (F(x + 1/2) - F(x - 1/2)) / 2      (the integral of a Gaussian convolved with a one-symbol rectangle),
 *   q(v) = (G(v - L/2) - G(-L/2)) / (G(L/2) - G(-L/2)) for 0 <= v <= L,   0 below,   1 above
 * so that q(0) = 0 and q(L) = 1 exactly and x is continuous in u.  The burst occupies the samples with
 * 0 <= u < nsyms; bursts that overlap in a channel add.  No sample depends on another.
 *
 * aisx_tx_render_host evaluates this in double for rows [nchan][n] of the sample window [t0, t0 + n), sums a sample's
 * bursts in double and rounds once to float; accumulate != 0 adds that float to what out holds.  sps >= 2 (any real
 * number), 0.1 <= bt <= 1, framing arguments as aisx_hdlc_frame's, descriptors as aisx_tx_batch_set_bursts checks
 * them (length_max = 1023). */
int aisx_tx_render_host(double sps, double bt, int training_bits, int ramp_syms, int tail_syms, int nchan,
                        const aisx_burst* bursts, int nbursts, const uint8_t* bytes, int64_t nbytes, int64_t t0, int64_t n,
                        aisx_cf32* out, int64_t out_stride, int accumulate);

/* The same on the device, for a schedule of at most max_bursts bursts of at most length_max payload octets on nchan
 * channels.  The handle belongs to the device that was current here. */
typedef struct aisx_tx_batch aisx_tx_batch;
int aisx_tx_batch_create(aisx_tx_batch** h, double sps, double bt, int training_bits, int ramp_syms, int tail_syms,
                         int nchan, int max_bursts, int length_max);
int aisx_tx_batch_destroy(aisx_tx_batch* h);
/* Replaces the schedule (bursts and bytes are host memory, free again at return; n = 0 empties it).  Checked on the
 * host: chan in [0, nchan), 1 <= len <= length_max, offset >= 0 and offset + len <= nbytes, frac in [0, 1), amp and phase
 * finite, |cfo| <= 0.5, |start| < 2^62, n <= max_bursts -- AISX_ERR_INVALID otherwise, and the schedule stays what it
 * was.  Waits for the handle's last render, uploads the bursts sorted by (chan, start, frac) and queues k_tx_frame on
 * `stream`: one wave per burst frames its payload into packed levels and per-word level counts. */
int aisx_tx_batch_set_bursts(aisx_tx_batch* h, const aisx_burst* bursts, int n, const uint8_t* bytes, int64_t nbytes,
                             void* stream);
/* Queues k_tx_render on `stream`: rows [nchan][n] at d_out (row stride out_stride >= n items, 8-byte aligned) for the
 * sample window [t0, t0 + n), 1 <= n <= 2^30.  accumulate == 0: every sample is written, zeros where no burst is;
 * accumulate != 0: out = out + (the sum of the sample's bursts), nothing written where no burst is near.  Stateless
 * in t0: the rows of one call and of any split of its window into calls are bit-identical. */
int aisx_tx_batch_render(aisx_tx_batch* h, int64_t t0, int64_t n, aisx_cf32* d_out, int64_t out_stride, int accumulate,
                         void* stream);
/* test and inspection hook: the levels k_tx_frame made for burst `index` (in the order they were given to
 * aisx_tx_batch_set_bursts), unpacked to one 0 / 1 per byte; synchronises `stream`.  *nsyms = the device's symbol
 * count; AISX_ERR_OVERFLOW when cap is smaller (nothing written). */
int aisx_tx_batch_read_levels(aisx_tx_batch* h, int index, uint8_t* levels, int cap, int* nsyms, void* stream);

/* ------------------------------------------------------------------------ */
/* 4-state sequence detector behind the timing recovery: the recovery's       */
/* symbols (one per symbol) to the bit stream the bit tail produces (NRZI     */
/* decoded, inverted; bit n belongs to symbol n), the levels decided by a     */
/* Viterbi search over the differential phase instead of one phase step each. */
/* On the host (the specification) and batched on the device, bit for bit.    */
/* ------------------------------------------------------------------------ */
/* Per channel: symbols s[0], s[1], ... with s[-1] = 0; z[n] = s[n] conj(s[n-1]), re = fma(a.im, b.im, a.re * b.re),
 * im = fma(a.im, b.re, -(a.re * b.im)) for a = s[n], b = s[n-1].  Levels b in {0, 1}, X = 2 x - 1 (1: a positive
 * phase step, as the slicer's).  z[n] turns by
 *     theta(p, q, r) = (pi/2) (c0 Q + c1 (P + R))      for (b[n-1], b[n], b[n+1]) = (p, q, r),
 * c0 = q(2.5) - q(1.5), c1 = q(3.5) - q(2.5) of the transmitter's L = 4 phase pulse q (above) at the handle's bt, in
 * double: 0.735928 and 0.131918 at bt = 0.4.  rot[p][q][r] = ((float)cos theta, (float)sin theta) is made once.
 * Branch metric g(n; p, q, r) = fma(z.im, sin, z.re * cos), in float.
 * Blocks of 64 symbols by absolute index, 16 symbols of overlap on each side: block k covers [64 k, 64 k + 64), its
 * window is [a, e) with a = max(0, 64 k - 16) and e = 64 k + 80 (at a flush min(64 k + 80, N), N = symbols seen).  All four
 * path metrics M[2 p + q], of (b[n-1], b[n]) = (p, q), are 0 entering step a.  Step n, for every (q, r):
 *     cand_p = M[2 p + q] + g(n; p, q, r),   the survivor is p = 1 exactly when cand_1 > cand_0,   M'[2 q + r] = its candidate
 * (compare and select, float, nothing renormalised).  Behind step e - 1 the best state is the lowest index whose metric
 * is the greatest; back from it, the state (q, r) of step n gives b[n] = q and its survivor the state of step n - 1,
 * down to b[64 k - 1] (b[-1] = 0).  bit[n] = 1 ^ b[n] ^ b[n-1] for the block's n: no block needs another's decision.
 * Block k is emitted as soon as 64 k + 80 <= N; the undecided symbols are carried (at most 96).  The concatenated output
 * is therefore the same for every split of a stream into calls.  A call of n symbols emits at most n + 79 bits. */
typedef struct aisx_mlse aisx_mlse;
int aisx_mlse_create(aisx_mlse** h, double bt); /* 0.1 <= bt <= 1 */
int aisx_mlse_destroy(aisx_mlse* h);
int aisx_mlse_reset(aisx_mlse* h);
/* c0, c1 and rot[16] = {cos, sin} of the triples in the order 4 p + 2 q + r; any pointer may be NULL */
int aisx_mlse_model(const aisx_mlse* h, double* c0, double* c1, float* rot);
/* n >= 0 symbols in, *nbits bits (one per byte) out; AISX_ERR_OVERFLOW with *nbits = what is needed when cap is
 * smaller: nothing was taken then */
int aisx_mlse_work(aisx_mlse* h, const aisx_cf32* syms, int n, uint8_t* bits, int cap, int* nbits);
/* the bits of the symbols still undecided (at most 79), their windows cut at the last symbol; leaves the handle as
 * after reset */
int aisx_mlse_flush(aisx_mlse* h, uint8_t* bits, int cap, int* nbits);

/* The same for nchan channels of at most max_syms (<= 2^27) symbols per call on the device: per channel exactly what
 * one aisx_mlse handle returns when fed that channel's symbols call by call.  The handle belongs to the device that was
 * current here. */
typedef struct aisx_mlse_batch aisx_mlse_batch;
int aisx_mlse_batch_create(aisx_mlse_batch** h, double bt, int nchan, int max_syms);
int aisx_mlse_batch_destroy(aisx_mlse_batch* h);
int aisx_mlse_batch_reset(aisx_mlse_batch* h); /* back to the state after create; waits for the last call's work */
/* d_syms [nchan][syms_stride] (syms_stride >= max_syms, 8-byte aligned), d_nsyms [nchan] on the DEVICE (the chain's
 * d_produced); d_bits [nchan][bits_stride] with bits_stride >= max_syms + 79 and d_nbits [nchan] receive what
 * aisx_hdlc_batch_process consumes.  Queued on `stream`, no host synchronisation; calls of one handle must be ordered.
 * A channel whose count is outside [0, max_syms] is treated as one with no new symbols, and the status says so. */
int aisx_mlse_batch_process(aisx_mlse_batch* h, const aisx_cf32* d_syms, long syms_stride, const int* d_nsyms,
                            uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream);
/* aisx_mlse_flush for every channel (bits_stride >= 79), queued on `stream` */
int aisx_mlse_batch_flush(aisx_mlse_batch* h, uint8_t* d_bits, long bits_stride, int* d_nbits, void* stream);
enum { AISX_MLSE_ST_BAD_COUNT = 1 };
/* *status = 0 or AISX_MLSE_ST_BAD_COUNT when a call since the previous read met a bad count (then cleared);
 * synchronises `stream`.  _status_device: the word itself, for a consumer on the device. */
int aisx_mlse_batch_status(aisx_mlse_batch* h, int* status, void* stream);
int aisx_mlse_batch_status_device(const aisx_mlse_batch* h, const int** d_status);

#ifdef __cplusplus
}
#endif
#endif /* AISX_H */
