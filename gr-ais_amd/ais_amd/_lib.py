"""ctypes loader for libaisx.so (the HIP kernels + C ABI, include/aisx.h).

There is deliberately no fallback: if the shared library is missing the import
fails, and if no MI355X is visible every block constructor raises.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# The product library reads no environment variable.  lib/libaisx_exp.so is the same code built with -DAISX_EXPERIMENTS
# (alternative kernels, AISX_* knobs): a process asks for it BEFORE the first call with AISX_LIB_VARIANT=exp (the twin tests
# under tests/exp_builds/, tools/ab_bench.py) -- a choice of this loader, not of the library.
LIB_VARIANT = os.environ.get("AISX_LIB_VARIANT", "")
LIB_PATH = os.path.join(os.path.dirname(_PKG), "lib", "libaisx_exp.so" if LIB_VARIANT == "exp" else "libaisx.so")

AISX_OK = 0
AISX_ERR_INVALID = -1
AISX_ERR_OUT_OF_RANGE = -2
AISX_ERR_HIP = -3
AISX_ERR_NO_DEVICE = -4
AISX_ERR_OVERFLOW = -5
AISX_ERR_RUNTIME = -6

AISX_FMT_CF32, AISX_FMT_CS16, AISX_FMT_CS8, AISX_FMT_CU8 = 0, 1, 2, 3
AISX_RX_ST_HDLC_OVERFLOW, AISX_RX_ST_NMEA_OVERFLOW, AISX_RX_ST_BAD_COUNT = 0x100, 0x200, 0x400
AISX_MSG_NA, AISX_MSG_STR = -(1 << 31), 48
AISX_HDLC_MAX_RULES = 16
AISX_HDLC_EV_SINGLE, AISX_HDLC_EV_PAIR, AISX_HDLC_EV_SKIP = 1, 2, 4  # error events of the deframers' repair
AISX_MLSE_ST_BAD_COUNT = 1
MLSE_BLOCK, MLSE_OVERLAP = 64, 16  # symbols a block of the sequence detector decides, and its window's overlap
AISX_MSG_FL_COMPLETE, AISX_MSG_FL_NO_LAYOUT, AISX_MSG_FL_BAD_RECORD = 1, 2, 4
AISX_MSG_ENC_NO_MMSI, AISX_MSG_ENC_NO_LAYOUT, AISX_MSG_ENC_RANGE, AISX_MSG_ENC_BAD_CHAR, AISX_MSG_ENC_BAD_ROW = 1, 2, 4, 8, 16
AISX_MSG_ENC_PITCH = 56  # octets between the payloads of two records of aisx_msg_enc_batch's list
AISX_NMEA_PARSE_REF_TAIL = 1
# what a call of the NMEA parsers reports (include/aisx.h, AISX_NMEAP_*), in order
AISX_NMEAP_NAMES = ("FOUND", "KEPT", "BAD_INPUT", "LINES", "SENTENCES", "REJ_FORMAT", "REJ_CHECKSUM", "REJ_CHANNEL",
                    "REJ_ARMOUR", "REJ_FRAGMENT", "REJ_LENGTH", "CARRIED")
AISX_NMEAP_NCNT = len(AISX_NMEAP_NAMES)

KEY_CORR_START, KEY_PHASE_EST, KEY_TIME_EST, KEY_CORR_EST, KEY_PORT1 = 0, 1, 2, 3, 0x100
KEY_NAMES = {0: "corr_start", 1: "phase_est", 2: "time_est", 3: "corr_est"}


class AisxError(RuntimeError):
    pass


class NoDeviceError(AisxError):
    pass


_lib = None
_torch_first = False


def lib(device=True):
    """libaisx.so, loaded once.  device=False: a host-only helper is asking (HDLC deframer, NMEA: plain C++
    in the same library) -- torch is then not imported on its account."""
    global _lib, _torch_first
    if _lib is not None:
        if device and not _torch_first:
            import sys
            import warnings

            if "torch" not in sys.modules:
                warnings.warn("ais_amd: libaisx.so was loaded by a host-only helper before torch; torch ships its own copy of "
                              "the HIP runtime, and a process with two of them may see no device through the second: import "
                              "torch (or ais_amd.blocks) first in processes that use both", RuntimeWarning, stacklevel=2)
            _torch_first = True  # (say it once)
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libaisx.so not built (%s): run `make -C gr-ais_amd` or __graft_entry__.build(); "
            "there is no CPU fallback" % LIB_PATH)
    # torch ships its own copy of the HIP runtime: load it FIRST, so that libaisx.so binds to the
    # runtime that owns the devices torch hands out pointers of (the other order leaves this
    # process with two runtimes, and the second one sees no device)
    import sys

    if device or "torch" in sys.modules:
        try:
            import torch  # noqa: F401

            _torch_first = True
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, f32, f64, u64, lng = C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_double, C.c_uint64, C.c_long
    pvp, pi32 = C.POINTER(C.c_void_p), C.POINTER(C.c_int)

    def sig(name, res, args):
        f = getattr(L, name)  # AttributeError = libaisx.so is older than this binding: rebuild
        f.restype = res
        f.argtypes = args

    sig("aisx_version", i32, [])
    sig("aisx_last_error", C.c_char_p, [])
    sig("aisx_device_count", i32, [pi32])
    sig("aisx_set_device", i32, [i32])
    sig("aisx_util_copy_GBs", i32, [C.c_size_t, i32, C.POINTER(C.c_float)])
    sig("aisx_util_agc_rcp_mismatches", i32, [f32, C.POINTER(C.c_ulonglong), C.POINTER(C.c_float)])
    sig("aisx_corr_create", i32, [pvp, vp, i32, f32, u32, f32, i32, i32, i32])
    sig("aisx_corr_destroy", i32, [vp])
    sig("aisx_corr_symbols", i32, [vp, vp, i32])
    sig("aisx_corr_set_symbols", i32, [vp, vp, i32])
    sig("aisx_corr_geometry", i32, [vp, pi32, pi32])
    sig("aisx_corr_history", i32, [vp])
    sig("aisx_corr_output_multiple", i32, [vp])
    sig("aisx_corr_max_noutput_items", i32, [vp])
    sig("aisx_corr_threshold", f32, [vp])
    sig("aisx_corr_mark_delay", u32, [vp])
    sig("aisx_corr_nitems_written", u64, [vp])
    sig("aisx_corr_reset", i32, [vp])
    sig("aisx_corr_process", i32, [vp, vp, lng, vp, lng, vp, lng, i32, vp])
    sig("aisx_corr_set_lds_claim", i32, [vp, i32])
    sig("aisx_corr_get_lds_claim", i32, [vp, pi32, pi32])
    sig("aisx_corr_set_profiling", i32, [vp, i32])
    sig("aisx_corr_last_kernel_ms", i32, [vp, C.POINTER(C.c_float)])
    sig("aisx_corr_kernel_ms_history", i32, [vp, C.POINTER(C.c_float), i32, pi32])
    sig("aisx_corr_tags_device", i32, [vp, pvp, pvp, pi32])
    sig("aisx_corr_read_tags", i32, [vp, vp, i32, pi32, vp])
    sig("aisx_corr_read_tags_back", i32, [vp, i32, vp, i32, pi32, vp])
    sig("aisx_corr_work_host", i32, [vp, vp, vp, vp, i32, u64, vp, i32, pi32])
    sig("aisx_msk_create", i32, [pvp, f32, f32, f32, i32, i32, i32])
    sig("aisx_msk_destroy", i32, [vp])
    sig("aisx_msk_set_gain", i32, [vp, f32])
    sig("aisx_msk_get_gain", f32, [vp])
    sig("aisx_msk_set_limit", i32, [vp, f32])
    sig("aisx_msk_get_limit", f32, [vp])
    sig("aisx_msk_set_sps", i32, [vp, f32])
    sig("aisx_msk_get_sps", f32, [vp])
    sig("aisx_msk_forecast", i32, [vp, i32])
    sig("aisx_msk_out_capacity", i32, [vp])
    sig("aisx_msk_reset", i32, [vp])
    sig("aisx_msk_process_stream", i32, [vp, vp, lng, i32, vp, vp, i32, vp, vp, vp, vp, lng, vp, vp])
    sig("aisx_msk_process_stream_after", i32, [vp, vp, lng, i32, vp, vp, i32, vp, vp, vp, vp, lng, vp, vp, vp])
    sig("aisx_msk_last_status", i32, [vp, pi32, vp])
    sig("aisx_msk_restart_stats", i32, [vp, vp, vp])
    sig("aisx_msk_set_profiling", i32, [vp, i32])
    sig("aisx_msk_kernel_ms_history", i32, [vp, C.POINTER(C.c_float), i32, pi32])
    sig("aisx_msk_set_max_noutput_items", i32, [vp, i32])
    sig("aisx_msk_set_time_parallel", i32, [vp, i32, i32, i32])
    sig("aisx_msk_get_max_noutput_items", i32, [vp])
    sig("aisx_msk_set_tail_stream", i32, [vp, vp, i32])
    sig("aisx_msk_wait_tail", i32, [vp, vp])
    sig("aisx_msk_set_fused_tail", i32, [vp, i32])
    sig("aisx_msk_get_fused_tail", i32, [vp])
    sig("aisx_msk_set_pair_core", i32, [vp, i32])
    sig("aisx_msk_get_pair_core", i32, [vp])
    sig("aisx_msk_last_tail_fused", i32, [vp])
    sig("aisx_msk_wait_prepass", i32, [vp, vp])
    sig("aisx_msk_set_head_start", i32, [vp, i32])
    sig("aisx_msk_geometry", i32, [vp, pi32, pi32])
    sig("aisx_msk_general_work_host", i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, u64, i32, pi32, pi32])
    sig("aisx_freqsync_create", i32, [pvp, f64, f64, i32, i32, i32])
    sig("aisx_freqest_create", i32, [pvp, f32, i32, i32, i32])
    sig("aisx_freqest_create_n", i32, [pvp, f32, i32, i32, i32, i32])
    sig("aisx_freqsync_is_estimator_only", i32, [vp])
    sig("aisx_freqsync_geometry", i32, [vp, pi32, pi32, pi32])
    sig("aisx_freqsync_drop_ahead", i32, [vp, vp])
    sig("aisx_freqsync_destroy", i32, [vp])
    sig("aisx_freqsync_reset", i32, [vp])
    sig("aisx_freqsync_process", i32, [vp, vp, lng, i32, vp, lng, vp, lng, pi32, vp])
    sig("aisx_freqest_work", i32, [vp, vp, lng, vp, lng, i32, vp])
    sig("aisx_freqest_work_host", i32, [vp, i32, vp, vp])
    sig("aisx_freqsync_work_host", i32, [vp, vp, i32, vp, i32, vp, i32])
    sig("aisx_agc_work_host", i32, [vp, i32, vp, vp])
    sig("aisx_freqsync_agc_process", i32, [vp, vp, vp, lng, i32, vp, lng, vp, lng, pi32, vp])
    sig("aisx_freqsync_estimate_ahead", i32, [vp, vp, lng, i32, vp, vp])
    sig("aisx_agc_create", i32, [pvp, i32, f32, i32, i32])
    sig("aisx_agc_destroy", i32, [vp])
    sig("aisx_agc_geometry", i32, [vp, pi32, pi32, pi32, pi32])
    sig("aisx_agc_reset", i32, [vp])
    sig("aisx_agc_set_floor", i32, [vp, f32])
    sig("aisx_agc_set_streaming", i32, [vp, i32])
    sig("aisx_agc_set_lds_claim", i32, [vp, i32])
    sig("aisx_agc_get_lds_claim", i32, [vp, pi32, pi32])
    sig("aisx_freqsync_set_walk_lds_claim", i32, [vp, i32])
    sig("aisx_freqsync_get_walk_lds_claim", i32, [vp, pi32, pi32])
    sig("aisx_msk_placement", i32, [vp, pi32, pi32])
    sig("aisx_agc_process", i32, [vp, vp, lng, vp, lng, i32, vp])
    sig("aisx_chain_create", i32, [pvp, vp, vp, vp, vp, i32, i32, i32])
    sig("aisx_chain_destroy", i32, [vp])
    sig("aisx_chain_depth", i32, [])
    sig("aisx_chain_step", i32, [vp, vp, lng, i32, vp, lng, i32, vp, vp, lng, vp, vp, C.POINTER(C.c_longlong)])
    sig("aisx_chain_wait", i32, [vp, C.c_longlong, vp, i32])
    sig("aisx_chain_wait_input", i32, [vp, C.c_longlong, vp, i32])
    sig("aisx_chain_synchronize", i32, [vp])
    sig("aisx_chain_read_corr_output", i32, [vp, C.c_longlong, i32, i32, vp, lng, pi32, vp])
    sig("aisx_chain_read_tags", i32, [vp, C.c_longlong, vp, i32, pi32, vp])
    sig("aisx_chain_stream", vp, [vp, i32])
    sig("aisx_pfb_create", i32, [pvp, i32, i32, vp, i32, i32, i32])
    sig("aisx_pfb_destroy", i32, [vp])
    sig("aisx_pfb_process", i32, [vp, vp, lng, i32, vp, lng, pi32, vp])
    pf64 = C.POINTER(C.c_double)
    sig("aisx_xlate_create", i32, [pvp, i32, vp, i32, vp, i32, f64, i32, i32])
    sig("aisx_xlate_destroy", i32, [vp])
    sig("aisx_xlate_reset", i32, [vp])
    sig("aisx_xlate_geometry", i32, [vp, pi32, pi32, pi32, pi32, pi32])
    sig("aisx_xlate_set_center_freq", i32, [vp, i32, i32, f64])
    sig("aisx_xlate_center_freq", i32, [vp, i32, i32, pf64])
    sig("aisx_xlate_output_count", i32, [vp, i32])
    sig("aisx_xlate_process", i32, [vp, vp, lng, i32, vp, lng, pi32, vp])
    sig("aisx_xlate_process_fmt", i32, [vp, vp, i32, f32, f32, lng, i32, vp, lng, pi32, vp])
    sig("aisx_msk_status_device", i32, [vp, pvp])
    pll, plng = C.POINTER(C.c_longlong), C.POINTER(C.c_long)
    sig("aisx_rx_create", i32, [pvp, f64, i32, i32, vp, C.POINTER(C.c_char_p), i32, f32, f32, i32, vp, i32, vp, i32, i32])
    sig("aisx_rx_destroy", i32, [vp])
    sig("aisx_rx_geometry", i32, [vp, pi32, pi32, pi32, pi32, pi32, plng])
    sig("aisx_rx_acquire", i32, [vp, pvp, plng])
    sig("aisx_rx_submit", i32, [vp, pll])
    sig("aisx_rx_push", i32, [vp, vp, lng, pll])
    sig("aisx_rx_flush", i32, [vp])
    sig("aisx_rx_pop", i32, [vp, i32, pll, vp, lng, plng, vp, i32, pi32, pi32])
    sig("aisx_rx_set_center_freq", i32, [vp, i32, i32, f64])
    sig("aisx_hdlc_create", i32, [pvp, i32, i32])
    sig("aisx_hdlc_destroy", i32, [vp])
    sig("aisx_hdlc_work", i32, [vp, vp, i32, vp, i32, vp, i32, pi32])
    sig("aisx_hdlc_set_repair", i32, [vp, vp, i32])
    sig("aisx_hdlc_work_repair", i32, [vp, vp, i32, vp, i32, vp, vp, i32, pi32])
    sig("aisx_hdlc_set_repair_events", i32, [vp, vp, i32, i32])
    sig("aisx_hdlc_event_table", i32, [i32, vp])
    sig("aisx_pdu_to_nmea", i32, [C.c_char_p, vp, i32, C.c_char_p, i32])
    sig("aisx_hdlc_batch_create", i32, [pvp, i32, i32, i32, i32, i32])
    sig("aisx_hdlc_batch_destroy", i32, [vp])
    sig("aisx_hdlc_batch_reset", i32, [vp])
    sig("aisx_hdlc_batch_process", i32, [vp, vp, lng, vp, vp])
    sig("aisx_hdlc_batch_results_device", i32, [vp, pvp, pvp, pvp])
    sig("aisx_hdlc_batch_read", i32, [vp, vp, i32, vp, lng, pi32, vp])
    sig("aisx_hdlc_batch_set_repair", i32, [vp, vp, i32])
    sig("aisx_hdlc_batch_repairs_device", i32, [vp, pvp])
    sig("aisx_hdlc_batch_read_repairs", i32, [vp, vp, i32, pi32, vp])
    sig("aisx_rx_enable_repair", i32, [vp, vp, i32])
    sig("aisx_hdlc_batch_set_repair_events", i32, [vp, vp, i32, i32])
    sig("aisx_rx_enable_repair_events", i32, [vp, vp, i32, i32])
    sig("aisx_rx_popped_repairs", i32, [vp, vp, i32, pi32])
    sig("aisx_nmea_batch_create", i32, [pvp, C.POINTER(C.c_char_p), i32, i32, i32, lng])
    sig("aisx_nmea_batch_destroy", i32, [vp])
    sig("aisx_nmea_batch_process", i32, [vp, vp, vp, vp, vp, vp])
    sig("aisx_nmea_batch_results_device", i32, [vp, pvp, pvp, pvp])
    sig("aisx_nmea_batch_read", i32, [vp, vp, i32, vp, lng, pi32, pi32, vp])
    sig("aisx_pdu_to_nmea_std", i32, [C.c_char_p, vp, i32, i32, C.c_char_p, C.c_int64, C.c_char_p, i32])
    sig("aisx_nmea_std_text_len", i32, [i32, i32, i32, C.c_int64])
    sig("aisx_nmea_batch_create_std", i32, [pvp, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32, i32, i32, lng])
    sig("aisx_nmea_batch_set_time", i32, [vp, C.c_int64])
    sig("aisx_nmea_batch_reset", i32, [vp])
    sig("aisx_nmea_batch_next_id", i32, [vp, pi32, vp])
    ppc = C.POINTER(C.c_char_p)
    sig("aisx_nmea_parse_create", i32, [pvp, ppc, i32, i32, i32, i32])
    sig("aisx_nmea_parse_destroy", i32, [vp])
    sig("aisx_nmea_parse_reset", i32, [vp])
    sig("aisx_nmea_parse_work", i32, [vp, vp, lng, vp, i32, vp, lng, vp, vp])
    sig("aisx_nmea_parse_batch_create", i32, [pvp, ppc, i32, i32, i32, i32, lng, i32, i32])
    sig("aisx_nmea_parse_batch_destroy", i32, [vp])
    sig("aisx_nmea_parse_batch_reset", i32, [vp])
    sig("aisx_nmea_parse_batch_process", i32, [vp, vp, vp, vp])
    sig("aisx_nmea_parse_batch_results_device", i32, [vp, pvp, pvp, pvp, pvp])
    sig("aisx_nmea_parse_batch_read", i32, [vp, vp, i32, vp, lng, vp, vp, vp])
    sig("aisx_msg_decode", i32, [vp, i32, vp, vp])
    sig("aisx_msg_batch_create", i32, [pvp, i32, i32, i32])
    sig("aisx_msg_batch_destroy", i32, [vp])
    sig("aisx_msg_batch_process", i32, [vp, vp, vp, vp, vp, vp])
    sig("aisx_msg_batch_results_device", i32, [vp, pvp, plng, pvp, pvp])
    sig("aisx_msg_batch_read", i32, [vp, vp, lng, vp, i32, pi32, pi32, vp])
    sig("aisx_msg_encode", i32, [vp, vp, i32, i32, vp, i32, pi32, pi32])
    sig("aisx_msg_enc_batch_create", i32, [pvp, i32, i32, i32])
    sig("aisx_msg_enc_batch_destroy", i32, [vp])
    sig("aisx_msg_enc_batch_process", i32, [vp, vp, lng, vp, vp, vp, vp, i32, i32, vp])
    sig("aisx_msg_enc_batch_results_device", i32, [vp, pvp, pvp, pvp, pvp])
    sig("aisx_msg_enc_batch_read", i32, [vp, vp, vp, i32, vp, lng, pi32, vp, vp])
    sig("aisx_rx_enable_messages", i32, [vp])
    sig("aisx_rx_pop_messages", i32, [vp, i32, pll, vp, lng, plng, vp, i32, pi32, vp, lng, vp, pi32])
    sig("aisx_track_create", i32, [pvp, i32])
    sig("aisx_track_destroy", i32, [vp])
    sig("aisx_track_update", i32, [vp, vp, lng, vp, vp, i32, i32, vp])
    sig("aisx_track_expire", i32, [vp, i32, vp])
    sig("aisx_track_data", i32, [vp, pvp, plng, pvp, pi32])
    sig("aisx_track_changed", i32, [vp, pvp, pi32])
    sig("aisx_track_batch_create", i32, [pvp, i32, i32])
    sig("aisx_track_batch_destroy", i32, [vp])
    sig("aisx_track_batch_reset", i32, [vp])
    sig("aisx_track_batch_process", i32, [vp, vp, lng, vp, vp, vp, i32, vp])
    sig("aisx_track_batch_expire", i32, [vp, i32, vp])
    sig("aisx_track_batch_results_device", i32, [vp, pvp, plng, pvp, pvp, pvp])
    sig("aisx_track_batch_read", i32, [vp, i32, i32, vp, lng, vp, pi32, vp])
    sig("aisx_track_batch_counts", i32, [vp, vp, vp])
    sig("aisx_track_batch_read_changed", i32, [vp, vp, vp, lng, vp, i32, pi32, vp])
    sig("aisx_rx_enable_tracks", i32, [vp, i32])
    sig("aisx_rx_read_tracks", i32, [vp, i32, i32, vp, lng, vp, pi32, pll])
    sig("aisx_rx_read_changed_tracks", i32, [vp, vp, vp, lng, vp, i32, pi32, pll])
    sig("aisx_dedup_key", i32, [vp, i32, C.POINTER(u64)])
    sig("aisx_dedup_create", i32, [pvp, i32, i32])
    sig("aisx_dedup_destroy", i32, [vp])
    sig("aisx_dedup_reset", i32, [vp])
    sig("aisx_dedup_update", i32, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp])
    sig("aisx_dedup_batch_create", i32, [pvp, i32, i32, i32])
    sig("aisx_dedup_batch_destroy", i32, [vp])
    sig("aisx_dedup_batch_reset", i32, [vp])
    sig("aisx_dedup_batch_process", i32, [vp, vp, vp, vp, vp, vp, i32, vp])
    sig("aisx_dedup_batch_results_device", i32, [vp, pvp, pvp, pvp, pvp, pvp, pvp])
    sig("aisx_dedup_batch_read", i32, [vp, vp, vp, vp, i32, vp, i32, vp, pi32, vp])
    sig("aisx_rx_enable_dedup", i32, [vp, i32])
    sig("aisx_rx_popped_dedup", i32, [vp, vp])
    i64 = C.c_int64
    sig("aisx_hdlc_frame", i32, [vp, i32, i32, i32, i32, vp, i32, pi32])
    sig("aisx_tx_render_host", i32, [f64, f64, i32, i32, i32, i32, vp, i32, vp, i64, i64, i64, vp, i64, i32])
    sig("aisx_tx_batch_create", i32, [pvp, f64, f64, i32, i32, i32, i32, i32, i32])
    sig("aisx_tx_batch_destroy", i32, [vp])
    sig("aisx_tx_batch_set_bursts", i32, [vp, vp, i32, vp, i64, vp])
    sig("aisx_tx_batch_render", i32, [vp, i64, i64, vp, i64, i32, vp])
    sig("aisx_tx_batch_read_levels", i32, [vp, i32, vp, i32, pi32, vp])
    sig("aisx_mlse_create", i32, [pvp, f64])
    sig("aisx_mlse_destroy", i32, [vp])
    sig("aisx_mlse_reset", i32, [vp])
    sig("aisx_mlse_model", i32, [vp, pf64, pf64, vp])
    sig("aisx_mlse_work", i32, [vp, vp, i32, vp, i32, pi32])
    sig("aisx_mlse_flush", i32, [vp, vp, i32, pi32])
    sig("aisx_mlse_batch_create", i32, [pvp, f64, i32, i32])
    sig("aisx_mlse_batch_destroy", i32, [vp])
    sig("aisx_mlse_batch_reset", i32, [vp])
    sig("aisx_mlse_batch_process", i32, [vp, vp, lng, vp, vp, lng, vp, vp])
    sig("aisx_mlse_batch_flush", i32, [vp, vp, lng, vp, vp])
    sig("aisx_mlse_batch_status", i32, [vp, pi32, vp])
    sig("aisx_mlse_batch_status_device", i32, [vp, pvp])
    sig("aisx_rx_enable_mlse", i32, [vp, f64])
    sig("aisx_rx_enable_standard_nmea", i32, [vp, C.POINTER(C.c_char_p), C.c_int64])
    _lib = L
    return L


def check(rc, what=""):
    """Map a C-ABI status to the exception the reference's Python binding raises."""
    if rc >= 0:
        return rc
    msg = lib().aisx_last_error().decode("utf-8", "replace")
    if rc == AISX_ERR_OUT_OF_RANGE:
        raise IndexError(msg or what)  # SWIG maps std::out_of_range to IndexError
    if rc == AISX_ERR_NO_DEVICE:
        raise NoDeviceError(msg or "no HIP device")
    if rc == AISX_ERR_RUNTIME:
        raise RuntimeError(msg or what)  # std::runtime_error
    if rc == AISX_ERR_INVALID:
        raise ValueError("%s: %s" % (what, msg))
    if rc == AISX_ERR_OVERFLOW:
        raise OverflowError("%s: %s" % (what, msg))
    raise AisxError("%s failed (%d): %s" % (what, rc, msg))
