"""The launch plans of the six batched tail stages (HdlcPlan, MlsePlan, NmeaPlan, NmpPlan, MsgPlan, TrkPlan at the end of
the stages' gr-ais_amd/csrc/k_*.h), which the C ABI and the CPU models both run, pinned to literals: every derived size for
two argument sets per stage (one as the receiver creates the stage, below every cap; one with every capped count at its
cap), and for the NMEA parser the (grid, ngroups, nwaves) of each of a call's twelve launches in order.  The literals
were worked out by hand from the formulas aisx_<stage>_batch_create and _process held before the plans existed; each
carries its formula.  The plans are reached through the emu_<stage>_plan entry points of the model libraries, which
build them at the device's constants.  -m "not gpu"."""
import ctypes as C

import numpy as np

import hdlc_cases as hc
import test_mlse_model as mlse
import test_msg_model as msg
import test_nmea_batch_model as nmea
import test_nmea_parse_model as nmp
import test_track_model as trk


def plan(fn, *args, n):
    out = np.full(n, -1, dtype=np.int64)
    assert fn(*args, out.ctypes.data) == 1
    return out.tolist()


def desig(*names):
    return (C.c_char_p * len(names))(*[s.encode() for s in names])


def test_hdlc_plan():
    f = hc.emu().emu_hdlc_plan
    # the receiver's deframer (RX_LMIN = 11, RX_LMAX = 64), 1000 bits a call: span = 8 (lmax + 1) + max_bits = 1520
    assert plan(f, 11, 64, 4, 1000, 4096, n=4) == [
        9,       # carry_words = (8 (lmax + 1) + 63) / 64 = 583 / 64
        19,      # rec_cap = span / (8 lmin + 1) + 2 = 1520 / 89 + 2
        198,     # byte_cap = span / 8 + 8 = 190 + 8
        258048,  # out_bytes_cap = max_pdus (lmax - 1) = 4096 x 63
    ]
    # every argument at its bound: span = 8 x 1025 + 2^28 = 268443656
    assert plan(f, 2, 1024, 1, 1 << 28, 1, n=4) == [
        129,       # 8263 / 64
        15790805,  # 268443656 / 17 + 2
        33555465,  # 268443656 / 8 + 8
        1023,      # 1 x 1023
    ]
    assert f(1, 64, 4, 1000, 4096, None) == 0 and f(11, 1025, 4, 1000, 4096, None) == 0


def test_mlse_plan():
    f = mlse.emu().emu_mlse_plan
    # groups = max(1, (blocks + MLSE_T - 1) / MLSE_T) with blocks = (max_syms + MLSE_B - 1) / MLSE_B, MLSE_B = MLSE_T = 64
    assert plan(f, 8, 8500, n=1) == [3]               # blocks = 133, (133 + 63) / 64
    assert plan(f, 1, 1, n=1) == [1]                  # blocks = 1
    assert plan(f, 1 << 20, 1 << 27, n=1) == [32768]  # both bounds: blocks = 2^21, 2^21 / 64
    assert f((1 << 20) + 1, 100, None) == 0 and f(1, (1 << 27) + 1, None) == 0


def test_nmea_plan():
    f = nmea.emu().emu_nmea_plan
    ab = desig("A", "B")
    # the receiver's armourer (RX_LMAX = 64, designators of one byte): a payload of 63 octets is P = (8 x 63 + 5) / 6 = 84
    # characters in F = 2 fragments, nm_text_len = F (18 + digits(F) + dlen) + P - 1 = 40 + 83 = 123
    assert plan(f, ab, 2, 4096, 64, 4096 * 124, n=2) == [
        507904,  # text_cap = min(text_cap, worst) with worst = max_pdus (123 + 1)
        1024,    # write_groups = min((max_pdus + NM_W_T / 64 - 1) / (NM_W_T / 64), NM_W_MAX_GROUPS) = 4096 / 4
    ]
    assert plan(f, ab, 2, 4096, 64, 0, n=2) == [507904, 1024]  # text_cap = 0: the worst case
    # more records than NM_W_MAX_GROUPS x 4 waves, a text capacity below the worst case
    assert plan(f, ab, 2, 20000, 64, 1000, n=2) == [
        1000,  # text_cap as given
        4096,  # 5000 capped at NM_W_MAX_GROUPS
    ]
    assert f(desig("A", "seventeen bytes !!"), 2, 10, 64, 0, None) == 0 and f(ab, 2, 10, 1025, 0, None) == 0


NMP_KERNELS = ("count", "scan", "index", "parse", "gcount", "gscan1", "gcompact", "gmsg", "gscan2", "gplace", "write", "carry")


def test_nmea_parse_plan():
    f = nmp.emu().emu_nmp_plan
    ab = desig("A", "B")
    n = 6 + 3 * len(NMP_KERNELS)
    # NP_T = 256 threads, NP_CHUNK = 16 bytes a lane, NP_GMAX = 8, groups(items, per) = clamp((items + per - 1) / per, 1, NP_MAX_GROUPS = 2048)
    got = plan(f, ab, 2, 64, 128, 0, 1 << 20, 4096, 2048, n=n)
    assert got[:6] == [
        256,   # ntiles = (max_bytes + NP_T NP_CHUNK - 1) / (NP_T NP_CHUNK) = 2^20 / 4096
        17,    # nlt = (max_lines + NP_GMAX + NP_T - 1) / NP_T = 4359 / 256
        256,   # tile_groups = groups(ntiles, 1)
        1024,  # line_groups = groups(max_lines, NP_T / 64) = 4096 / 4
        17,    # ltile_groups = groups(nlt, 1)
        512,   # pdu_groups = groups(max_pdus, NP_T / 64) = 2048 / 4
    ]
    # a call as aisx_nmea_parse_batch_process queues it: ngroups = tile_groups and nwaves = line_groups x 4 up to the
    # parse, ngroups = ltile_groups from the group kernels on, nwaves = pdu_groups x 4 for the write and the carry
    want = [(256, 256, 4096), (1, 256, 4096), (256, 256, 4096), (1024, 256, 4096),
            (17, 17, 4096), (1, 17, 4096), (17, 17, 4096), (17, 17, 4096), (1, 17, 4096), (17, 17, 4096),
            (512, 17, 2048), (1, 17, 2048)]
    for k, name in enumerate(NMP_KERNELS):
        assert tuple(got[6 + 3 * k: 9 + 3 * k]) == want[k], name
    # every count at NP_MAX_GROUPS: 2^30 bytes are 262144 tiles, 2^26 lines 2^24 groups of four waves and 262145 tiles
    # of lines ((2^26 + 8 + 255) / 256), 2^20 records 262144 groups
    got = plan(f, ab, 2, 64, 4096, 1, 1 << 30, 1 << 26, 1 << 20, n=n)
    assert got[:6] == [262144, 262145, 2048, 2048, 2048, 2048]
    for k, name in enumerate(NMP_KERNELS):
        assert tuple(got[6 + 3 * k: 9 + 3 * k]) == ((1 if "scan" in name or name == "carry" else 2048), 2048, 8192), name
    assert f(ab, 2, 64, 63, 0, 1 << 20, 4096, 2048, None) == 0 and f(ab, 2, 64, 128, 2, 1 << 20, 4096, 2048, None) == 0


def test_msg_plan():
    f = msg.emu().emu_msg_plan
    # groups = min((max_pdus + MSG_T - 1) / MSG_T, MSG_MAX_GROUPS) with MSG_T = 256, MSG_MAX_GROUPS = 4096
    assert plan(f, 4, 4096, 64, n=1) == [16]        # the receiver's decoder (RX_LMAX = 64): 4096 / 256
    assert plan(f, 4, 1 << 21, 64, n=1) == [4096]   # 8192 capped
    assert f(4, 0, 64, None) == 0 and f(4, 10, 1, None) == 0


def test_track_plan():
    f = trk.emu().emu_trk_plan
    # trk_hash_bits(n): the least b >= 6 with 2^b >= 2 n; TRK_T = 256
    assert plan(f, 100000, 4096, n=7) == [
        18,   # hbits = trk_hash_bits(capacity): 2^18 = 262144 >= 200000 > 2^17
        13,   # bbits = trk_hash_bits(max_rows): 2^13 = 8192
        16,   # row_groups = (max_rows + TRK_T - 1) / TRK_T
        391,  # cap_groups = (capacity + TRK_T - 1) / TRK_T = 100255 / 256
        16,   # clear_groups = min(row_groups, 1024)
        782,  # bsum: 2 max(row_groups, cap_groups)
        391,  # nbmax = max(row_groups, cap_groups)
    ]
    # both at TRK_MAX = 2^24: the clear kernel's grid is the one capped count
    assert plan(f, 1 << 24, 1 << 24, n=7) == [25, 25, 65536, 65536, 1024, 131072, 65536]
    assert f(0, 10, None) == 0 and f(10, (1 << 24) + 1, None) == 0
