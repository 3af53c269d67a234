// emul_msk_trips.cpp -- the CPU lane model (tests/emul/emul.cpp, included as it is) built with the timing recovery's
// counters of plain lock-step runs per length (k_msk.h: msk_run_stats) and with the pair as C++ statements taking trips
// as long as the device's hand-scheduled build takes them (MSK_TRIP; tests/emul's own build -- tests/test_emul_msk_pair_runs.py
// -- takes MSK_TRIP_CXX's).  With MSK_EMU_END_STAGE (tests/emul_msk_trips_end) the plain pair loop stages a pair's symbol at
// the end of its own pair, as the device's compiler-scheduled builds do, instead of while the next pair loads.
// TEST INFRASTRUCTURE (tests/test_emul_msk_trips.py).
#define MSK_EMU_RUN_STATS 1
#define MSK_TRIP_CXX 8
struct EmuCtx;
#include "../../gr-ais_amd/csrc/k_msk.h"
static_assert(MSK_TRIP_CXX == MSK_TRIP, "the trip length of the hand-scheduled build");
#ifdef MSK_EMU_END_STAGE
namespace aisx {
template <>
struct msk_stage_rot<EmuCtx> { static constexpr bool value = false; };
}
#endif
#include "../emul/emul.cpp"

namespace aisx { long msk_run_stats[MSK_PAIRS_MAX + 1]; }

extern "C" long* emu_msk_run_stats() { return aisx::msk_run_stats; }
extern "C" void emu_msk_run_stats_reset()
{
    for (int i = 0; i <= MSK_PAIRS_MAX; i++)
        aisx::msk_run_stats[i] = 0;
}
extern "C" int emu_msk_end_stage()
{
#ifdef MSK_EMU_END_STAGE
    return 1;
#else
    return 0;
#endif
}
#ifdef MSK_EMU_END_STAGE
static_assert(!aisx::msk_stage_rot<EmuCtx>::value, "the end-of-pair staging scheme");
#else
static_assert(aisx::msk_stage_rot<EmuCtx>::value, "the rotated staging scheme");
#endif
