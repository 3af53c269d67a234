// emul_msk_trips_end.cpp -- tests/emul_msk_trips's lane model with the plain pair loop staging a pair's symbol at the end
// of its own pair (the scheme of the device's compiler-scheduled builds).  TEST INFRASTRUCTURE (tests/test_emul_msk_trips.py).
#define MSK_EMU_END_STAGE 1
#include "../emul_msk_trips/emul_msk_trips.cpp"
