// emul_plan.h -- what the models of the batched stages (../emul_*/) share: storage for a buffer of the stage's launch
// plan (the *Plan struct of its gr-ais_amd/csrc/k_*.h), filled the way the device form leaves it (TEST INFRASTRUCTURE).
#pragma once
#include <string.h>

#include <vector>

#include "../../gr-ais_amd/csrc/aisx_common.h"

// zeroed where the device form allocates it zeroed, else 0x5a in every byte (what is not written shows)
template <class T>
void emu_alloc(std::vector<T>& v, const aisx::PlanBuf& b)
{
    v.resize(b.n ? b.n : 1);
    memset((void*)v.data(), b.zeroed ? 0 : 0x5a, sizeof(T) * v.size());
}
