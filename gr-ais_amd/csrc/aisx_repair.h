// aisx_repair.h -- what the host deframer (aisx_framing.cpp, the specification of the single-bit repair) shares with
// the C ABI of the batched one (aisx_hdlc.hip): the check of a rule list and the table of single-error syndromes.
#pragma once
#include <stdint.h>

#include "../../include/aisx.h"

namespace aisx {

// AISX_OK, or AISX_ERR_INVALID for more than AISX_HDLC_MAX_RULES rules, a payload length outside
// [length_min - 2, length_max - 2] or given twice, or a reserved field that is not 0
int hdlc_rules_check(const aisx_hdlc_rule* rules, int nrules, int length_min, int length_max);
// uint16_t [65536]: for (computed FCS) xor (sent FCS), the distance + 1 of the one wrong bit from the frame's last
// bit that gives it, 0 where no single error does
const uint16_t* hdlc_syndrome_table();

} // namespace aisx
