// aisx_repair.h -- what the host deframer (aisx_framing.cpp, the specification of the repair by CRC syndrome) shares
// with the C ABI of the batched one (aisx_hdlc.hip): the check of a rule list and of an event mask, the table of
// single-error syndromes and the table of error-event syndromes for a mask.
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
// an event mask names at least one of AISX_HDLC_EV_SINGLE / _PAIR / _SKIP and nothing else
inline bool hdlc_events_ok(int events) { return events > 0 && (events & ~AISX_HDLC_EV_ALL) == 0; }
// out [65536]: for (computed FCS) xor (sent FCS), the enabled event (id 0 = single `1`, 1 = pair `11`, 2 = skip `101`;
// its span is its id) whose LAST flipped bit is nearest the frame's last bit, as id << 14 | distance + 1 of that bit
// for distances below AISX_HDLC_EV_REACH, 0 where no enabled event gives the syndrome.  The syndrome of an event at
// distance d is s(d) ^ s(d + span) with s the single-error syndrome (0x8000 for d = 0, one step of the shift
// register per bit further from the end).
void hdlc_event_table(int events, uint16_t* out);
// the same table, built once per mask and kept
const uint16_t* hdlc_event_table(int events);

} // namespace aisx
