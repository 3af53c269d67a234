// aisx_msg.cpp -- aisx_msg_decode (include/aisx.h): the ITU-R M.1371 fields of one PDU, plain C++.  It is the
// specification of the batched kernel (k_msg.h), which reads the same table (aisx_msgtab.h) through the same helpers:
// the two differ only in how a payload reaches its big-endian words and in where a row is stored.
#include <string.h>

#include "../../include/aisx.h"
#include "aisx_msgtab.h"

using namespace aisx;

static_assert(MSG_NCOL == AISX_MSG_NCOL && MSG_STR == AISX_MSG_STR && MSG_NA == AISX_MSG_NA, "table sizes");
static_assert(MC_FLAGS == AISX_MSG_COL_FLAGS && MC_ROT == AISX_MSG_COL_ROT && MC_LAT == AISX_MSG_COL_LAT &&
                  MC_RADIO == AISX_MSG_COL_RADIO && MC_TO_STARBOARD == AISX_MSG_COL_TO_STARBOARD && MC_MINUTE == AISX_MSG_COL_MINUTE &&
                  MC_PART == AISX_MSG_COL_PART && MC_CS_FLAGS == AISX_MSG_COL_CS_FLAGS,
              "column order");
static_assert(MSG_FL_COMPLETE == AISX_MSG_FL_COMPLETE && MSG_FL_NO_LAYOUT == AISX_MSG_FL_NO_LAYOUT &&
                  MSG_FL_BAD_RECORD == AISX_MSG_FL_BAD_RECORD,
              "flag bits");

namespace aisx {
extern const MsgTab MSG_TAB; // (aisx_msg.hip uploads it for the kernel)
const MsgTab MSG_TAB = msg_make_tab();
} // namespace aisx

extern "C" int aisx_msg_decode(const uint8_t* pdu, int len, int32_t* cols, char* strs)
{
    if (len < 0 || (len > 0 && !pdu) || !cols || !strs)
        return AISX_ERR_INVALID;
    uint32_t w[MSG_ROW] = {};
    const int take = len < MSG_OCTETS ? len : MSG_OCTETS;
    for (int k = 0; k < take; k++)
        w[k >> 2] |= (uint32_t)pdu[k] << (24 - 8 * (k & 3));
    const int nbits = 8 * take; // (no field and no minimum length lies beyond MSG_OCTETS)
    const int layout = msg_layout_of(w, nbits);
    const uint32_t* lay = MSG_TAB.f[layout];
    for (int c = 0; c < MSG_NCOL; c++)
        cols[c] = c == MC_FLAGS ? msg_flags(lay, layout, nbits) : msg_field(w, lay[c], nbits);
    for (int j = 0; j < MSG_STR_WORDS; j++) {
        const uint32_t v = msg_str_word(w, lay, nbits, j);
        for (int b = 0; b < 4; b++)
            strs[4 * j + b] = (char)(v >> (8 * b) & 255u);
    }
    return AISX_OK;
}
