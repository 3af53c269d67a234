// aisx_msg_enc.cpp -- aisx_msg_encode (include/aisx.h): one row of the column table back into the payload octets of
// its layout, plain C++.  It is the specification of the batched kernel (k_msg_enc.h), which runs the same rule
// (aisx_msgtab.h: msg_encode_row) on the same table: the two differ only in how a row reaches the rule and in where
// the staged payload's big-endian words are stored.
#include <string.h>

#include "../../include/aisx.h"
#include "aisx_msgtab.h"

using namespace aisx;

static_assert(MSG_ENC_NO_MMSI == AISX_MSG_ENC_NO_MMSI && MSG_ENC_NO_LAYOUT == AISX_MSG_ENC_NO_LAYOUT &&
                  MSG_ENC_RANGE == AISX_MSG_ENC_RANGE && MSG_ENC_BAD_CHAR == AISX_MSG_ENC_BAD_CHAR &&
                  MSG_ENC_BAD_ROW == AISX_MSG_ENC_BAD_ROW && MSG_ENC_OCTETS == AISX_MSG_ENC_PITCH,
              "status bits");
static_assert(sizeof(MsgEncTab) == sizeof(uint32_t) * MSG_ENC_TAB_WORDS, "table layout");

namespace aisx {
extern const MsgEncTab MSG_ENC_TAB; // (aisx_msg_enc.hip uploads it for the kernel)
const MsgEncTab MSG_ENC_TAB = msg_make_enc_tab();
} // namespace aisx

extern "C" int aisx_msg_encode(const int32_t* cols, const char* strs, int as_type, int as_part, uint8_t* pdu, int cap, int* len,
                               int* status)
{
    if (!cols || !pdu || !len || !status || cap < 0)
        return AISX_ERR_INVALID;
    uint32_t str[MSG_STR_WORDS], w[MSG_ROW];
    if (strs)
        for (int j = 0; j < MSG_STR_WORDS; j++) {
            str[j] = 0;
            for (int b = 0; b < 4; b++)
                str[j] |= (uint32_t)(uint8_t)strs[4 * j + b] << (8 * b);
        }
    int n = 0;
    const int st = msg_encode_row(cols, strs ? str : nullptr, as_type, as_part, (const uint32_t*)&MSG_ENC_TAB, w, &n);
    if (n > cap)
        return AISX_ERR_OVERFLOW;
    for (int k = 0; k < n; k++)
        pdu[k] = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
    *len = n;
    *status = st;
    return AISX_OK;
}
