// enc_san.cpp -- a stand-alone program for the sanitizers (make san): the host form of the field encoder
// (gr-ais_amd/csrc/aisx_msg_enc.cpp) and the kernel body on the lane model (emul_msg_enc.cpp) on the same table -- rows
// decoded from random payloads of every type, some of them spoilt (NA, out of range, bad characters) -- without and
// with an index list and a channel column, compared bit for bit.  Prints "enc_san ok".
#include <stdio.h>

#include <random>

#include "emul_msg_enc.cpp"
#include "../../include/aisx.h"

static int fail(const char* what, int call, int i)
{
    printf("enc_san: call %d, record %d: %s differs\n", call, i, what);
    return 1;
}

int main()
{
    const int rows = 700, stride = rows + 5, max_rows = 900, nchan = 3;
    const int types[] = { 1, 2, 3, 4, 5, 11, 18, 19, 21, 24, 27, 6, 0 };
    std::mt19937 rng(11);
    std::vector<int32_t> cols((size_t)MSG_NCOL * stride, MSG_NA), chan(rows), idx(max_rows);
    std::vector<char> strs((size_t)rows * MSG_STR);
    for (int r = 0; r < rows; r++) {
        unsigned char p[62];
        for (auto& b : p)
            b = (unsigned char)rng();
        p[0] = (unsigned char)(types[rng() % 13] << 2 | (p[0] & 3));
        int32_t c[MSG_NCOL];
        if (aisx_msg_decode(p, 62, c, &strs[(size_t)r * MSG_STR]) != AISX_OK)
            return 2;
        const unsigned spoil = rng() % 8;
        if (spoil == 0)
            c[rng() % MSG_NCOL] = MSG_NA;
        else if (spoil == 1)
            c[rng() % MSG_NCOL] = (int32_t)rng();
        else if (spoil == 2)
            strs[(size_t)r * MSG_STR + rng() % MSG_STR] = (char)rng();
        for (int k = 0; k < MSG_NCOL; k++)
            cols[(size_t)k * stride + r] = c[k];
        chan[r] = (int)(rng() % (nchan + 1)) - (rng() % 16 == 0); // (some outside [0, nchan))
    }
    for (int i = 0; i < max_rows; i++)
        idx[i] = (int)(rng() % (rows + 20)) - 10; // (repeats, any order, some outside the table)
    void* lane = emu_msg_enc_create(nchan, max_rows, rows);
    if (!lane)
        return 2;
    std::vector<HdlcRec> pdus(max_rows);
    std::vector<unsigned char> bytes((size_t)max_rows * MSG_ENC_OCTETS);
    std::vector<int32_t> status(max_rows);
    long total = 0;
    for (int call = 0; call < 4; call++) {
        const bool with_idx = call & 1, with_chan = call & 2;
        const int n = with_idx ? max_rows : rows, as_type = call == 3 ? 18 : 0;
        int count[MENC_NCNT];
        if (!emu_msg_enc_process(lane, cols.data(), stride, strs.data(), with_idx ? idx.data() : nullptr, &n,
                                 with_chan ? chan.data() : nullptr, as_type, -1))
            return 2;
        emu_msg_enc_read(lane, pdus.data(), bytes.data(), status.data(), count);
        int good = 0;
        for (int i = 0; i < n; i++) {
            const int r = with_idx ? idx[i] : i;
            bool ok = r >= 0 && r < rows;
            int ch = 0;
            if (ok && with_chan) {
                ch = chan[r];
                if (ch < 0 || ch >= nchan)
                    ok = false, ch = 0;
            }
            unsigned char want[MSG_ENC_OCTETS] = {};
            int len = 0, st = AISX_MSG_ENC_BAD_ROW;
            if (ok) {
                int32_t c[MSG_NCOL];
                for (int k = 0; k < MSG_NCOL; k++)
                    c[k] = cols[(size_t)k * stride + r];
                if (aisx_msg_encode(c, &strs[(size_t)r * MSG_STR], as_type, -1, want, MSG_ENC_OCTETS, &len, &st) != AISX_OK)
                    return 2;
            }
            good += st == 0;
            if (status[i] != st)
                return fail("status", call, i);
            if (pdus[i].end_bit != (unsigned long long)i || pdus[i].offset != (long long)MSG_ENC_OCTETS * i || pdus[i].chan != ch ||
                pdus[i].len != len)
                return fail("record", call, i);
            if (memcmp(&bytes[(size_t)MSG_ENC_OCTETS * i], want, MSG_ENC_OCTETS) != 0)
                return fail("payload", call, i);
            total += len;
        }
        if (count[0] != n || count[1] != n || count[2] != 0 || count[3] != good || count[4] != n - good)
            return fail("counts", call, -1);
    }
    emu_msg_enc_destroy(lane);
    printf("enc_san ok: %ld octets\n", total);
    return 0;
}
