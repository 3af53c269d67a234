// parse_san.cpp -- a stand-alone driver of the host NMEA parser (gr-ais_amd/csrc/aisx_nmea_parse.cpp) for sanitizer
// builds (TEST INFRASTRUCTURE: tests/test_nmea_parse_asan.py compiles both with -fsanitize=address,undefined).  Reads
// a file of cases -- u32 calls, then per call u32 bytes and the bytes -- and feeds every call from a heap block of
// exactly its size, into result buffers of exactly the capacity it names, so that any access past either is seen.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/aisx.h"

static bool rd32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    const char* des[4] = { "A", "B", "", "CHANNEL-16-BYTES" };
    long ncase = 0, ncall = 0, found = 0, kept = 0, lines = 0, octets = 0;
    uint32_t calls;
    while (rd32(f, &calls)) {
        aisx_nmea_parse* h = nullptr;
        if (aisx_nmea_parse_create(&h, des, 4, 64, 128, (int)(ncase & 1)) != AISX_OK)
            return 3;
        for (uint32_t c = 0; c < calls; c++) {
            uint32_t n;
            if (!rd32(f, &n))
                return 4;
            char* text = (char*)malloc(n ? n : 1);
            if (n && fread(text, 1, n, f) != n)
                return 4;
            // capacities: ample, tight on records, tight on bytes, none -- in turn
            const int mode = (int)((ncase + c) % 4);
            long nl = 1;
            for (uint32_t i = 0; i < n; i++)
                nl += text[i] == '\n';
            const int pdu_cap = mode == 1 ? 2 : mode == 3 ? 0 : (int)nl;
            const long bytes_cap = mode == 2 ? 30 : mode == 3 ? 0 : nl * 63;
            std::vector<aisx_pdu> pdus((size_t)pdu_cap);
            std::vector<uint8_t> bytes((size_t)bytes_cap);
            std::vector<int64_t> times((size_t)pdu_cap);
            int cnt[AISX_NMEAP_NCNT];
            const int rc = aisx_nmea_parse_work(h, n ? text : nullptr, (long)n, pdu_cap ? pdus.data() : nullptr, pdu_cap,
                                                bytes_cap ? bytes.data() : nullptr, bytes_cap, mode == 0 ? times.data() : nullptr, cnt);
            if (rc != AISX_OK && rc != AISX_ERR_OVERFLOW)
                return 5;
            if ((rc == AISX_ERR_OVERFLOW) != (cnt[AISX_NMEAP_KEPT] < cnt[AISX_NMEAP_FOUND]))
                return 6;
            for (int k = 0; k < cnt[AISX_NMEAP_KEPT]; k++) { // (every kept record lies inside the buffers)
                if (pdus[k].offset < 0 || pdus[k].len < 1 || pdus[k].offset + pdus[k].len > bytes_cap)
                    return 7;
                octets += bytes[(size_t)(pdus[k].offset + pdus[k].len - 1)];
            }
            found += cnt[AISX_NMEAP_FOUND];
            kept += cnt[AISX_NMEAP_KEPT];
            lines += cnt[AISX_NMEAP_LINES];
            free(text);
            ncall++;
        }
        if (ncase % 3 == 0)
            aisx_nmea_parse_reset(h);
        aisx_nmea_parse_destroy(h);
        ncase++;
    }
    fclose(f);
    printf("%ld cases, %ld calls, %ld lines, %ld messages, %ld kept (last octets sum to %ld)\n", ncase, ncall, lines, found, kept, octets);
    return 0;
}
