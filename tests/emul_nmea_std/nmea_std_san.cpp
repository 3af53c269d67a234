// nmea_std_san.cpp -- a stand-alone driver of the standard-form NMEA armouring for sanitizer builds (TEST
// INFRASTRUCTURE: tests/test_nmea_std_asan.py builds it by the Makefile beside it with -fsanitize=address,undefined):
// the lane model of the kernel bodies (emul_nmea_std.cpp, through the shared launch plan) and the host function
// (gr-ais_amd/csrc/aisx_framing.cpp) in one program.  Reads a file of cases --
//   u32 nchan, per channel { u8 n, designator bytes, u8 n, station bytes }, i32 length_max, i32 max_pdus, i64 text_cap,
//   u32 calls, per call { i64 time, i32 npdus, u8 reset first, u32 records, per record { i32 chan, i32 len, bytes } }
// -- and feeds every call from heap blocks of exactly the records' and the payloads' size; the handle's own buffers are
// exactly what the plan asks for.  Every text is compared with the host function's, the ids counted here.
#include "emul_nmea_std.cpp"

#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../include/aisx.h"

template <class T>
static bool rd(FILE* f, T* v) { return fread(v, sizeof(T), 1, f) == 1; }

static bool rd_str(FILE* f, std::string* s)
{
    uint8_t n;
    if (!rd(f, &n))
        return false;
    s->resize(n);
    return n == 0 || fread(&(*s)[0], 1, n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    long ncase = 0, ncall = 0, nrec = 0, nbytes = 0;
    uint32_t nchan;
    while (rd(f, &nchan)) {
        std::vector<std::string> des(nchan), sta(nchan);
        for (uint32_t c = 0; c < nchan; c++)
            if (!rd_str(f, &des[c]) || !rd_str(f, &sta[c]))
                return 3;
        std::vector<const char*> dp, sp;
        for (uint32_t c = 0; c < nchan; c++) {
            dp.push_back(des[c].c_str());
            sp.push_back(sta[c].c_str());
        }
        int32_t length_max, max_pdus;
        int64_t text_cap;
        uint32_t calls;
        if (!rd(f, &length_max) || !rd(f, &max_pdus) || !rd(f, &text_cap) || !rd(f, &calls))
            return 3;
        void* h = emu_nmea_std_create(dp.data(), sp.data(), (int)nchan, max_pdus, length_max, (long)text_cap);
        if (!h)
            return 4;
        const long cap = emu_nmea_std_text_cap(h);
        int id = 0;
        for (uint32_t k = 0; k < calls; k++) {
            int64_t time;
            int32_t npdus;
            uint8_t reset;
            uint32_t n;
            if (!rd(f, &time) || !rd(f, &npdus) || !rd(f, &reset) || !rd(f, &n))
                return 3;
            if (reset) {
                emu_nmea_std_reset(h);
                id = 0;
            }
            if (!emu_nmea_std_set_time(h, time))
                return 5;
            HdlcRec* recs = (HdlcRec*)malloc(sizeof(HdlcRec) * (n ? n : 1));
            std::vector<unsigned char> all;
            for (uint32_t i = 0; i < n; i++) {
                int32_t chan, len;
                if (!rd(f, &chan) || !rd(f, &len) || len < 0)
                    return 3;
                recs[i].end_bit = 11ull * i + k;
                recs[i].offset = (long long)all.size();
                recs[i].chan = chan;
                recs[i].len = len;
                all.resize(all.size() + (size_t)len);
                if (len && fread(all.data() + recs[i].offset, 1, (size_t)len, f) != (size_t)len)
                    return 3;
            }
            unsigned char* bytes = (unsigned char*)malloc(all.size() ? all.size() : 1);
            if (!all.empty())
                memcpy(bytes, all.data(), all.size());
            int* cnt_in = (int*)malloc(sizeof(int));
            *cnt_in = npdus;
            emu_nmea_std_process(h, recs, bytes, cnt_in, nullptr);
            std::vector<HdlcRec> out((size_t)max_pdus);
            std::vector<char> text((size_t)cap + 1);
            int cnt[3];
            emu_nmea_std_read(h, out.data(), text.data(), cnt);
            // what the host function and the rules of include/aisx.h say
            const bool bad_count = npdus < 0 || npdus > max_pdus;
            long long pos = 0;
            int kept = 0;
            bool bad = bad_count;
            for (int i = 0; !bad_count && i < npdus; i++) {
                const HdlcRec& r = recs[i];
                char want[2048];
                int wn = 0;
                const bool good = r.chan >= 0 && r.chan < (int)nchan && r.len <= length_max - 1;
                bad = bad || !good;
                if (good && r.len > 0) {
                    wn = aisx_pdu_to_nmea_std(dp[r.chan], bytes + r.offset, r.len, id, sp[r.chan], time, want, (int)sizeof want);
                    if (wn <= 0)
                        return 6;
                }
                if (pos + (wn ? wn + 1 : 0) > cap)
                    break;
                if (i >= cnt[1])
                    return 7;
                const HdlcRec& o = out[i];
                if (o.offset != pos || o.len != wn || o.chan != r.chan || o.end_bit != r.end_bit)
                    return 8;
                if (wn && (memcmp(text.data() + pos, want, (size_t)wn) != 0 || text[pos + wn] != '\n')) {
                    fprintf(stderr, "case %ld call %u record %d:\n%.*s\n%s\n", ncase, k, i, wn, text.data() + pos, want);
                    return 9;
                }
                pos += wn ? wn + 1 : 0;
                kept++;
                if (good && 6 * NM_FRAG < 8 * r.len)
                    id = (id + 1) % 10;
                nbytes += wn;
            }
            if (cnt[1] != kept || cnt[0] != (bad_count ? 0 : npdus))
                return 10;
            // (the flag speaks of the whole list, cut or not)
            for (int i = kept; !bad_count && i < npdus; i++)
                bad = bad || !(recs[i].chan >= 0 && recs[i].chan < (int)nchan && recs[i].len <= length_max - 1);
            if ((cnt[2] != 0) != bad || emu_nmea_std_next_id(h) != id)
                return 11;
            free(recs);
            free(bytes);
            free(cnt_in);
            nrec += kept;
            ncall++;
        }
        emu_nmea_std_destroy(h);
        ncase++;
    }
    fclose(f);
    printf("%ld cases, %ld calls, %ld records, %ld bytes of text identical to the host function's\n", ncase, ncall, nrec, nbytes);
    return 0;
}
