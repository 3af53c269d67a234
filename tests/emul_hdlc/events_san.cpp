// events_san.cpp -- a stand-alone program for the sanitizers (make san): the host form of the error-event repair
// (gr-ais_amd/csrc/aisx_framing.cpp) and the kernel bodies on the lane model (emul_hdlc.cpp) on the same ragged
// multi-channel script -- frames of the rules' lengths with one planted event of every kind (at the frame's first bit,
// across octets, in the FCS, at its last bit) or two, in noise, three calls per mask, the mask switched between them, the
// rows off 16-byte alignment -- compared record for record, bytes and marks.  Prints "events_san ok".
#include <stdio.h>

#include <random>

#include "emul_hdlc.cpp"

namespace {

std::mt19937 rng(11);

void put_flag(std::vector<unsigned char>& s)
{
    const unsigned char f[8] = { 0, 1, 1, 1, 1, 1, 1, 0 };
    s.insert(s.end(), f, f + 8);
}

// flag, the payload and its FCS with the bits of `flips` inverted, stuffed, flag
void put_frame(std::vector<unsigned char>& s, const std::vector<unsigned char>& payload, const std::vector<int>& flips)
{
    std::vector<unsigned char> bits;
    unsigned reg = 0xFFFFu;
    for (unsigned char o : payload)
        for (int k = 0; k < 8; k++) {
            const unsigned b = (o >> k) & 1u;
            bits.push_back((unsigned char)b);
            reg = ((reg ^ b) & 1u) ? (reg >> 1) ^ 0x8408u : reg >> 1;
        }
    const unsigned fcs = ~reg & 0xFFFFu;
    for (int k = 0; k < 16; k++)
        bits.push_back((unsigned char)((fcs >> k) & 1u));
    for (int i : flips)
        bits[(size_t)i] ^= 1;
    put_flag(s);
    int run = 0;
    for (unsigned char b : bits) {
        s.push_back(b);
        run = b ? run + 1 : 0;
        if (run == 5) {
            s.push_back(0);
            run = 0;
        }
    }
    put_flag(s);
}

std::vector<unsigned char> stream(int nbits)
{
    const int lens[] = { 21, 53, 39, 20, 12, 17 }, types[] = { 1, 5, 19, 24, 27, 1 };
    std::vector<unsigned char> s;
    while ((int)s.size() < nbits) {
        for (int k = (int)(rng() % 300); k > 0; k--)
            s.push_back((unsigned char)(rng() & 1u) * (unsigned char)(1 + rng() % 255)); // (any nonzero byte is a 1)
        const int w = (int)(rng() % 6), n = 8 * (lens[w] + 2);
        std::vector<unsigned char> p((size_t)lens[w]);
        for (auto& o : p)
            o = (unsigned char)rng();
        p[0] = (unsigned char)((types[w] << 2) | (p[0] & 3));
        std::vector<int> flips;
        const int kind = (int)(rng() % 10), span = (int)(rng() % 3);
        const int at = kind == 0 ? 0 : kind == 1 ? n - 1 - span : kind == 2 ? 8 * lens[w] - 1 : (int)(rng() % (unsigned)(n - span));
        if (kind != 9) {
            flips.push_back(at);
            if (span)
                flips.push_back(at + span);
        }
        if (kind == 8)
            flips.push_back((int)(rng() % (unsigned)n));
        put_frame(s, p, flips);
    }
    s.resize((size_t)nbits);
    return s;
}

} // namespace

int main()
{
    const int nchan = 5, max_bits = 9000, stride = max_bits + 7, max_pdus = 512, lmin = 11, lmax = 64;
    const aisx_hdlc_rule rules[5] = { { 21, 0, 0x104021EULL }, { 53, 0, 1ULL << 5 }, { 39, 0, 1ULL << 19 }, { 20, 0, 1ULL << 24 },
                                      { 12, 0, ~0ULL } };
    const int masks[] = { 7, 6, 1, 2, 5, 4, 3, 7 };
    aisx_hdlc* host[nchan];
    for (int c = 0; c < nchan; c++)
        if (aisx_hdlc_create(&host[c], lmin, lmax) != AISX_OK)
            return 2;
    void* lane = emu_hdlc_create(lmin, lmax, nchan, max_bits, max_pdus);
    std::vector<unsigned char> rows((size_t)nchan * stride + 16), hbytes((size_t)max_pdus * lmax), lbytes((size_t)max_pdus * lmax + 1);
    std::vector<HdlcRec> recs(max_pdus);
    std::vector<int> n(nchan), offs(max_pdus + 1), lfix(max_pdus), hfix(max_pdus);
    long total = 0, fixed = 0;
    for (int call = 0; call < 8; call++) {
        const int nrules = call == 6 ? 0 : 5;
        emu_hdlc_set_repair(lane, (const HdlcRule*)rules, nrules, masks[call]);
        unsigned char* base = rows.data() + (call % 3) * 5; // rows off 16-byte alignment
        for (int c = 0; c < nchan; c++) {
            if (aisx_hdlc_set_repair_events(host[c], rules, nrules, masks[call]) != AISX_OK)
                return 2;
            n[c] = c == 3 ? (call % 2) * 4097 : 5000 + (int)(rng() % 4000);
            const std::vector<unsigned char> s = stream(n[c]);
            if (!s.empty())
                memcpy(base + (size_t)c * stride, s.data(), s.size());
        }
        emu_hdlc_process(lane, base, stride, n.data());
        int count[3];
        emu_hdlc_read(lane, recs.data(), lbytes.data(), lfix.data(), count);
        int k = 0;
        for (int c = 0; c < nchan; c++) {
            int found = -1;
            if (aisx_hdlc_work_repair(host[c], base + (size_t)c * stride, n[c], hbytes.data(), (int)hbytes.size(), offs.data(),
                                      hfix.data(), max_pdus, &found) != AISX_OK)
                return 2;
            for (int j = 0; j < found; j++, k++) {
                const int len = offs[j + 1] - offs[j];
                if (k >= count[1] || recs[k].chan != c || recs[k].len != len || lfix[k] != hfix[j] ||
                    memcmp(&lbytes[(size_t)recs[k].offset], &hbytes[(size_t)offs[j]], (size_t)len) != 0) {
                    printf("events_san: call %d channel %d record %d differs (mark host %d)\n", call, c, j, hfix[j]);
                    return 1;
                }
                fixed += hfix[j] >= 0;
            }
        }
        if (k != count[0] || count[2]) {
            printf("events_san: call %d: host %d records, lanes %d (flag %d)\n", call, k, count[0], count[2]);
            return 1;
        }
        total += k;
    }
    for (int c = 0; c < nchan; c++)
        aisx_hdlc_destroy(host[c]);
    emu_hdlc_destroy(lane);
    if (total < 100 || fixed < 40) {
        printf("events_san: only %ld records, %ld repaired\n", total, fixed);
        return 1;
    }
    printf("events_san ok: %ld records, %ld repaired\n", total, fixed);
    return 0;
}
