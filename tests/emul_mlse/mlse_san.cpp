// mlse_san.cpp -- a stand-alone program for the sanitizers (make san): the host form of the sequence detector
// (gr-ais_amd/csrc/aisx_mlse.cpp) and the kernel body on the lane model (emul_mlse.cpp) on the same ragged
// multi-channel script -- four calls, a flush, a reset and one more call -- compared bit for bit.  Prints "mlse_san ok".
#include <stdio.h>

#include <random>

#include "emul_mlse.cpp"
#include "../../include/aisx.h"

namespace aisx {
char* err_buf() // (aisx_lib.hip's, which is not linked here)
{
    static thread_local char buf[512];
    return buf;
}
} // namespace aisx

int main()
{
    const int counts[] = { 0, 1, 15, 16, 17, 63, 64, 79, 80, 81, 143, 144, 145, 5000 };
    const int nchan = 5, max_syms = 5000, stride = max_syms + 3, bstride = max_syms + MLSE_EXTRA;
    std::mt19937 rng(7);
    std::normal_distribution<float> g(0.f, 1.f);
    aisx_mlse* host[nchan];
    float rot[16];
    for (int c = 0; c < nchan; c++)
        if (aisx_mlse_create(&host[c], 0.4) != AISX_OK)
            return 2;
    aisx_mlse_model(host[0], nullptr, nullptr, rot);
    void* lane = emu_mlse_create(rot, nchan, max_syms);
    std::vector<cf> syms((size_t)nchan * stride);
    std::vector<unsigned char> bits((size_t)nchan * bstride), hb((size_t)bstride);
    std::vector<int> n(nchan), nb(nchan);
    long total = 0;
    auto compare = [&](int c, int hn, const char* what) {
        if (hn != nb[c] || memcmp(hb.data(), &bits[(size_t)c * bstride], (size_t)hn) != 0) {
            printf("mlse_san: %s: channel %d differs (host %d bits, lanes %d)\n", what, c, hn, nb[c]);
            exit(1);
        }
        total += hn;
    };
    for (int round = 0; round < 2; round++) {
        for (int call = 0; call < (round ? 1 : 4); call++) {
            for (int c = 0; c < nchan; c++) {
                n[c] = counts[rng() % 14];
                for (int i = 0; i < n[c]; i++)
                    syms[(size_t)c * stride + i] = mk(g(rng), g(rng));
            }
            emu_mlse_process(lane, syms.data(), stride, n.data(), bits.data(), bstride, nb.data());
            for (int c = 0; c < nchan; c++) {
                int hn = -1;
                if (aisx_mlse_work(host[c], (const aisx_cf32*)&syms[(size_t)c * stride], n[c], hb.data(), bstride, &hn) != AISX_OK)
                    return 2;
                compare(c, hn, "process");
            }
        }
        emu_mlse_flush(lane, bits.data(), bstride, nb.data());
        for (int c = 0; c < nchan; c++) {
            int hn = -1;
            if (aisx_mlse_flush(host[c], hb.data(), bstride, &hn) != AISX_OK)
                return 2;
            compare(c, hn, "flush");
        }
        emu_mlse_reset(lane);
    }
    for (int c = 0; c < nchan; c++)
        aisx_mlse_destroy(host[c]);
    emu_mlse_destroy(lane);
    printf("mlse_san ok: %ld bits\n", total);
    return 0;
}
