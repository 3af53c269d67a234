// Host check of the pair loops' address helpers (gr-ais_amd/csrc/aisx_common.h) against the formulas they replace:
//   mmse_row / mmse_row_off for every float mu in [0, 1] (both zeros included) against rintf(mu * 128) * pitch + base,
//   ring_read_off against (odd ? sb + adv * slot : sb) & mask for every build's slot row and ring mask.
// Prints "ok" and exits 0, or the first mismatch and exits 1.
#include <cfenv>
#include <cstdio>
#include <cstring>

#include "aisx_common.h"

using namespace aisx;

static float u2f(unsigned u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main()
{
    if (fegetround() != FE_TONEAREST)
        return 2;
    const unsigned pitch = 48, base = 0x1234u * 16u, rbase = mmse_row_base(base, pitch);
    unsigned long long n = 0;
    for (unsigned u = 0; u <= 0x3F800000u; u++) { // +0 .. 1.0
        const float mu = u2f(u);
        const unsigned want = (unsigned)(int)rintf(mu * 128.0f);
        if (mmse_row(mu) != want || mmse_row_off(mu, pitch, rbase) != want * pitch + base) {
            printf("row: mu %a (0x%08x): %u, off %u, want %u\n", mu, u, mmse_row(mu), mmse_row_off(mu, pitch, rbase), want);
            return 1;
        }
        n++;
    }
    if (mmse_row(-0.0f) != 0u || mmse_row_off(-0.0f, pitch, rbase) != base) {
        printf("row: -0\n");
        return 1;
    }
    n++;
    // every ring layout: LPW 4 .. 64 channels per slot row, MSK_RING = 256 slots (the mask of k_msk.h)
    for (unsigned lpw = 4; lpw <= 64; lpw *= 2) {
        const unsigned slot = lpw * 8, mask = 255u * slot;
        for (int sb = -(1 << 16); sb < (1 << 20); sb += (int)slot / 4)
            for (int adv = 0; adv < 24; adv++)
                for (int odd = 0; odd < 2; odd++) {
                    const unsigned want = (unsigned)(odd ? sb + adv * (int)slot : sb) & mask;
                    const unsigned got = ring_read_off(sb, adv, odd ? slot : 0u, mask);
                    if (got != want) {
                        printf("ring: lpw %u sb %d adv %d odd %d: %u want %u\n", lpw, sb, adv, odd, got, want);
                        return 1;
                    }
                    n++;
                }
    }
    printf("ok %llu\n", n);
    return 0;
}
