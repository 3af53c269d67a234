// k_tx.h -- the transmitter's kernel bodies (include/aisx.h: aisx_tx_batch_*).
//
//   tx_frame_body   one wave per burst: payload octets -> the burst's NRZ levels, packed 64 to a word, and per word the
//                   count of 1 levels before it, so that S(i) = 2 popcount(levels[0 .. i]) - (i + 1) is two loads and a
//                   popcount wherever a sample lands.  The stuffed positions come from one ballot per 64 frame bits (a
//                   bit is followed by a stuffed 0 when its place in its run of 1s is a multiple of five), the places
//                   behind stuffing from a prefix popcount, the NRZI levels from the prefix parity of the toggles.
//   tx_render_body  one workgroup per (channel, tile of TX_TILE samples), walking the tiles with a grid stride so that the
//                   phase pulse table is staged in LDS once per workgroup: finds the channel's bursts that touch the tile
//                   by binary search in the list sorted by start, stages each one's words for the tile's symbols in LDS and
//                   evaluates the specification's formula per sample -- no sample depends on another.  Two neighbouring
//                   samples per lane go out as one 16-byte store.
//
// Where float is enough and where it is not: u = (d - frac) / sps reaches 10^4 symbols and the phase turns pi/2 per
// symbol, so u, m = floor(u) and v = u - m are formed in double (six operations per sample); everything behind v is
// float.  The carrier offset is a 64-bit fixed-point turn count: cfo * 2^64 is an integer for every float |cfo| >= 2^-40,
// its product with d wraps modulo one turn exactly, and the top 32 bits are the turn to 2^-32 however large d is.
// (pi/2) S is applied as a swap / negation of the sine and cosine, so the argument that reaches sincospif is the sum
// of at most one turn of pulse terms, the offset's turn fraction and the phase, reduced to [-1/2, 1/2] of a turn.
//
// The table holds q at TX_QSTEPS = 2048 points per symbol and is read with linear interpolation: the error is at most
// h^2 / 8 max|q''| with h = 1 / 2048 and |q''| <= max|g'| < 1.3 (bt >= 0.3; 3.5 at bt = 1), i.e. 4e-8 of a quarter turn
// = 6e-8 rad per term, a quarter of the half-ulp (2.4e-7) of a float argument of a few radians.
#pragma once
#include "aisx_common.h"

namespace aisx {

constexpr int TXF_T = 64;                   // k_tx_frame: one wave
constexpr int TXF_MAX_SYMS = 10752;         // >= tx_max_nsyms(256, 64, 64, 1023) = 10240
constexpr int TXR_T = 256;                  // k_tx_render
constexpr int TX_TILE = 2048;               // samples of a tile: TXR_T lanes x 2 samples x TX_IT rounds
constexpr int TX_IT = TX_TILE / (2 * TXR_T);
constexpr int TX_QSTEPS = 2048;             // table points per symbol
constexpr int TX_QTAB = 4 * TX_QSTEPS + 2;  // q at 0, h, ..., 4 and one more for the upper neighbour of the last
constexpr int TX_STAGE_WORDS = 20;          // a tile spans at most TX_TILE / 2 + 6 symbols: 18 words
constexpr int TXR_LDS_BYTES = TX_QTAB * 4 + TX_STAGE_WORDS * 12 + 8;

struct TxBurst { // one scheduled burst on the device, sorted by (chan, start, frac)
    long long start;
    unsigned long long cfo_fix; // cfo * 2^64, modulo 2^64
    long long offset;           // payload in the handle's byte buffer
    double frac;
    int first, end;             // samples d = t - start of the burst: [first, end)
    int nsyms;                  // as the host counted them (k_tx_frame writes its own count beside the levels)
    int len;
    float amp, turn;            // turn = phase / 2 pi, in [-1/2, 1/2]
    int chan, pad;
};
static_assert(sizeof(TxBurst) == 64, "burst record");

struct TxFrameParams {
    const TxBurst* bursts;
    const unsigned char* bytes;
    int nbursts;
    int training, ramp, tail;
    int words;                  // words per burst in levels / wsum
    unsigned long long* levels; // [nbursts][words]
    int* wsum;                  // [nbursts][words] 1 levels in the words before
    int* nsyms;                 // [nbursts]
};

struct TxRenderParams {
    const TxBurst* bursts;
    const int* chan_off;        // [nchan + 1] the channels' ranges in bursts
    const unsigned long long* levels;
    const int* wsum;
    const float* qtab;          // [TX_QTAB]
    int words;
    int nchan;
    int max_end;                // the largest `end` of the schedule
    int ramp;
    double inv_sps;
    long long t0, n;
    cf* out;
    long long stride;
    int accumulate;
    int tiles_x;                // tiles per row
    long long ntiles;
};

template <class Ctx>
AISX_DI void tx_frame_body(Ctx& cx, const TxFrameParams& p)
{
    unsigned char* tg = reinterpret_cast<unsigned char*>(cx.lds()); // [TXF_MAX_SYMS] 1 = the level toggles at this symbol
    const int b = cx.bx();
    if (b >= p.nbursts)
        return;
    const int lane = cx.tid();
    const TxBurst& B = p.bursts[b];
    const unsigned char* payload = p.bytes + B.offset;
    const int len = B.len;
    // the FCS: every lane walks the octets (uniform loads, a 16-entry step table in registers would not be shorter)
    unsigned reg = 0xFFFFu;
    for (int k = 0; k < len; k++) {
        reg ^= payload[k];
        for (int i = 0; i < 8; i++)
            reg = (reg >> 1) ^ ((reg & 1u) ? 0x8408u : 0u);
    }
    const unsigned fcs = ~reg & 0xFFFFu;
    const int pre = p.ramp + p.training;
    // ramp 1, 0, 1, ... and training 1, 1, 0, 0, ... as toggles against a level of 0 before the burst
    for (int n = lane; n < pre; n += TXF_T) {
        const int lv = n < p.ramp ? ((n & 1) ^ 1) : (((n - p.ramp) & 3) < 2);
        const int m = n - 1;
        const int lp = m < 0 ? 0 : m < p.ramp ? ((m & 1) ^ 1) : (((m - p.ramp) & 3) < 2);
        tg[n] = (unsigned char)(lv ^ lp);
    }
    if (lane < 8) // the opening flag 0x7E: 0 toggles, 1 keeps
        tg[pre + lane] = (unsigned char)(lane == 0 || lane == 7);
    const int nbits = 8 * (len + 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    int outbase = pre + 8, carry = 0; // carry: the run of 1s the last block ended in
    for (int b0 = 0; b0 < nbits; b0 += 64) {
        const int bi = b0 + lane;
        const bool valid = bi < nbits;
        const int oct = bi >> 3;
        const unsigned octet = !valid ? 0u : oct < len ? payload[oct] : oct == len ? (fcs & 0xFFu) : (fcs >> 8);
        const bool bit = valid && ((octet >> (bi & 7)) & 1u);
        const unsigned long long M = cx.ballot(bit);
        const unsigned long long zlow = ~M & below;
        // this bit's place in its run of 1s, counted from 1
        const int j = zlow ? lane - (63 - __builtin_clzll(zlow)) : lane + 1 + carry;
        const bool stuff = bit && (j % 5) == 0;
        const unsigned long long St = cx.ballot(stuff);
        const int pos = outbase + lane + aisx_popc64(St & below);
        if (valid && pos + 1 < TXF_MAX_SYMS) {
            tg[pos] = (unsigned char)!bit;
            if (stuff)
                tg[pos + 1] = 1; // the stuffed 0
        }
        const int nv = nbits - b0 < 64 ? nbits - b0 : 64;
        outbase += nv + aisx_popc64(St);
        carry = M == ~0ull ? carry + 64 : __builtin_clzll(~M);
    }
    if (lane < 8 && outbase + lane < TXF_MAX_SYMS)
        tg[outbase + lane] = (unsigned char)(lane == 0 || lane == 7);
    int nsyms = outbase + 8 + p.tail;
    nsyms = nsyms < TXF_MAX_SYMS ? nsyms : TXF_MAX_SYMS;
    nsyms = nsyms < 64 * p.words ? nsyms : 64 * p.words;
    for (int n = outbase + 8 + lane; n < nsyms; n += TXF_T)
        tg[n] = 0;
    cx.wave_lds_sync();
    // levels = prefix parity of the toggles
    const unsigned long long upto = below | (1ull << lane);
    unsigned level = 0;
    int ones = 0;
    unsigned long long* W = p.levels + (size_t)b * p.words;
    int* Ws = p.wsum + (size_t)b * p.words;
    for (int w = 0; w < p.words; w++) {
        const int n = 64 * w + lane;
        const bool t = n < nsyms && tg[n];
        const unsigned long long T = cx.ballot(t);
        const unsigned lv = level ^ ((unsigned)aisx_popc64(T & upto) & 1u);
        const unsigned long long word = cx.ballot(n < nsyms && lv);
        if (lane == 0) {
            W[w] = word;
            Ws[w] = ones;
        }
        ones += aisx_popc64(word);
        level ^= (unsigned)aisx_popc64(T) & 1u;
    }
    if (lane == 0)
        p.nsyms[b] = nsyms;
}

// the value of burst B at sample d = t - start (first <= d < end), from the words staged in LDS
AISX_DI cf tx_sample(const TxBurst& B, int d, double inv_sps, float inv_r, bool ramped, const float* q,
                     const unsigned long long* sw, const int* ss, int wlo)
{
    const double u = ((double)d - B.frac) * inv_sps;
    int m = (int)floor(u);
    m = m < 0 ? 0 : m > B.nsyms - 1 ? B.nsyms - 1 : m;
    float v = (float)(u - (double)m);
    v = v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v;
    // the four levels a_{m-3} .. a_m and S(m - 4) modulo 4
    const int k0 = m - 3 + 64; // (+ 64: the word before the burst's first is staged as zeros)
    const int wi = (k0 >> 6) - (wlo + 1);
    const unsigned long long w0 = sw[wi], w1 = sw[wi + 1];
    const int sh = k0 & 63;
    const unsigned nib = (unsigned)((sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0) & 15ull);
    int quad = 0;
    const int i4 = m - 4;
    if (i4 >= 0) {
        const int wj = (i4 >> 6) - wlo;
        const int ones = ss[wj] + aisx_popc64(sw[wj] & (~0ull >> (63 - (i4 & 63))));
        quad = 2 * ones - (i4 + 1);
    }
    const float xv = v * (float)TX_QSTEPS;
    int i0 = (int)xv;
    i0 = i0 > TX_QSTEPS ? TX_QSTEPS : i0;
    const float f = xv - (float)i0;
    float sum = 0.0f;
#pragma unroll
    for (int j = 3; j >= 0; j--) { // a_{m-j} q(v + j), the oldest level first
        const int k = m - j;
        const float qa = q[i0 + j * TX_QSTEPS], qb = q[i0 + j * TX_QSTEPS + 1];
        const float qv = qa + f * (qb - qa);
        const float a = k < 0 ? 0.0f : ((nib >> (3 - j)) & 1u) ? 1.0f : -1.0f;
        sum += a * qv;
    }
    const float ct = (float)(int)(unsigned)((B.cfo_fix * (unsigned long long)(long long)d) >> 32) * 2.3283064365386963e-10f;
    float r = 0.25f * sum + ct + B.turn;
    r -= rintf(r);
    float s, c;
    sincospif(2.0f * r, &s, &c);
    const int qd = quad & 3;
    const float c1 = (qd & 1) ? -s : c, s1 = (qd & 1) ? c : s;
    const float c2 = (qd & 2) ? -c1 : c1, s2 = (qd & 2) ? -s1 : s1;
    float env = 1.0f;
    if (ramped) {
        const float ea = (float)u * inv_r, eb = (float)((double)B.nsyms - u) * inv_r;
        env = ea < eb ? ea : eb;
        env = env > 1.0f ? 1.0f : env < 0.0f ? 0.0f : env;
    }
    const float a = B.amp * env;
    return mk(a * c2, a * s2);
}

template <class Ctx>
AISX_DI void tx_render_body(Ctx& cx, const TxRenderParams& p)
{
    float* q = reinterpret_cast<float*>(cx.lds());
    unsigned long long* sw = reinterpret_cast<unsigned long long*>(cx.lds() + ((TX_QTAB * 4 + 7) & ~7));
    int* ss = reinterpret_cast<int*>(sw + TX_STAGE_WORDS);
    const int tid = cx.tid();
    for (int k = tid; k < TX_QTAB; k += TXR_T)
        q[k] = p.qtab[k];
    cx.sync();
    const bool ramped = p.ramp > 0;
    const float inv_r = ramped ? 2.0f / (float)p.ramp : 1.0f;
    for (long long tile = cx.bx(); tile < p.ntiles; tile += gridDim.x) {
        const int c = (int)(tile / p.tiles_x);
        const int tx = (int)(tile - (long long)c * p.tiles_x);
        cf* row = p.out + (size_t)c * (size_t)p.stride;
        const int mis = (int)(((size_t)row >> 3) & 1u); // 1: the row begins in the upper half of a 16-byte line
        // the tile's items: i = g - mis for g in [g_lo, g_lo + TX_TILE), pairs (g even, g + 1) share a 16-byte line
        const long long g_lo = (long long)tx * TX_TILE;
        long long i_lo = g_lo - mis, i_hi = g_lo + TX_TILE - mis;
        i_lo = i_lo < 0 ? 0 : i_lo;
        i_hi = i_hi > p.n ? p.n : i_hi;
        const long long T0 = p.t0 + i_lo, T1 = p.t0 + i_hi; // absolute samples [T0, T1)
        cf acc[2 * TX_IT];
#pragma unroll
        for (int k = 0; k < 2 * TX_IT; k++)
            acc[k] = mk(0.0f, 0.0f);
        bool any = false;
        if (i_lo < i_hi) {
            // bursts of the channel with start in (T0 - max_end, T1): the only ones that can touch [T0, T1)
            const int lo = p.chan_off[c], hi = p.chan_off[c + 1];
            int a = lo, e = hi;
            while (a < e) { // first with start > T0 - max_end
                const int mid = (a + e) >> 1;
                if (p.bursts[mid].start > T0 - p.max_end)
                    e = mid;
                else
                    a = mid + 1;
            }
            const int first = a;
            e = hi;
            while (a < e) { // first with start >= T1
                const int mid = (a + e) >> 1;
                if (p.bursts[mid].start >= T1)
                    e = mid;
                else
                    a = mid + 1;
            }
            const int last = a;
            for (int bi = first; bi < last; bi++) {
                const TxBurst B = p.bursts[bi];
                long long da = T0 - B.start, db = T1 - B.start; // the tile in the burst's own samples: [da, db)
                da = da < B.first ? B.first : da;
                db = db > B.end ? B.end : db;
                if (da >= db)
                    continue;
                any = true;
                // the symbols these samples reach: m - 4 of the first to m of the last (the same expression as
                // tx_sample's, which is monotone in d)
                int ma = (int)floor(((double)da - B.frac) * p.inv_sps), mb = (int)floor(((double)(db - 1) - B.frac) * p.inv_sps);
                ma = ma < 0 ? 0 : ma > B.nsyms - 1 ? B.nsyms - 1 : ma;
                mb = mb < 0 ? 0 : mb > B.nsyms - 1 ? B.nsyms - 1 : mb;
                const int wlo = (ma - 4 + 64) / 64 - 1; // floor((ma - 4) / 64), -1 for the symbols before the burst
                const int whi = mb >> 6;
                const int nwords = (B.nsyms + 63) >> 6;
                cx.sync(); // (the words of the burst before this one are no longer read)
                if (tid < TX_STAGE_WORDS) {
                    const int w = wlo + tid;
                    const bool in = w >= 0 && w < nwords && w <= whi + 1;
                    sw[tid] = in ? p.levels[(size_t)bi * p.words + w] : 0ull;
                    ss[tid] = in ? p.wsum[(size_t)bi * p.words + w] : 0;
                }
                cx.sync();
#pragma unroll
                for (int it = 0; it < TX_IT; it++) {
                    const long long i0 = g_lo + it * (2 * TXR_T) + 2 * tid - mis;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const long long d = p.t0 + i0 + h - B.start;
                        if (d >= da && d < db) {
                            const cf x = tx_sample(B, (int)d, p.inv_sps, inv_r, ramped, q, sw, ss, wlo);
                            acc[2 * it + h] = acc[2 * it + h] + x;
                        }
                    }
                }
            }
        }
        if (p.accumulate && !any)
            continue;
#pragma unroll
        for (int it = 0; it < TX_IT; it++) {
            const long long i0 = g_lo + it * (2 * TXR_T) + 2 * tid - mis;
            const bool v0 = i0 >= 0 && i0 < p.n, v1 = i0 + 1 >= 0 && i0 + 1 < p.n;
            cf x0 = acc[2 * it], x1 = acc[2 * it + 1];
            if (v0 && v1) {
                if (p.accumulate) {
                    cf o0, o1;
                    ld16(row + i0, o0, o1);
                    x0 = o0 + x0;
                    x1 = o1 + x1;
                }
                st16(row + i0, x0, x1);
            } else if (v0) {
                st8(row + i0, p.accumulate ? ld8(row + i0) + x0 : x0);
            } else if (v1) {
                st8(row + i0 + 1, p.accumulate ? ld8(row + i0 + 1) + x1 : x1);
            }
        }
    }
}

} // namespace aisx
