// k_xlate.h -- batched freq_xlating_fir_filter_ccf (the general block): any
// decimation D, any real prototype h[0..L-1], any centre frequency per output row.  The filter is evaluated in the
// mix-first form, algebraically the block GNU Radio 3.8 builds (rotated taps, decimating FIR, rotator):
//   y[k] = sum_n h[n] z[kD - n],   z[m] = x[m] e^{-j w m},   w = 2 pi f_c / fs,   x[m] = 0 for m < 0
// so each tap costs one packed fma per output (re and im against the same real tap).
//
// Phase.  The phase of input m is a 64-bit fixed-point fraction of a turn, P(m) = inc*m + off (mod 2^64), a function
// of the absolute index only: inc = f_c/fs * 2^64, and off carries the constant of every retune (the rotator goes on
// from its phase: off += (inc_old - inc_new) * D * k_r).  The rotation of m is the product of the rotation of its
// block of XL_B inputs (computed in double from P at the block start) and an in-block entry of a per-row table (built
// in double on the host).  Both are pure functions of m, so is z[m].
//
// Work split.  One workgroup per (tile of G*R outputs, stream); lane l < G owns R consecutive outputs.  Relative to
// the tile's first needed input, output l*R + r reads input l*P + u with tap n = rD + L-1-u (P = R*D): at offset u the
// R taps are the same for every lane (a wave-uniform row of the host's tap table, zero where n leaves [0, L)), and one
// LDS read of z feeds R fmas.  For each channel of the stream the raw inputs of the window are mixed while they are
// staged into LDS.  Lane l's inputs start at window item l*P; the window is stored with one pad item per P items when P
// is even (odd stride: the 32 lanes of a half-wave hit 32 different bank pairs).  A window too large for LDS is cut
// into chunks of u; every output's sum runs over u = 0 .. (R-1)D + L - 1 in that order in one fma chain whatever the
// tile, chunk or call boundaries are, so any split of the input into calls gives the same bits.
#pragma once
#include <initializer_list>
#include <vector>

#include "aisx_common.h"

namespace aisx {

constexpr int XL_T = 256;                          // threads per workgroup
constexpr int XL_WCAP = 6144;                      // LDS window in items (48 KB): 3 workgroups per CU
constexpr int XL_LB = 8, XL_B = 1 << XL_LB;        // rotation blocks of XL_B inputs
constexpr int XL_NB = XL_WCAP / XL_B + 2;          // block rotations one window can touch
constexpr int XL_LDS_ITEMS = XL_WCAP + XL_B + XL_NB;
constexpr int XL_MAX_DECIM = 4096;
constexpr int XL_MAX_TAPS = 1 << 17;
constexpr int XL_MAX_CHAN = 1024;

struct XlateParams {
    const void* in;                     // [nstreams][in_stride] items of the loader's format: n new inputs per stream
    long long in_stride;
    const cf* hist_in;                  // [nstreams][Lh]: inputs m_abs - Lh .. m_abs - 1
    cf* hist_out;                       // [nstreams][Lh]: the same after this call
    const cf* tab;                      // [nrows][XL_B]: e^{-j 2 pi inc i / 2^64}
    const unsigned long long* par;      // [nrows][2]: inc, off
    cf* out;                            // [nrows][out_stride], row = stream * nch + chan, column = k - k_first
    long long out_stride;
    long long m_abs;                    // absolute index of this call's first input
    long long k_first;                  // absolute index of this call's first output
    int n, nout, Lh, nch, D, L;
    int P, S, G, U, Utot;               // the plan (XlatePlan)
    unsigned long long magic;           // j / P = (j * magic) >> 32 for the window's j
    float scale = 1.f, bias = 0.f;      // integer formats: value = ((float)raw - bias) * scale (fc32 ignores them)
};

// The input's item in memory (include/aisx.h, AISX_FMT_*).  An integer item becomes ((float)raw - bias) * scale on re
// and im alike: two float32 operations, each rounded once ((a - b) * c cannot contract into an fma), so numpy's
// (raw.astype(float32) - float32(bias)) * float32(scale) gives the same bits.  The history stays converted values.
enum { XL_FMT_CF32 = 0, XL_FMT_CS16 = 1, XL_FMT_CS8 = 2, XL_FMT_CU8 = 3, XL_NFMT = 4 };

struct XlLoadCF32 {
    typedef cf item;
    static AISX_HD cf load(const item* x, long long i, float, float) { return x[i]; }
};
template <class I>
struct XlLoadInt {
    struct item {
        I re, im;
    };
    static AISX_HD cf load(const item* x, long long i, float scale, float bias)
    {
        const item v = x[i];
        return mk(((float)v.re - bias) * scale, ((float)v.im - bias) * scale);
    }
};
typedef XlLoadInt<short> XlLoadCS16;
typedef XlLoadInt<signed char> XlLoadCS8;
typedef XlLoadInt<unsigned char> XlLoadCU8;

inline bool xlate_fmt_ok(int fmt, float scale, float bias)
{
    return fmt >= 0 && fmt < XL_NFMT && isfinite(scale) && isfinite(bias);
}
inline int xlate_item_bytes(int fmt) { return fmt == XL_FMT_CF32 ? 8 : fmt == XL_FMT_CS16 ? 4 : 2; }

// acc + h * z on re and im: one v_pk_fma_f32 on the device
AISX_HD cf xl_fma(float h, cf z, cf acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f hv, zv, av;
    hv.x = h;
    hv.y = h;
    zv.x = z.re;
    zv.y = z.im;
    av.x = acc.re;
    av.y = acc.im;
    const v2f r = __builtin_elementwise_fma(hv, zv, av);
    return mk(r.x, r.y);
#else
    return mk(fmaf(h, z.re, acc.re), fmaf(h, z.im, acc.im));
#endif
}

// e^{-j 2 pi (inc m + off) / 2^64}, the phase reduced exactly in 64 bits, then evaluated in double
AISX_HD cf xl_rot(unsigned long long inc, unsigned long long off, long long m)
{
    const unsigned long long ph = inc * (unsigned long long)m + off;
    const double a = (double)(long long)ph * (6.283185307179586476925286766559 / 18446744073709551616.0);
    double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, &sn, &cs);
#else
    sn = sin(a);
    cs = cos(a);
#endif
    return mk((float)cs, (float)-sn);
}

template <int R, class Ctx, class Ld = XlLoadCF32>
AISX_DI void xlate_body(Ctx& cx, const XlateParams& p, const float* __restrict__ taps)
{
    const int t = cx.tid(), nt = cx.nthreads();
    const int s = cx.by();
    cf* win = (cf*)cx.lds();
    cf* tab = win + XL_WCAP;
    cf* base = tab + XL_B;
    const int col0 = cx.bx() * p.G * R;         // this tile's first output column
    const bool tile_on = col0 < p.nout;
    const long long mb = (p.k_first + col0) * (long long)p.D - (p.L - 1);
    const long long m_end = p.m_abs + p.n;
    const typename Ld::item* xin = (const typename Ld::item*)p.in + (long long)s * p.in_stride;
    const cf* hin = p.hist_in + (long long)s * p.Lh;
    const bool lane_on = t < p.G;
    const int P = p.P, S = p.S;
    for (int c = 0; tile_on && c < p.nch; c++) {
        const int row = s * p.nch + c;
        const unsigned long long inc = p.par[2 * row], off = p.par[2 * row + 1];
        for (int i = t; i < XL_B; i += nt)
            tab[i] = p.tab[(long long)row * XL_B + i];
        cf acc[R];
#pragma unroll
        for (int r = 0; r < R; r++)
            acc[r] = mk(0.f, 0.f);
        for (int u0 = 0; u0 < p.Utot; u0 += p.U) {
            const int Uc = p.Utot - u0 < p.U ? p.Utot - u0 : p.U;
            const int W = (p.G - 1) * P + Uc;
            const long long m0 = mb + u0; // absolute index of window item 0
            const long long b0 = m0 >> XL_LB;
            const int nb = (int)(((m0 + W - 1) >> XL_LB) - b0) + 1;
            for (int i = t; i < nb; i += nt)
                base[i] = xl_rot(inc, off, (b0 + i) * XL_B);
            cx.sync(); // (also: every lane is done reading the previous chunk's window)
            for (int j = t; j < W; j += nt) {
                const long long m = m0 + j;
                cf z = mk(0.f, 0.f);
                if (m >= 0 && m < m_end && m >= p.m_abs - p.Lh) {
                    const cf x = m >= p.m_abs ? Ld::load(xin, m - p.m_abs, p.scale, p.bias) : hin[m - (p.m_abs - p.Lh)];
                    const cf rot = cmul_fma(base[(m >> XL_LB) - b0], tab[m & (XL_B - 1)]);
                    z = cmul_fma(x, rot);
                }
                const int q = (int)(((unsigned long long)(unsigned)j * p.magic) >> 32); // j / P (j < 2^16)
                win[q * S + (j - q * P)] = z;
            }
            cx.sync();
            if (lane_on) {
                const cf* wl = win + t * S;
                const float* tp = taps + (long long)u0 * R;
                for (int uu = 0, sg = 0; uu < Uc; sg++) {
                    const int len = Uc - uu < P ? Uc - uu : P;
                    const cf* zp = wl + sg * S;
                    const float* hp = tp + uu * R;
#pragma unroll 4
                    for (int v = 0; v < len; v++) {
                        const cf z = zp[v];
#pragma unroll
                        for (int r = 0; r < R; r++)
                            acc[r] = xl_fma(hp[v * R + r], z, acc[r]);
                    }
                    uu += len;
                }
            }
        }
        if (lane_on) {
            cf* o = p.out + (long long)row * p.out_stride + col0 + t * R;
#pragma unroll
            for (int r = 0; r < R; r++)
                if (col0 + t * R + r < p.nout)
                    o[r] = acc[r];
        }
    }
    // history for the next call: the last Lh inputs of (history ++ this call's), by the first tile of each stream
    if (cx.bx() == 0) {
        cf* ho = p.hist_out + (long long)s * p.Lh;
        for (int j = t; j < p.Lh; j += nt) {
            const long long m = m_end - p.Lh + j;
            cf v = mk(0.f, 0.f);
            if (m >= p.m_abs)
                v = Ld::load(xin, m - p.m_abs, p.scale, p.bias);
            else if (m >= p.m_abs - p.Lh)
                v = hin[m - (p.m_abs - p.Lh)];
            ho[j] = v;
        }
    }
}

// ---- host side: the plan, the tap table, the phase increments (shared by aisx_xlate.hip and the lane model) ----

struct XlatePlan {
    int R, P, S, G, U, Utot;
    unsigned long long magic;
};

inline long long xl_window_items(int G, int U, int P, int S)
{
    const long long j = (long long)(G - 1) * P + U - 1;
    return (j / P) * S + j % P + 1;
}

// R outputs per lane: the largest of 8, 4, 2, 1 whose edge waste ((R-1)D zero taps per output) stays within an eighth
// of L and whose window, for all nt lanes and 512 offsets u, fits the LDS; then the chunk of u as large as fits.
// With R = 1 and a stride too large for nt lanes, fewer lanes take part (large decimations).
inline XlatePlan xlate_plan(int D, int L, int nt, int wcap)
{
    XlatePlan pl;
    int R = 1;
    for (int r : { 8, 4, 2 }) {
        const int P = r * D, S = P + ((P & 1) ? 0 : 1), Utot = (r - 1) * D + L;
        if ((long long)(r - 1) * D * 8 <= L && xl_window_items(nt, Utot < 512 ? Utot : 512, P, S) <= wcap) {
            R = r;
            break;
        }
    }
    pl.R = R;
    pl.P = R * D;
    pl.S = pl.P + ((pl.P & 1) ? 0 : 1);
    pl.Utot = (R - 1) * D + L;
    const int umin = pl.Utot < 64 ? pl.Utot : 64;
    pl.G = nt;
    while (pl.G > 1 && xl_window_items(pl.G, umin, pl.P, pl.S) > wcap)
        pl.G--;
    int lo = 1, hi = pl.Utot; // largest U with the window within wcap
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (xl_window_items(pl.G, mid, pl.P, pl.S) <= wcap)
            lo = mid;
        else
            hi = mid - 1;
    }
    pl.U = lo;
    pl.magic = (1ull << 32) / (unsigned long long)pl.P + 1;
    return pl;
}

// [Utot][R]: row u holds h[rD + L-1-u] for r = 0..R-1, zero where that leaves [0, L)
inline void xlate_tap_table(const float* h, int L, int D, const XlatePlan& pl, float* out)
{
    for (int u = 0; u < pl.Utot; u++)
        for (int r = 0; r < pl.R; r++) {
            const long long n = (long long)r * D + L - 1 - u;
            out[(long long)u * pl.R + r] = (n >= 0 && n < L) ? h[n] : 0.f;
        }
}

// f / fs as a 64-bit fraction of a turn (|f| <= fs / 2), rounded to nearest
inline unsigned long long xlate_inc(double f, double fs)
{
    long double v = (long double)f / (long double)fs * 18446744073709551616.0L;
    if (v >= 9223372036854775808.0L)
        v -= 18446744073709551616.0L;
    return (unsigned long long)(long long)llroundl(v);
}

inline void xlate_row_table(unsigned long long inc, cf* out)
{
    for (int i = 0; i < XL_B; i++)
        out[i] = xl_rot(inc, 0, i);
}

inline bool xlate_freq_ok(double f, double fs) { return f == f && fabs(f) <= fs / 2; }

inline long long xl_floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The host half of a handle (the product's aisx_xlate and the lane model both hold one): geometry, the plan, the
// phase of every row and the stream position.  Everything a call's launch needs but the device buffers.
struct XlateHost {
    int ns = 0, nch = 0, D = 0, L = 0, Lh = 0, max_items = 0;
    double fs = 0;
    XlatePlan plan{};
    std::vector<double> freq;              // [nrows]
    std::vector<unsigned long long> par;   // [nrows][2]: inc, off
    std::vector<cf> tab;                   // [nrows][XL_B]
    std::vector<float> taps;               // [Utot][R]
    long long m_abs = 0, k_abs = 0;        // inputs taken, outputs produced since create / reset
    int nrows() const { return ns * nch; }

    // the argument checks of aisx_xlate_create: nullptr when they pass, else what is wrong
    static const char* check(int decim, const float* h, int ntaps, const double* freqs, int nch_, double fs_, int ns_,
                             int max_items_)
    {
        if (!h || !freqs || decim < 1 || decim > XL_MAX_DECIM || ntaps < 1 || ntaps > XL_MAX_TAPS || nch_ < 1 ||
            nch_ > XL_MAX_CHAN || !(fs_ > 0) || !isfinite(fs_) || ns_ < 1 || ns_ > 65535 || max_items_ < 1 ||
            max_items_ > (1 << 30))
            return "need taps, centre frequencies, 1 <= decim <= 4096, 1 <= ntaps <= 131072, 1 <= nchan_per_stream "
                   "<= 1024, samp_rate > 0, 1 <= nstreams <= 65535, 1 <= max_items <= 2^30";
        for (long long r = 0; r < (long long)ns_ * nch_; r++)
            if (!xlate_freq_ok(freqs[r], fs_))
                return "a centre frequency is outside [-fs/2, fs/2]";
        return nullptr;
    }
    void init(int decim, const float* h, int ntaps, const double* freqs, int nch_, double fs_, int ns_, int max_items_,
              int nt)
    {
        ns = ns_;
        nch = nch_;
        D = decim;
        L = ntaps;
        Lh = ntaps - 1;
        max_items = max_items_;
        fs = fs_;
        plan = xlate_plan(D, L, nt, XL_WCAP);
        freq.assign(freqs, freqs + nrows());
        par.assign(2 * (size_t)nrows(), 0);
        tab.resize((size_t)nrows() * XL_B);
        for (int r = 0; r < nrows(); r++) {
            par[2 * r] = xlate_inc(freq[r], fs);
            xlate_row_table(par[2 * r], tab.data() + (size_t)r * XL_B);
        }
        taps.resize((size_t)plan.Utot * plan.R);
        xlate_tap_table(h, L, D, plan, taps.data());
    }
    // outputs k with k D in [m_abs, m_abs + n): ceil((m_abs + n) / D) - ceil(m_abs / D)
    int count(long long n) const { return (int)(xl_floor_div(-m_abs, D) - xl_floor_div(-(m_abs + n), D)); }
    // from the next call on; the rotator goes on from its phase at the next output k_r:
    // off += (inc_old - inc_new) D k_r (mod 2^64)
    void retune(int r, double f)
    {
        const unsigned long long inc = xlate_inc(f, fs);
        par[2 * r + 1] += (par[2 * r] - inc) * (unsigned long long)D * (unsigned long long)k_abs;
        par[2 * r] = inc;
        freq[r] = f;
        xlate_row_table(inc, tab.data() + (size_t)r * XL_B);
    }
    void reset()
    {
        for (int r = 0; r < nrows(); r++)
            par[2 * r + 1] = 0;
        m_abs = k_abs = 0;
    }
    // a call's parameters but the buffers; advances the stream position
    XlateParams params(int n, long long in_stride, long long out_stride)
    {
        XlateParams p{};
        p.in_stride = in_stride;
        p.out_stride = out_stride;
        p.m_abs = m_abs;
        p.k_first = k_abs;
        p.n = n;
        p.nout = count(n);
        p.Lh = Lh;
        p.nch = nch;
        p.D = D;
        p.L = L;
        p.P = plan.P;
        p.S = plan.S;
        p.G = plan.G;
        p.U = plan.U;
        p.Utot = plan.Utot;
        p.magic = plan.magic;
        m_abs += n;
        k_abs += p.nout;
        return p;
    }
    int tiles(int nout) const { return nout > 0 ? (nout + plan.G * plan.R - 1) / (plan.G * plan.R) : 1; }
};

} // namespace aisx
