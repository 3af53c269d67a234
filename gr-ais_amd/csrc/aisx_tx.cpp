// aisx_tx.cpp -- the transmit side on the host, plain C++ (include/aisx.h: aisx_hdlc_frame, aisx_tx_render_host): the
// specification of what aisx_tx.hip does on the device.
//
//   aisx_hdlc_frame      the inverse of aisx_hdlc_work behind an NRZI decoder: payload octets to the NRZ levels of one
//                        burst (ramp, training sequence, flag, stuffed payload + FCS, flag, tail);
//   aisx_tx_render_host  the GMSK waveform of a schedule of bursts, every output sample from the closed form in
//                        double: an exact quadrant from the integer level sum, the last L = 4 levels through the
//                        phase pulse q, the carrier offset, one rounding to float.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "aisx_tx.h"

namespace aisx {

char* err_buf(); // thread-local message buffer (aisx_lib.hip)

namespace {

void tx_err(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
}

// CRC-16/X.25, bit by bit: polynomial 0x1021 reflected (0x8408), preset 0xFFFF, complemented result
unsigned x25_fcs(const uint8_t* octets, int count)
{
    unsigned reg = 0xFFFFu;
    for (int k = 0; k < count; k++) {
        reg ^= octets[k];
        for (int b = 0; b < 8; b++)
            reg = (reg >> 1) ^ ((reg & 1u) ? 0x8408u : 0u);
    }
    return ~reg & 0xFFFFu;
}

// payload + FCS, bit by bit in transmission order, with the stuffed zeros: emit(bit)
template <class Emit>
int stuffed_frame(const uint8_t* payload, int len, Emit&& emit)
{
    const unsigned fcs = x25_fcs(payload, len);
    int run = 0, count = 0;
    for (int k = 0; k < len + 2; k++) {
        const unsigned octet = k < len ? payload[k] : k == len ? (fcs & 0xFFu) : (fcs >> 8);
        for (int b = 0; b < 8; b++) {
            const unsigned bit = (octet >> b) & 1u;
            emit(bit);
            count++;
            run = bit ? run + 1 : 0;
            if (run == 5) {
                emit(0u);
                count++;
                run = 0;
            }
        }
    }
    return count;
}

} // namespace

int tx_cfg_check(double sps, double bt, int training_bits, int ramp_syms, int tail_syms)
{
    if (!(sps >= 2.0 && sps <= TX_MAX_SPS) || !(bt >= 0.1 && bt <= 1.0) || training_bits < 1 || training_bits > TX_MAX_TRAINING ||
        ramp_syms < 0 || ramp_syms > TX_MAX_RAMP || tail_syms < 0 || tail_syms > TX_MAX_TAIL) {
        tx_err("transmitter: need 2 <= sps <= %g, 0.1 <= bt <= 1, 1 <= training_bits <= %d, 0 <= ramp_syms <= %d, "
               "0 <= tail_syms <= %d", TX_MAX_SPS, TX_MAX_TRAINING, TX_MAX_RAMP, TX_MAX_TAIL);
        return AISX_ERR_INVALID;
    }
    return AISX_OK;
}

int tx_stuffed_bits(const uint8_t* payload, int len)
{
    return stuffed_frame(payload, len, [](unsigned) {});
}

int tx_bursts_check(const char* who, const aisx_burst* bursts, int n, int nchan, int length_max, const uint8_t* bytes, int64_t nbytes)
{
    if (n < 0 || nbytes < 0 || (n > 0 && (!bursts || !bytes))) {
        tx_err("%s: bursts and bytes are needed", who);
        return AISX_ERR_INVALID;
    }
    for (int k = 0; k < n; k++) {
        const aisx_burst& b = bursts[k];
        const char* bad = nullptr;
        if (b.chan < 0 || b.chan >= nchan)
            bad = "chan outside [0, nchan)";
        else if (b.len < 1 || b.len > length_max)
            bad = "len outside [1, length_max]";
        else if (b.offset < 0 || b.offset > nbytes - b.len)
            bad = "offset + len beyond the bytes";
        else if (!(b.frac >= 0.0f && b.frac < 1.0f))
            bad = "frac outside [0, 1)";
        else if (!isfinite(b.amp) || !isfinite(b.phase))
            bad = "amp or phase not finite";
        else if (!(fabsf(b.cfo) <= 0.5f))
            bad = "|cfo| above 0.5 cycles per sample";
        else if (b.start <= -(1LL << 62) || b.start >= (1LL << 62))
            bad = "|start| of 2^62 or more";
        if (bad) {
            tx_err("%s: burst %d: %s", who, k, bad);
            return AISX_ERR_INVALID;
        }
    }
    return AISX_OK;
}

double tx_qpulse(double v, double bt)
{
    if (v <= 0.0)
        return 0.0;
    if (v >= (double)TX_L)
        return 1.0;
    const double beta = M_PI * bt * sqrt(2.0 / M_LN2);
    auto F = [beta](double x) { return x * erf(beta * x) + exp(-beta * beta * x * x) / (beta * sqrt(M_PI)); };
    auto G = [&F](double x) { return 0.5 + 0.5 * (F(x + 0.5) - F(x - 0.5)); };
    const double lo = G(-0.5 * TX_L), hi = G(0.5 * TX_L);
    return (G(v - 0.5 * TX_L) - lo) / (hi - lo);
}

void tx_extent(double sps, double frac, int nsyms, int* first, int* end)
{
    *first = frac > 0.0 ? 1 : 0; // (the least d >= frac, frac in [0, 1))
    int64_t d = (int64_t)ceil((double)nsyms * sps + frac);
    while (d > 0 && !(tx_u(d - 1, frac, sps) < (double)nsyms))
        d--;
    while (tx_u(d, frac, sps) < (double)nsyms)
        d++;
    *end = (int)d;
}

} // namespace aisx

using namespace aisx;

extern "C" int aisx_hdlc_frame(const uint8_t* payload, int len, int training_bits, int ramp_syms, int tail_syms, uint8_t* levels,
                               int cap, int* nsyms)
{
    if (!payload || !nsyms || len < 1 || len > TX_MAX_OCTETS || cap < 0 || (cap > 0 && !levels) ||
        tx_cfg_check(2.0, 0.4, training_bits, ramp_syms, tail_syms) != AISX_OK)
        return AISX_ERR_INVALID;
    const int total = tx_nsyms(training_bits, ramp_syms, tail_syms, tx_stuffed_bits(payload, len));
    *nsyms = total;
    if (total > cap)
        return AISX_ERR_OVERFLOW;
    uint8_t* w = levels;
    for (int k = 0; k < ramp_syms; k++)
        *w++ = (uint8_t)((k & 1) ^ 1);
    for (int k = 0; k < training_bits; k++)
        *w++ = (uint8_t)((k & 3) < 2);
    unsigned level = w[-1];
    auto nrzi = [&](unsigned bit) {
        level ^= bit ^ 1u; // a 0 toggles, a 1 keeps
        *w++ = (uint8_t)level;
    };
    for (int b = 0; b < 8; b++)
        nrzi((0x7Eu >> b) & 1u);
    stuffed_frame(payload, len, nrzi);
    for (int b = 0; b < 8; b++)
        nrzi((0x7Eu >> b) & 1u);
    for (int k = 0; k < tail_syms; k++)
        *w++ = (uint8_t)level;
    return AISX_OK;
}

extern "C" int aisx_tx_render_host(double sps, double bt, int training_bits, int ramp_syms, int tail_syms, int nchan,
                                   const aisx_burst* bursts, int nbursts, const uint8_t* bytes, int64_t nbytes, int64_t t0, int64_t n,
                                   aisx_cf32* out, int64_t out_stride, int accumulate)
{
    if (tx_cfg_check(sps, bt, training_bits, ramp_syms, tail_syms) != AISX_OK)
        return AISX_ERR_INVALID;
    if (nchan < 1 || n < 1 || n > (1LL << 30) || !out || out_stride < n || t0 <= -(1LL << 62) || t0 >= (1LL << 62)) {
        tx_err("aisx_tx_render_host: need nchan >= 1, 1 <= n <= 2^30, out, out_stride >= n, |t0| < 2^62");
        return AISX_ERR_INVALID;
    }
    int rc = tx_bursts_check("aisx_tx_render_host", bursts, nbursts, nchan, TX_MAX_OCTETS, bytes, nbytes);
    if (rc != AISX_OK)
        return rc;
    std::vector<double> acc((size_t)nchan * (size_t)n * 2, 0.0);
    std::vector<uint8_t> lv;
    std::vector<int> S; // S[i + 1] = a_0 + ... + a_i, S[0] = 0
    const double r = ramp_syms > 0 ? 0.5 * ramp_syms : 1.0;
    for (int k = 0; k < nbursts; k++) {
        const aisx_burst& b = bursts[k];
        const uint8_t* payload = bytes + b.offset;
        int nsyms = 0;
        lv.resize((size_t)tx_max_nsyms(training_bits, ramp_syms, tail_syms, b.len));
        if ((rc = aisx_hdlc_frame(payload, b.len, training_bits, ramp_syms, tail_syms, lv.data(), (int)lv.size(), &nsyms)) != AISX_OK)
            return rc;
        S.assign((size_t)nsyms + 1, 0);
        for (int i = 0; i < nsyms; i++)
            S[(size_t)i + 1] = S[(size_t)i] + (lv[(size_t)i] ? 1 : -1);
        const double frac = (double)b.frac;
        int first, end;
        tx_extent(sps, frac, nsyms, &first, &end);
        const int64_t lo = b.start + first > t0 ? b.start + first : t0;
        const int64_t hi = b.start + end < t0 + n ? b.start + end : t0 + n;
        double* row = acc.data() + (size_t)b.chan * (size_t)n * 2;
        for (int64_t t = lo; t < hi; t++) {
            const int64_t d = t - b.start;
            const double u = tx_u(d, frac, sps);
            int m = (int)floor(u);
            m = m < 0 ? 0 : m > nsyms - 1 ? nsyms - 1 : m;
            double sum = m - TX_L >= 0 ? (double)S[(size_t)(m - TX_L) + 1] : 0.0;
            for (int j = m - TX_L + 1; j <= m; j++)
                if (j >= 0)
                    sum += (lv[(size_t)j] ? 1.0 : -1.0) * tx_qpulse(u - (double)j, bt);
            double env = u / r < ((double)nsyms - u) / r ? u / r : ((double)nsyms - u) / r;
            env = ramp_syms == 0 || env > 1.0 ? 1.0 : env < 0.0 ? 0.0 : env;
            const double ph = 0.5 * M_PI * sum + 2.0 * M_PI * (double)b.cfo * (double)d + (double)b.phase;
            const double a = (double)b.amp * env;
            row[2 * (t - t0)] += a * cos(ph);
            row[2 * (t - t0) + 1] += a * sin(ph);
        }
    }
    for (int c = 0; c < nchan; c++)
        for (int64_t i = 0; i < n; i++) {
            aisx_cf32& o = out[(size_t)c * (size_t)out_stride + (size_t)i];
            const float re = (float)acc[((size_t)c * (size_t)n + (size_t)i) * 2], im = (float)acc[((size_t)c * (size_t)n + (size_t)i) * 2 + 1];
            if (accumulate) {
                o.re += re;
                o.im += im;
            } else {
                o.re = re;
                o.im = im;
            }
        }
    return AISX_OK;
}
