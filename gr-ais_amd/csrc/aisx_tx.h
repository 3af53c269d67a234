// aisx_tx.h -- what the host specification of the transmitter (aisx_tx.cpp) and the device handle (aisx_tx.hip) share:
// argument checks, a burst's symbol count and sample extent, the phase pulse in closed form.
#pragma once
#include <stdint.h>

#include "../../include/aisx.h"

namespace aisx {

constexpr int TX_L = 4;              // symbols the phase pulse spans
constexpr int TX_MAX_OCTETS = 1023;  // payload octets, as the deframer's limit
constexpr int TX_MAX_RAMP = 64, TX_MAX_TRAINING = 256, TX_MAX_TAIL = 64;
constexpr double TX_MAX_SPS = 4096.0;

// symbols of a burst with `stuffed` data bits behind stuffing
inline int tx_nsyms(int training_bits, int ramp_syms, int tail_syms, int stuffed) { return ramp_syms + training_bits + 16 + stuffed + tail_syms; }
// the most a payload of `len` octets can come to: one stuffed bit per five of payload + FCS
inline int tx_max_nsyms(int training_bits, int ramp_syms, int tail_syms, int len)
{
    const int bits = 8 * (len + 2);
    return tx_nsyms(training_bits, ramp_syms, tail_syms, bits + bits / 5);
}

int tx_cfg_check(double sps, double bt, int training_bits, int ramp_syms, int tail_syms); // AISX_OK or AISX_ERR_INVALID
// payload + FCS behind stuffing, in bits (len checked by the caller)
int tx_stuffed_bits(const uint8_t* payload, int len);
// descriptor checks of aisx_tx_batch_set_bursts; sets the error text
int tx_bursts_check(const char* who, const aisx_burst* bursts, int n, int nchan, int length_max, const uint8_t* bytes, int64_t nbytes);
// q(v) of include/aisx.h, any v
double tx_qpulse(double v, double bt);

// u of sample d = t - start, as the specification computes it
inline double tx_u(int64_t d, double frac, double sps) { return ((double)d - frac) / sps; }
// the samples d = t - start with 0 <= u < nsyms are [*first, *end)
void tx_extent(double sps, double frac, int nsyms, int* first, int* end);

} // namespace aisx
