// aisx_mlse.cpp -- the 4-state sequence detector on the host (include/aisx.h, aisx_mlse_*): the specification of the
// device form (aisx_mlse.hip, k_mlse.h), which equals it bit for bit.  Plain C++: one channel, host pointers, the
// arithmetic of a step shared with the kernel body through k_mlse.h.
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "aisx_tx.h"
#include "k_mlse.h"

namespace aisx {

char* err_buf(); // thread-local message buffer (aisx_lib.hip)

namespace {

void mlse_err(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
}

} // namespace

// c0, c1 and the eight rotations of BT = bt GMSK sampled at the symbol boundaries, in double, rounded once to float
int mlse_model(double bt, double* c0, double* c1, MlseRot* rot)
{
    if (!(bt >= 0.1 && bt <= 1.0))
        return AISX_ERR_INVALID;
    const double a = tx_qpulse(2.5, bt) - tx_qpulse(1.5, bt), b = tx_qpulse(3.5, bt) - tx_qpulse(2.5, bt);
    for (int i = 0; i < 8; i++) {
        const int P = 2 * (i >> 2) - 1, Q = 2 * ((i >> 1) & 1) - 1, R = 2 * (i & 1) - 1;
        const double theta = M_PI / 2 * (a * Q + b * (P + R));
        rot->c[i] = (float)cos(theta);
        rot->s[i] = (float)sin(theta);
    }
    if (c0)
        *c0 = a;
    if (c1)
        *c1 = b;
    return AISX_OK;
}

} // namespace aisx

using namespace aisx;

struct aisx_mlse {
    double bt = 0, c0 = 0, c1 = 0;
    MlseRot rot = {};
    long long nseen = 0, a0 = 0; // symbols seen; hold[0] is symbol a0
    std::vector<cf> hold;
};

namespace {

// block k over the window that ends before symbol e: bits of symbols [k B, min(k B + B, e))
int decide_block(const aisx_mlse* h, long long k, long long e, uint8_t* out)
{
    const long long kb = k * MLSE_B, a = kb - MLSE_W > 0 ? kb - MLSE_W : 0;
    auto S = [h](long long n) { return n < 0 ? mk(0.f, 0.f) : h->hold[(size_t)(n - h->a0)]; };
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    unsigned char nib[MLSE_STEPS];
    for (long long n = a; n < e; n++)
        nib[n - a] = (unsigned char)mlse_step(h->rot, mlse_z(S(n), S(n - 1)), m0, m1, m2, m3);
    unsigned st = (unsigned)mlse_best(m0, m1, m2, m3);
    unsigned char lev[MLSE_B + 1] = {}; // lev[i] = b[k B - 1 + i]
    const long long lo = a > kb - 1 ? a : kb - 1;
    for (long long n = e - 1; n >= lo; n--) {
        const unsigned b = mlse_back(nib[n - a], st);
        if (n < kb + MLSE_B)
            lev[n - kb + 1] = (unsigned char)b;
    }
    if (k == 0)
        lev[0] = 0;
    const long long end = kb + MLSE_B < e ? kb + MLSE_B : e;
    for (long long n = kb; n < end; n++)
        out[n - kb] = (uint8_t)(1u ^ lev[n - kb + 1] ^ lev[n - kb]);
    return (int)(end - kb);
}

// forgets the symbols no window to come will read
void trim(aisx_mlse* h, long long kdone)
{
    const long long a1 = kdone * MLSE_B - (MLSE_W + 1) > 0 ? kdone * MLSE_B - (MLSE_W + 1) : 0;
    if (a1 > h->a0) {
        h->hold.erase(h->hold.begin(), h->hold.begin() + (size_t)(a1 - h->a0));
        h->a0 = a1;
    }
}

} // namespace

extern "C" int aisx_mlse_create(aisx_mlse** out, double bt)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    aisx_mlse* h = new aisx_mlse();
    if (mlse_model(bt, &h->c0, &h->c1, &h->rot) != AISX_OK) {
        delete h;
        mlse_err("aisx_mlse_create: need 0.1 <= bt <= 1");
        return AISX_ERR_INVALID;
    }
    h->bt = bt;
    *out = h;
    return AISX_OK;
}

extern "C" int aisx_mlse_destroy(aisx_mlse* h)
{
    delete h;
    return AISX_OK;
}

extern "C" int aisx_mlse_reset(aisx_mlse* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    h->nseen = h->a0 = 0;
    h->hold.clear();
    return AISX_OK;
}

extern "C" int aisx_mlse_model(const aisx_mlse* h, double* c0, double* c1, float* rot)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (c0)
        *c0 = h->c0;
    if (c1)
        *c1 = h->c1;
    for (int i = 0; rot && i < 8; i++) {
        rot[2 * i] = h->rot.c[i];
        rot[2 * i + 1] = h->rot.s[i];
    }
    return AISX_OK;
}

extern "C" int aisx_mlse_work(aisx_mlse* h, const aisx_cf32* syms, int n, uint8_t* bits, int cap, int* nbits)
{
    if (!h || !nbits || n < 0 || cap < 0 || (n > 0 && !syms) || (cap > 0 && !bits)) {
        mlse_err("aisx_mlse_work: need a handle, n >= 0 symbols, a bit buffer for its capacity and somewhere to put the count");
        return AISX_ERR_INVALID;
    }
    const long long kold = mlse_blocks_done(h->nseen), kend = mlse_blocks_done(h->nseen + n);
    *nbits = (int)((kend - kold) * MLSE_B);
    if (*nbits > cap) {
        mlse_err("aisx_mlse_work: the call decides %d bits, the buffer holds %d; nothing was taken", *nbits, cap);
        return AISX_ERR_OVERFLOW;
    }
    const cf* s = (const cf*)syms;
    h->hold.insert(h->hold.end(), s, s + n);
    h->nseen += n;
    for (long long k = kold; k < kend; k++)
        decide_block(h, k, k * MLSE_B + MLSE_HOLD, bits + (k - kold) * MLSE_B);
    trim(h, kend);
    return AISX_OK;
}

extern "C" int aisx_mlse_flush(aisx_mlse* h, uint8_t* bits, int cap, int* nbits)
{
    if (!h || !nbits || cap < 0 || (cap > 0 && !bits)) {
        mlse_err("aisx_mlse_flush: need a handle, a bit buffer for its capacity and somewhere to put the count");
        return AISX_ERR_INVALID;
    }
    const long long kold = mlse_blocks_done(h->nseen), N = h->nseen;
    *nbits = (int)(N - kold * MLSE_B);
    if (*nbits > cap) {
        mlse_err("aisx_mlse_flush: %d bits are left, the buffer holds %d; nothing was done", *nbits, cap);
        return AISX_ERR_OVERFLOW;
    }
    for (long long k = kold; k * MLSE_B < N; k++)
        decide_block(h, k, N, bits + (k - kold) * MLSE_B);
    return aisx_mlse_reset(h);
}
