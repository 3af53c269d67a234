// k_mlse.h -- the 4-state sequence detector behind the timing recovery (include/aisx.h, aisx_mlse_*): what the host
// form (aisx_mlse.cpp, the specification) and the device form share -- the differential symbol, the branch metric, one
// step of the recursion, the choice of the best state, one step of the trace back -- and the device form's kernel body.
//
// Levels b[n] in {0, 1}; z[n] = s[n] conj(s[n-1]) turns by theta(b[n-1], b[n], b[n+1]); the path metric M[2 p + q] entering
// step n belongs to (b[n-1], b[n]) = (p, q), and step n extends it by r = b[n+1]:
//     cand_p = M[2 p + q] + g(n; p, q, r),    survivor p = cand_1 > cand_0,    M'[2 q + r] = the chosen candidate.
// Blocks of MLSE_B symbols by absolute index are decided independently, each over its own window of MLSE_W more symbols
// on either side with all metrics starting at 0, so a lane needs nobody else's decision.
//
// The kernel: one wave per workgroup, lane l decides block k0 + l.  The wave stages the z of its 64 blocks and their
// overlap -- 4128 values, 32.25 KB -- in LDS with coalesced loads (a lane reads its 96 at a stride of one block, 512 B,
// which global memory would serve a line per lane), one slot of padding per 64 so that the lanes of a half wave read 32
// different bank pairs.  Survivors: 4 bits a step, one word per 8 steps, written to LDS as each word fills and read back
// in reverse by the trace back -- registers hold one word at a time, nothing is indexed dynamically.  The 64 decisions of
// a lane leave as one 64-bit word, transposed by wave shuffles into 64 coalesced byte stores.
#pragma once
#include "aisx_common.h"

namespace aisx {

constexpr int MLSE_B = 64;                           // symbols a block decides
constexpr int MLSE_W = 16;                           // overlap on each side
constexpr int MLSE_STEPS = MLSE_B + 2 * MLSE_W;      // steps of a full window
constexpr int MLSE_HOLD = MLSE_B + MLSE_W;           // block k is decided once k B + MLSE_HOLD symbols have been seen
constexpr int MLSE_CARRY = MLSE_B + 2 * MLSE_W + 1;  // undecided symbols a channel carries at most (96 are ever held)
constexpr int MLSE_EXTRA = MLSE_B + MLSE_W - 1;      // a call of n symbols emits at most n + MLSE_EXTRA bits
constexpr int MLSE_T = 64;                           // threads of a workgroup: one wave
constexpr int MLSE_TILE = MLSE_T * MLSE_B + 2 * MLSE_W;          // z values a wave stages
constexpr int MLSE_ZSLOTS = MLSE_TILE + (MLSE_TILE + 63) / 64;   // with one slot of padding per 64
constexpr int MLSE_SVWORDS = MLSE_STEPS / 8;
constexpr int MLSE_LDS_BYTES = MLSE_ZSLOTS * 8 + MLSE_SVWORDS * MLSE_T * 4;
enum { MLSE_ST_BAD_COUNT = 1 };

// (cos theta, sin theta) of the eight level triples, index 4 p + 2 q + r
struct MlseRot {
    float c[8], s[8];
};

// the model of BT = bt GMSK (aisx_mlse.cpp, in double): AISX_OK, or AISX_ERR_INVALID outside 0.1 <= bt <= 1
int mlse_model(double bt, double* c0, double* c1, MlseRot* rot);

struct MlseState {
    long long nseen; // symbols of the channel seen so far
    int ncarry;      // of which the last ncarry are in the carry buffer
    int pad;
};

// blocks decided once n symbols have been seen
AISX_HD long long mlse_blocks_done(long long n) { return n < MLSE_HOLD ? 0 : (n - MLSE_HOLD) / MLSE_B + 1; }

// z = a conj(b): re = a.re b.re + a.im b.im, im = a.im b.re - a.re b.im, one product rounded and one fused step each
AISX_HD cf mlse_z(cf a, cf b) { return mk(fmaf(a.im, b.im, a.re * b.re), fmaf(a.im, b.re, -(a.re * b.im))); }

// one step of the recursion on z; returns the four survivor bits, bit 2 q + r = the predecessor p of the new state (q, r)
AISX_HD unsigned mlse_step(const MlseRot& R, cf z, float& m0, float& m1, float& m2, float& m3)
{
    float nm[4];
    unsigned nib = 0;
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i0 = 2 * q + r, i1 = 4 + 2 * q + r;
            const float g0 = fmaf(z.im, R.s[i0], z.re * R.c[i0]);
            const float g1 = fmaf(z.im, R.s[i1], z.re * R.c[i1]);
            const float c0 = (q ? m1 : m0) + g0;
            const float c1 = (q ? m3 : m2) + g1;
            const bool one = c1 > c0;
            nm[2 * q + r] = one ? c1 : c0;
            nib |= (one ? 1u : 0u) << (2 * q + r);
        }
    m0 = nm[0];
    m1 = nm[1];
    m2 = nm[2];
    m3 = nm[3];
    return nib;
}

// the lowest state whose metric is maximal
AISX_HD int mlse_best(float m0, float m1, float m2, float m3)
{
    int best = 0;
    float bm = m0;
    if (m1 > bm) {
        bm = m1;
        best = 1;
    }
    if (m2 > bm) {
        bm = m2;
        best = 2;
    }
    if (m3 > bm)
        best = 3;
    return best;
}

// the state (q, r) of a step and that step's survivor bits: returns b = q and moves `st` to the step before
AISX_HD unsigned mlse_back(unsigned nib, unsigned& st)
{
    const unsigned b = st >> 1, p = (nib >> st) & 1u;
    st = (p << 1) | b;
    return b;
}

struct MlseParams {
    const cf* syms; long long sym_stride; // [nchan][sym_stride]; nullptr at a flush
    const int* nsyms;                      // [nchan] on the device; nullptr at a flush
    int max_syms;
    unsigned char* bits; long long bit_stride;
    int* nbits;                            // [nchan]
    const MlseState* st_in; MlseState* st_out;
    const cf* carry_in; cf* carry_out;     // [nchan][MLSE_CARRY]
    int* flag;
    MlseRot rot;
};

// symbol n of a channel: 0 outside what the carry and the call's input hold
struct MlseView {
    const cf* carry; const cf* in;
    long long a0, nend; // the carry starts at symbol a0, the input ends before symbol nend
    int cn;
};
AISX_DI cf mlse_sym(const MlseView& v, long long n)
{
    if (n < v.a0 || n >= v.nend)
        return mk(0.f, 0.f);
    const long long i = n - v.a0;
    return i < v.cn ? v.carry[i] : v.in[i - v.cn];
}

AISX_HD int mlse_zslot(int t) { return t + (t >> 6); }

// workgroup (ch, by): the 64 blocks from (blocks done before the call) + 64 by of channel ch = bx.  CUT: a flush -- the
// windows end at the last symbol seen, every block that has a symbol is decided, and the channel is left empty.
template <class Ctx, bool CUT>
AISX_DI void mlse_body(Ctx& cx, const MlseParams& p)
{
    const int ch = cx.bx(), grp = cx.by(), l = cx.tid();
    cf* zt = (cf*)cx.lds();
    unsigned* sv = (unsigned*)(cx.lds() + (size_t)MLSE_ZSLOTS * 8);
    const MlseState st = p.st_in[ch];
    int nin = 0;
    if (!CUT) {
        nin = p.nsyms[ch];
        if (nin < 0 || nin > p.max_syms) {
            nin = 0;
            if (grp == 0 && l == 0)
                *p.flag = MLSE_ST_BAD_COUNT;
        }
    }
    MlseView v;
    v.carry = p.carry_in + (long long)ch * MLSE_CARRY;
    v.in = CUT ? v.carry : p.syms + (long long)ch * p.sym_stride; // (a flush has no input: nend ends the carry)
    v.cn = st.ncarry;
    v.a0 = st.nseen - st.ncarry;
    v.nend = st.nseen + nin;
    const long long N = v.nend;
    const long long kold = mlse_blocks_done(st.nseen);
    const long long kend = CUT ? (N + MLSE_B - 1) / MLSE_B : mlse_blocks_done(N);
    if (grp == 0) { // the channel's state behind this call, into the other buffer: the other workgroups read this one
        const long long a1 = kend * MLSE_B - (MLSE_W + 1) > 0 ? kend * MLSE_B - (MLSE_W + 1) : 0;
        const int keep = CUT ? 0 : (int)(N - a1);
        cf* co = p.carry_out + (long long)ch * MLSE_CARRY;
        for (int i = l; i < keep; i += MLSE_T)
            co[i] = mlse_sym(v, a1 + i);
        if (l == 0) {
            MlseState so;
            so.nseen = CUT ? 0 : N;
            so.ncarry = keep;
            so.pad = 0;
            p.st_out[ch] = so;
            p.nbits[ch] = CUT ? (int)(N - kold * MLSE_B > 0 ? N - kold * MLSE_B : 0) : (int)((kend - kold) * MLSE_B);
        }
    }
    const long long k0 = kold + (long long)grp * MLSE_T;
    if (k0 >= kend)
        return;
    // z[nb + t], t = 0 .. MLSE_TILE - 1, with s[n - 1] from the lane below (lane 0 reads it)
    const long long nb = k0 * MLSE_B - MLSE_W;
    for (int t0 = 0; t0 < MLSE_TILE; t0 += MLSE_T) {
        const int t = t0 + l;
        const cf cur = mlse_sym(v, nb + t);
        cf prev;
        prev.re = cx.shfl_f32(cur.re, l > 0 ? l - 1 : 0);
        prev.im = cx.shfl_f32(cur.im, l > 0 ? l - 1 : 0);
        if (l == 0)
            prev = mlse_sym(v, nb + t - 1);
        if (t < MLSE_TILE)
            st8(&zt[mlse_zslot(t)], mlse_z(cur, prev));
    }
    cx.sync();
    const long long k = k0 + l;
    // the last step of this lane's window (step j is symbol k B - W + j)
    int jl = MLSE_STEPS - 1;
    if (CUT) {
        const long long m = N - 1 - (k * MLSE_B - MLSE_W);
        jl = m < MLSE_STEPS - 1 ? (int)m : MLSE_STEPS - 1;
    }
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    unsigned best = 0;
    const cf* zl = zt + l * (MLSE_B + 1);
    for (int w = 0; w < MLSE_SVWORDS; w++) {
        unsigned word = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int j = 8 * w + i;
            const cf z = ld8(&zl[j + (j >> 6)]);
            if (!CUT || j <= jl) {
                word |= mlse_step(p.rot, z, m0, m1, m2, m3) << (4 * i);
                if (CUT && j == jl)
                    best = (unsigned)mlse_best(m0, m1, m2, m3);
            }
        }
        sv[w * MLSE_T + l] = word;
    }
    if (!CUT)
        best = (unsigned)mlse_best(m0, m1, m2, m3);
    // back from the last step: b of steps W .. W + B - 1 (the block) and of step W - 1 (block 0: b[-1] = 0)
    unsigned state = best;
    unsigned long long lv = 0;
    unsigned bprev = 0;
    for (int w = MLSE_SVWORDS - 1; w >= 0; w--) {
        const unsigned word = sv[w * MLSE_T + l];
#pragma unroll
        for (int i = 7; i >= 0; i--) {
            const int j = 8 * w + i;
            if (CUT && j > jl)
                continue;
            if (j < MLSE_W - 1)
                continue;
            const unsigned b = mlse_back((word >> (4 * i)) & 15u, state);
            if (j >= MLSE_W + MLSE_B)
                continue; // (the overlap behind the block only leads the path here)
            if (j >= MLSE_W)
                lv |= (unsigned long long)b << (j - MLSE_W);
            else
                bprev = k > 0 ? b : 0u;
        }
    }
    const unsigned long long outw = ~(lv ^ ((lv << 1) | bprev));
    unsigned char* ob = p.bits + (long long)ch * p.bit_stride + (k0 - kold) * MLSE_B;
    for (int m = 0; m < MLSE_T; m++) {
        const unsigned long long w = cx.shfl_u64(outw, m);
        const long long kk = k0 + m;
        if (kk >= kend)
            break;
        const long long left = N - kk * MLSE_B;
        const int nv = CUT && left < MLSE_B ? (int)left : MLSE_B;
        if (l < nv)
            ob[m * MLSE_B + l] = (unsigned char)((w >> l) & 1ull);
    }
}

// ------------------------------------------------------------------
// The launch plan of aisx_mlse_batch_* (host only): the argument check, the derived sizes, the buffers and the
// per-call sequence.  aisx_mlse.hip runs it on device memory, tests/emul_mlse on host memory.
// ------------------------------------------------------------------
enum { MLSE_K_PROCESS, MLSE_K_FLUSH };

struct MlseBufs {
    MlseState* st[2];
    cf* carry[2]; // [nchan][MLSE_CARRY]
    int* flag;
};

struct MlsePlan {
    int nchan, max_syms, groups;
    int cur = 0; // which state / carry buffer the calls issued so far leave the channels in
    MlseRot rot;
    PlanBuf st, carry, flag;

    // the argument check of aisx_mlse_batch_create (bt_ok: mlse_model took the bt): nullptr when it passes
    static const char* check(int nchan, int max_syms, bool bt_ok)
    {
        if (nchan < 1 || nchan > (1 << 20) || max_syms < 1 || max_syms > (1 << 27) || !bt_ok)
            return "need 0.1 <= bt <= 1, 1 <= nchan <= 2^20 and 1 <= max_syms <= 2^27";
        return nullptr;
    }
    MlsePlan(const MlseRot& rot_, int nchan_, int max_syms_) : nchan(nchan_), max_syms(max_syms_), rot(rot_)
    {
        // a call decides at most (max_syms + MLSE_B - 1) / MLSE_B blocks of a channel
        const int blocks = (max_syms + MLSE_B - 1) / MLSE_B;
        groups = (blocks + MLSE_T - 1) / MLSE_T;
        groups = groups < 1 ? 1 : groups;
        st = { (size_t)nchan, true };
        carry = { (size_t)nchan * MLSE_CARRY, true };
        flag = { 1, true };
    }
    void reset() { cur = 0; }

    // a call with symbols, or (syms == nullptr) the flush: one launch, after which the buffers have changed roles
    template <class Launch>
    bool process(const MlseBufs& b, const cf* syms, long syms_stride, const int* nsyms, unsigned char* bits, long bits_stride,
                 int* nbits, Launch&& launch)
    {
        MlseParams p = {};
        p.max_syms = max_syms;
        p.bits = bits;
        p.bit_stride = bits_stride;
        p.nbits = nbits;
        p.st_in = b.st[cur];
        p.st_out = b.st[cur ^ 1];
        p.carry_in = b.carry[cur];
        p.carry_out = b.carry[cur ^ 1];
        p.flag = b.flag;
        p.rot = rot;
        p.syms = syms;
        p.sym_stride = syms_stride;
        p.nsyms = nsyms;
        // (at a flush at most two blocks of a channel are left)
        const PlanLaunch l = { syms ? MLSE_K_PROCESS : MLSE_K_FLUSH, nchan, syms ? groups : 1, MLSE_T, MLSE_LDS_BYTES };
        if (!launch(l, p))
            return false;
        cur ^= 1;
        return true;
    }
};

} // namespace aisx
