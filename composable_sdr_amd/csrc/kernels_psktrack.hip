// pskTracker ("csdr psktrack v1"): power normaliser, carrier PLL, T/2 equaliser and BPSK / QPSK decisions on C
// independent CF32 rows, the part of liquid's symtrack_cccf (Liquid.chs:119-175) behind the symbol synchroniser.
//   k_psktrack : the whole per-sample loop, one lane per row, 64 rows per wave                          sequential in t
// The structure is k_symsyncc's (kernels_symsyncc.hip): input blocks of SB samples staged through LDS while the lanes run the
// current block, a row's slot an odd number of pairs wide.  A lane's weights and window (up to 17 complex taps each) live in LDS
// next to each other at an odd pair stride; the window is a ring whose write position starts at 0 in every call, and the state
// record in HBM holds it oldest sample first, so the arithmetic never sees where a call began.  Every loop's trip count comes
// from the launch parameters and the row's sample count (clamped to n); no index comes from sample data.
// Arithmetic contract: plain f32, no contraction, every sum in the order written here; sqrtf and / correctly rounded; sine,
// cosine and word() from psktrack_common.h.  The output is the same for every chunking of the stream, row count and row
// position, bit for bit, and tests/psktrack_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr uint32_t SL = PSK_SL, SB = PSK_SB, XS = PSK_XS;

// LDS: xs[SL][XS] pairs | win[SL][stride(L)] pairs (w[L] | buf[L] per lane)
__global__ __launch_bounds__(PSK_SL) void k_psktrack(const float2 *__restrict__ X, const uint32_t *__restrict__ NX, float2 *__restrict__ Y,
                                                     uint32_t *__restrict__ SYM, uint32_t *__restrict__ NY,
                                                     const uint32_t *__restrict__ st_in, uint32_t *__restrict__ st_out, PskLaunch l)
{
    extern __shared__ float2 ldsp[];
    const uint32_t L = l.L, ST = psk_win_stride(L), R = psk_state_words(L), n = l.n;
    float2 *xs = ldsp;
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * SL, nc = min(SL, l.C - c0);
    const bool act = lane < nc;
    const size_t rowi = c0 + (act ? lane : 0);
    float2 *wv = ldsp + SL * XS + lane * ST, *bv = wv + L;
    // element e = lane + SL q of a block (q < SB): row e / SB, step e % SB
    float2 qx[SB];
    auto load = [&](uint32_t blk) {
#pragma unroll
        for (uint32_t q = 0; q < SB; q++) {
            const uint32_t e = lane + SL * q, rw = e / SB, t = blk * SB + e % SB;
            qx[q] = (rw < nc && t < n) ? X[(size_t)(c0 + rw) * n + t] : make_float2(0.f, 0.f);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (uint32_t q = 0; q < SB; q++) {
            const uint32_t e = lane + SL * q;
            xs[(e / SB) * XS + e % SB] = qx[q];
        }
    };
    // the row's state: a record whose first word is 0 is the state right after new
    float p = 1.f;
    uint32_t theta = 0, freq = 0, par = 0, nsym = 0, nx = 0;
    if (act) {
        const uint32_t *s = st_in + rowi * R;
        const bool live = s[0] != 0u;
        if (live) { p = __uint_as_float(s[1]); theta = s[2]; freq = s[3]; par = s[4]; nsym = s[5]; }
        for (uint32_t i = 0; i < L; i++) {
            const uint32_t *q = s + PSK_HDR + 2 * i;
            wv[i] = live ? make_float2(__uint_as_float(q[0]), __uint_as_float(q[1])) : make_float2(2 * i + 1 == L ? 1.f : 0.f, 0.f);
            bv[i] = live ? make_float2(__uint_as_float(q[2 * L]), __uint_as_float(q[2 * L + 1])) : make_float2(0.f, 0.f);
        }
        nx = NX ? min(NX[rowi], n) : n;
    }
    const uint32_t cpar = L ? ((L - 1) / 2) & 1u : 0u;     // an output is due when the sample under the centre tap has parity phase
    uint32_t pos = 0, cnt = 0;                              // ring: the next write, which is also the oldest sample
    float2 *yrow = Y + rowi * n;
    uint32_t *srow = SYM ? SYM + rowi * n : nullptr;
    const float2 *row = xs + lane * XS;
    const uint32_t nb = (n + SB - 1) / SB;
    if (nb) { load(0); stage(); }
    __syncthreads();
    for (uint32_t blk = 0; blk < nb; blk++) {
        if (blk + 1 < nb) load(blk + 1);                               // in flight while the recurrence runs
        const uint32_t t0 = blk * SB, steps = min(SB, n - t0);
        for (uint32_t j = 0; j < steps; j++) {
            if (t0 + j >= nx) break;
            const float2 v = row[j];
            // 1. power normaliser
            const float m2 = v.x * v.x + v.y * v.y;
            p = p + l.agc_bw * (m2 - p);
            p = p < PSK_P_MIN ? PSK_P_MIN : p;
            const float g = sqrtf(p);
            const float vr = v.x / g, vi = v.y / g;
            // 2. derotation
            float sn, cs;
            psk_sincos_word(theta, &sn, &cs);
            const float ur = vr * cs + vi * sn, ui = vi * cs - vr * sn;
            theta += freq;
            // 3. window and symbol decimation
            if (L) { bv[pos] = make_float2(ur, ui); pos = pos + 1 == L ? 0 : pos + 1; }
            const bool inst = l.sps == 1 || ((par + cpar) & 1u) == l.phase;
            par ^= 1u;
            if (!inst) continue;
            float dr = ur, di = ui, E = 0.f;
            if (L) {
                dr = 0.f; di = 0.f;
                uint32_t idx = pos;
                for (uint32_t i = 0; i < L; i++) {
                    const float2 w = wv[i], b = bv[idx];
                    idx = idx + 1 == L ? 0 : idx + 1;
                    dr = dr + (w.x * b.x + w.y * b.y);                 // conj(w) b
                    di = di + (w.x * b.y - w.y * b.x);
                    E = E + (b.x * b.x + b.y * b.y);
                }
            }
            // 4. decision
            const bool bI = dr < 0.f, bQ = l.bits == 2 && di < 0.f;
            float hr, hi;
            if (l.bits == 1) { hr = bI ? -1.f : 1.f; hi = 0.f; }
            else { hr = bI ? -PSK_A_QPSK : PSK_A_QPSK; hi = bQ ? -PSK_A_QPSK : PSK_A_QPSK; }
            const uint32_t k = (bI ? 1u : 0u) | (bQ ? 2u : 0u);
            // 5. phase error and PLL
            const float e = di * hr - dr * hi;                         // Im(d conj(x_hat))
            freq += psk_word(l.alpha * e);
            theta += psk_word(l.beta * e);
            // 6. equaliser update
            if (L && nsym >= l.delay) {
                float er, ei;
                if (l.mode == CSDR_PSKTRACK_EQ_DD) { er = hr - dr; ei = hi - di; }
                else {
                    const float r = sqrtf(dr * dr + di * di);
                    const bool ok = r > 0.f;
                    const float rs = ok ? r : 1.f;
                    er = ok ? dr / rs - dr : 0.f;
                    ei = ok ? di / rs - di : 0.f;
                }
                const float gn = l.mu / (E + PSK_EQ_EPS);
                uint32_t idx = pos;
                for (uint32_t i = 0; i < L; i++) {
                    const float2 b = bv[idx];
                    idx = idx + 1 == L ? 0 : idx + 1;
                    float2 w = wv[i];
                    w.x = w.x + gn * (er * b.x + ei * b.y);            // conj(err) b
                    w.y = w.y + gn * (er * b.y - ei * b.x);
                    wv[i] = w;
                }
            }
            nsym += nsym != 0xffffffffu ? 1u : 0u;
            // 7. output
            yrow[cnt] = make_float2(dr, di);
            if (srow) srow[cnt] = k;
            cnt++;
        }
        __syncthreads();
        if (blk + 1 < nb) stage();
        __syncthreads();
    }
    if (act) {
        uint32_t *s = st_out + rowi * R;
        s[0] = 1u; s[1] = __float_as_uint(p); s[2] = theta; s[3] = freq; s[4] = par; s[5] = nsym; s[6] = 0u; s[7] = 0u;
        uint32_t idx = pos;
        for (uint32_t i = 0; i < L; i++) {
            uint32_t *q = s + PSK_HDR + 2 * i;
            const float2 w = wv[i], b = bv[idx];
            idx = idx + 1 == L ? 0 : idx + 1;
            q[0] = __float_as_uint(w.x); q[1] = __float_as_uint(w.y);
            q[2 * L] = __float_as_uint(b.x); q[2 * L + 1] = __float_as_uint(b.y);
        }
        NY[rowi] = cnt;
    }
}

}  // namespace

int launch_psktrack(const float2 *x, const uint32_t *nx, float2 *y, uint32_t *sym, uint32_t *ny, const uint32_t *st_in,
                    uint32_t *st_out, const PskLaunch &l, hipStream_t s)
{
    if (!l.C) return 0;
    hipLaunchKernelGGL(k_psktrack, dim3((l.C + SL - 1) / SL), dim3(SL), psk_lds_bytes(l.L), s, x, nx, y, sym, ny, st_in, st_out, l);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
