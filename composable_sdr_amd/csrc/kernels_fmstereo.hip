// Stereo FM decoder: stereoFMDecoder' quadRate decim (Liquid.chs:985-1078) on `C` independent F32 MPX streams [C][n]
// (DESIGN.md 4.9).  Per stream, with s[t] = x[t - d] the delayed wire (Trans.hs:86-104, as a constant delay):
//   k_fms_front  : p = mixUp ncoF . firPilot . mixDown ncoF (x + 0j)  and  lpr = Re firLPR(s)     parallel over (tile, stream)
//   k_fms_pll    : pllStep (Liquid.chs:972-989): one lane per stream, u[t] = s[t] cos(phase(theta_SS))  sequential in t
//   k_fms_back   : lmr = 2 Re firLMR(u);  L = lpr + lmr, R = lpr - lmr  into [2C][n] planes           parallel over (tile, stream)
//   k_fms_deemph : iirFilter 2 (5000 / q) 0 10 10 on every plane row, one lane per row              sequential in t
//   k_fms_decim  : firDecimator decim on L and R, written interleaved L, R, L, R ... [C][2 (n / M)]   parallel
// The NCO phase of sample t is theta_0 + t d_nco (uint32 wrap: exact for any chunking).  The two sequential kernels run the
// reference's recurrences in order; every other kernel computes each output from the same operands in the same order whatever
// the call boundaries, so the output does not depend on how the stream is chunked, bit for bit.
#include "../../include/csdr.h"
#include "csdr_internal.h"

namespace csdr {

namespace {

constexpr int FT = 256;     // outputs per workgroup of the parallel kernels
constexpr int SB = 16;      // time steps per LDS block of the sequential kernels
constexpr int SL = 64;      // streams (rows) per workgroup of the sequential kernels: one wave, one lane each

// nco_crcf_get_phase: 2 pi theta / 2^32 with theta converted to f32 first (nco_phasor in design.cpp)
__device__ __forceinline__ float fms_phase(uint32_t th) { return (float)(6.283185307179586 * (double)(float)th / 4294967296.0); }

// nco_crcf's constrain: float radians -> uint32 phase word (as nco_freq_word in design.cpp, including the
// f32 * 2^32 == 2^32 case, which wraps to 0 as the x86-64 conversion does)
__device__ __forceinline__ uint32_t fms_constrain(float x)
{
    const float p = (float)((double)x * 0.159154943091895);
    float fp = p - (float)(long long)p;
    if (fp < 0.f) fp = (float)((double)fp + 1.0);
    return (uint32_t)(unsigned long long)(fp * 4294967296.0f);
}

// Haskell's `phase` on Complex Float: GHC's class-default atan2 (atan (y / x) plus quadrant fixes), not atan2f
__device__ __forceinline__ float hs_atan2(float y, float x)
{
    const float PI_F = 3.14159265358979323846f;
    const bool neg = (x <= 0.f && y < 0.f) || (x < 0.f && y == 0.f && signbit(y)) || (x == 0.f && signbit(x) && y == 0.f && signbit(y));
    if (neg) y = -y;
    float r;
    if (x > 0.f) r = atanf(y / x);
    else if (x == 0.f && y > 0.f) r = PI_F / 2.f;
    else if (x < 0.f && y > 0.f) r = PI_F + atanf(y / x);
    else if (y == 0.f && (x < 0.f || (x == 0.f && signbit(x)))) r = PI_F;
    else if (x == 0.f && y == 0.f) r = y;
    else r = x + y;
    return neg ? -r : r;
}

// LDS: xm[N - 1 + FT] float2 | hp[N] | ha[N] | xs[Hx + FT], Hx = N - 1 + d
__global__ __launch_bounds__(FT) void k_fms_front(const float *__restrict__ mpx, const float *__restrict__ xh_in, float *__restrict__ xh_out,
                                                  const float *__restrict__ hp, const float *__restrict__ ha, float2 *__restrict__ P,
                                                  float *__restrict__ LPR, uint32_t n, uint32_t N, uint32_t d, uint32_t theta0, uint32_t dnco,
                                                  float sp, float sa)
{
    extern __shared__ float2 lds2[];
    const uint32_t Hx = N - 1 + d, c = blockIdx.y, t0 = blockIdx.x * FT, tid = threadIdx.x;
    float2 *xm = lds2;
    float *hsp = (float *)(xm + (N - 1 + FT)), *hsa = hsp + N, *xs = hsa + N;
    const float *row = mpx + (size_t)c * n, *hin = xh_in + (size_t)c * Hx;
    for (uint32_t i = tid; i < N; i += FT) { hsp[i] = hp[i]; hsa[i] = ha[i]; }
    // x at call positions r = t0 - Hx + j (history in front of the call, 0 behind its end)
    for (uint32_t j = tid; j < Hx + FT; j += FT) {
        const int64_t r = (int64_t)t0 - Hx + j;
        xs[j] = r < 0 ? hin[Hx + r] : (r < (int64_t)n ? row[r] : 0.f);
    }
    __syncthreads();
    // mixDown: x conj(v) at positions r = t0 - (N - 1) + j
    for (uint32_t j = tid; j < N - 1 + FT; j += FT) {
        const int64_t r = (int64_t)t0 - (N - 1) + j;
        const uint32_t th = theta0 + (uint32_t)r * dnco;
        float sn, cs;
        sincosf(fms_phase(th), &sn, &cs);
        const float xv = xs[j + d];
        xm[j] = make_float2(xv * cs, -(xv * sn));
    }
    __syncthreads();
    const uint32_t t = t0 + tid;
    if (t < n) {
        float ar = 0.f, ai = 0.f, al = 0.f;
        const float2 *w = xm + tid + N - 1;
        const float *ws = xs + tid + Hx - d;
        for (uint32_t k = 0; k < N; k++) {
            const float h = hsp[k], g = hsa[k];
            const float2 v = w[-(int)k];
            ar = fmaf(h, v.x, ar); ai = fmaf(h, v.y, ai);
            al = fmaf(g, ws[-(int)k], al);
        }
        const float zr = ar * sp, zi = ai * sp;
        float sn, cs;
        sincosf(fms_phase(theta0 + t * dnco), &sn, &cs);
        P[(size_t)c * n + t] = make_float2(zr * cs - zi * sn, zr * sn + zi * cs);      // mixUp
        LPR[(size_t)c * n + t] = al * sa;
    }
    // the first workgroup of every stream moves the input history forward: the last Hx samples of (history | call)
    if (blockIdx.x == 0)
        for (uint32_t i = tid; i < Hx; i += FT) {
            const int64_t r = (int64_t)n - Hx + i;
            xh_out[(size_t)c * Hx + i] = r >= 0 ? row[r] : hin[Hx + r];
        }
}

// pllStep on stream c = blockIdx.x * SL + lane.  The whole wave stages the next SB steps of p and s for its SL streams into
// LDS while every lane runs the current SB steps of its own recurrence; u goes out through LDS in the same layout.
__global__ __launch_bounds__(SL) void k_fms_pll(const float2 *__restrict__ P, const float *__restrict__ xh_in, const float *__restrict__ mpx,
                                                float *__restrict__ ub, uint2 *__restrict__ pll, uint32_t C, uint32_t n, uint32_t N,
                                                uint32_t d, uint32_t ustride, float alpha, float beta)
{
    __shared__ float2 ps[2][SL][SB + 1];
    __shared__ float ss[2][SL][SB + 1];
    __shared__ float us[SL][SB + 1];
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * SL, nc = min((uint32_t)SL, C - c0), Hx = N - 1 + d;
    const uint32_t nb = (n + SB - 1) / SB;
    // element e = lane + SL k of a block (k < SB): stream row e / SB, step e % SB
    constexpr int PER = SB;
    float2 qp[PER]; float qs[PER];
    auto load = [&](uint32_t b) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t e = lane + SL * k, rw = e / SB, st = e % SB, t = b * SB + st, cc = c0 + rw;
            const bool ok = rw < nc && t < n;
            const int64_t r = (int64_t)t - d;
            qp[k] = ok ? P[(size_t)cc * n + t] : make_float2(0.f, 0.f);
            qs[k] = ok ? (r < 0 ? xh_in[(size_t)cc * Hx + Hx + r] : mpx[(size_t)cc * n + r]) : 0.f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t e = lane + SL * k;
            ps[buf][e / SB][e % SB] = qp[k]; ss[buf][e / SB][e % SB] = qs[k];
        }
    };
    const bool act = lane < nc;
    uint32_t th = 0, dth = 0;
    if (act) { const uint2 w = pll[c0 + lane]; th = w.x; dth = w.y; }
    if (nb) { load(0); stage(0); }
    __syncthreads();
    for (uint32_t b = 0; b < nb; b++) {
        const int cur = b & 1;
        if (b + 1 < nb) load(b + 1);                         // in flight while the recurrence runs
        const uint32_t steps = min((uint32_t)SB, n - b * SB);
        if (act) {
            for (uint32_t j = 0; j < steps; j++) {
                const float2 pv = ps[cur][lane][j];
                const float sv = ss[cur][lane][j];
                const float phi = fms_phase(th);
                const uint32_t th_ss = fms_constrain(2.f * phi);          // ncoSS set_phase (2 phi)
                float sn, cs;
                sincosf(phi, &sn, &cs);                                  // ncoPE cexpf
                const float re = pv.x * cs - pv.y * (-sn), im = pv.x * (-sn) + pv.y * cs;   // p * conjugate c
                const float e = hs_atan2(im, re);
                dth += fms_constrain(e * alpha);                         // nco_crcf_pll_step
                th += fms_constrain(e * beta);
                th += dth;                                               // nco_crcf_step
                us[lane][j] = sv * cosf(fms_phase(th_ss));               // Re mix_block_down ncoSS (s + 0j)
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t e = lane + SL * k, rw = e / SB, st = e % SB, t = b * SB + st;
            if (rw < nc && t < n) ub[(size_t)(c0 + rw) * ustride + (N - 1) + t] = us[rw][st];
        }
        if (b + 1 < nb) stage(cur ^ 1);
        __syncthreads();
    }
    if (act) pll[c0 + lane] = make_uint2(th, dth);
}

// LDS: ha[N] | us[N - 1 + FT]
__global__ __launch_bounds__(FT) void k_fms_back(const float *__restrict__ ub, float *__restrict__ ub_next, const float *__restrict__ ha,
                                                 const float *__restrict__ LPR, float *__restrict__ LR, uint32_t n, uint32_t N, uint32_t ustride,
                                                 float sa)
{
    extern __shared__ float lds1[];
    const uint32_t c = blockIdx.y, t0 = blockIdx.x * FT, tid = threadIdx.x;
    float *hs = lds1, *us = lds1 + N;
    const float *urow = ub + (size_t)c * ustride;            // u[t] at urow[N - 1 + t], t >= -(N - 1)
    for (uint32_t i = tid; i < N; i += FT) hs[i] = ha[i];
    for (uint32_t j = tid; j < N - 1 + FT; j += FT) us[j] = t0 + j < N - 1 + n ? urow[t0 + j] : 0.f;
    __syncthreads();
    const uint32_t t = t0 + tid;
    if (t < n) {
        float acc = 0.f;
        const float *w = us + tid + N - 1;
        for (uint32_t k = 0; k < N; k++) acc = fmaf(hs[k], w[-(int)k], acc);
        const float lmr = 2.f * (acc * sa), lpr = LPR[(size_t)c * n + t];
        LR[(size_t)(2 * c) * n + t] = lpr + lmr;
        LR[(size_t)(2 * c + 1) * n + t] = lpr - lmr;
    }
    if (blockIdx.x == 0)
        for (uint32_t i = tid; i < N - 1; i += FT) ub_next[(size_t)c * ustride + i] = urow[n + i];
}

// iirfilt_rrrf execute_df2 on rows [R][n] in place, one lane per row, inputs staged like k_fms_pll's
__global__ __launch_bounds__(SL) void k_fms_deemph(float *__restrict__ X, float2 *__restrict__ st, uint32_t R, uint32_t n, float b0, float b1,
                                                   float b2, float a1, float a2)
{
    __shared__ float xs[2][SL][SB + 1];
    __shared__ float ys[SL][SB + 1];
    const uint32_t lane = threadIdx.x, r0 = blockIdx.x * SL, nr = min((uint32_t)SL, R - r0), nb = (n + SB - 1) / SB;
    float q[SB];
    auto load = [&](uint32_t b) {
#pragma unroll
        for (int k = 0; k < SB; k++) {
            const uint32_t e = lane + SL * k, rw = e / SB, t = b * SB + e % SB;
            q[k] = rw < nr && t < n ? X[(size_t)(r0 + rw) * n + t] : 0.f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int k = 0; k < SB; k++) { const uint32_t e = lane + SL * k; xs[buf][e / SB][e % SB] = q[k]; }
    };
    const bool act = lane < nr;
    float v1 = 0.f, v2 = 0.f;
    if (act) { const float2 w = st[r0 + lane]; v1 = w.x; v2 = w.y; }
    if (nb) { load(0); stage(0); }
    __syncthreads();
    for (uint32_t b = 0; b < nb; b++) {
        const int cur = b & 1;
        if (b + 1 < nb) load(b + 1);
        const uint32_t steps = min((uint32_t)SB, n - b * SB);
        if (act)
            for (uint32_t j = 0; j < steps; j++) {
                const float v0 = xs[cur][lane][j] - a1 * v1 - a2 * v2;
                ys[lane][j] = b0 * v0 + b1 * v1 + b2 * v2;
                v2 = v1; v1 = v0;
            }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SB; k++) {
            const uint32_t e = lane + SL * k, rw = e / SB, t = b * SB + e % SB;
            if (rw < nr && t < n) X[(size_t)(r0 + rw) * n + t] = ys[rw][e % SB];
        }
        if (b + 1 < nb) stage(cur ^ 1);
        __syncthreads();
    }
    if (act) st[r0 + lane] = make_float2(v1, v2);
}

// y[j] = sum_i h[i] x[jM - i] on the L and R rows of stream c, written interleaved; consumes floor(n / M) M samples per call
// (firdecim_rrrf_execute_block with the reference's `div`), the rest of the call never enters the window
__global__ __launch_bounds__(256) void k_fms_decim(const float *__restrict__ LR, float *__restrict__ out, uint32_t n, uint32_t M,
                                                   const float *__restrict__ h, uint32_t h_len, const float *__restrict__ hist_in,
                                                   float *__restrict__ hist_out)
{
    const uint32_t c = blockIdx.y, no = n / M, H = h_len - 1, j = blockIdx.x * 256 + threadIdx.x;
    if (j < no) {
#pragma unroll
        for (uint32_t ch = 0; ch < 2; ch++) {
            const float *row = LR + (size_t)(2 * c + ch) * n, *hin = hist_in + (size_t)(2 * c + ch) * H;
            const int64_t t0 = (int64_t)j * M;
            float acc = 0.f;
            for (uint32_t i = 0; i < h_len; i++) {
                const int64_t t = t0 - i;
                acc = fmaf(h[i], t >= 0 ? row[t] : hin[(int64_t)H + t], acc);
            }
            out[(size_t)c * 2 * no + 2 * j + ch] = acc;
        }
    }
    if (blockIdx.x == 0) {
        const int64_t nu = (int64_t)no * M;
        for (uint32_t ch = 0; ch < 2; ch++) {
            const float *row = LR + (size_t)(2 * c + ch) * n, *hin = hist_in + (size_t)(2 * c + ch) * H;
            for (uint32_t i = threadIdx.x; i < H; i += 256) {
                const int64_t t = nu - H + i;
                hist_out[(size_t)(2 * c + ch) * H + i] = t >= 0 ? row[t] : hin[(int64_t)H + t];
            }
        }
    }
}

}  // namespace

size_t fms_front_lds(uint32_t N, uint32_t d) { return sizeof(float2) * (N - 1 + FT) + sizeof(float) * (2 * N + N - 1 + d + FT); }

int launch_fmstereo(const float *mpx, float *out, const FmsBufs &b, const FmsLaunch &l, hipStream_t s, hipEvent_t *ev)
{
    if (!l.C || !l.n) return 0;
    const int cur = l.cur, nxt = cur ^ 1;
    const uint32_t tiles = (l.n + FT - 1) / FT, no = l.n / l.M;
    auto mark = [&](int i) -> int { if (ev) CSDR_HIP(hipEventRecord(ev[i], s)); return 0; };
    int r;
    if ((r = mark(0))) return r;
    hipLaunchKernelGGL(k_fms_front, dim3(tiles, l.C), dim3(FT), fms_front_lds(l.N, l.d), s, mpx, b.xh[cur], b.xh[nxt], b.hp, b.ha, b.p,
                       b.lpr, l.n, l.N, l.d, l.theta0, l.d_nco, l.scale_pilot, l.scale_audio);
    CSDR_HIP(hipGetLastError());
    if ((r = mark(1))) return r;
    hipLaunchKernelGGL(k_fms_pll, dim3((l.C + SL - 1) / SL), dim3(SL), 0, s, b.p, b.xh[cur], mpx, b.ub[cur], b.pll, l.C, l.n, l.N, l.d,
                       l.ustride, l.alpha, l.beta);
    CSDR_HIP(hipGetLastError());
    if ((r = mark(2))) return r;
    hipLaunchKernelGGL(k_fms_back, dim3(tiles, l.C), dim3(FT), sizeof(float) * (2 * l.N - 1 + FT), s, b.ub[cur], b.ub[nxt], b.ha, b.lpr,
                       b.lr, l.n, l.N, l.ustride, l.scale_audio);
    CSDR_HIP(hipGetLastError());
    if ((r = mark(3))) return r;
    hipLaunchKernelGGL(k_fms_deemph, dim3((2 * l.C + SL - 1) / SL), dim3(SL), 0, s, b.lr, b.bq, 2 * l.C, l.n, l.b0, l.b1, l.b2, l.a1, l.a2);
    CSDR_HIP(hipGetLastError());
    if ((r = mark(4))) return r;
    hipLaunchKernelGGL(k_fms_decim, dim3(no ? (no + 255) / 256 : 1, l.C), dim3(256), 0, s, b.lr, out, l.n, l.M, b.hdec, l.h_dec_len,
                       b.dh[cur], b.dh[nxt]);
    CSDR_HIP(hipGetLastError());
    return mark(5);
}

}  // namespace csdr
