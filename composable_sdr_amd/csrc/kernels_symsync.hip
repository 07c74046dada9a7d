// symSyncR k m beta M (Liquid.chs:244-282): liquid's symsync_rrrf on C independent F32 streams.
//   k_symsync : symsync_rrrf_step per input sample, one lane per stream, 64 streams per wave        sequential in t
// Input blocks of SB samples are staged through LDS behind the last L - 1 samples of every stream (L = h_sub_len = 2 k m);
// both filter banks sit in LDS tap-major ([tap][phase]): the lanes of a wave read different phases b at the same tap, which
// lands them on different banks (or one broadcast).  Every stream's state lives in HBM between calls.
// Arithmetic contract: plain f32, no contraction, each dot product summed oldest sample first starting from the first
// product, roundf for b and a correctly rounded / k.  The output is the same for every chunking of the stream, bit for bit,
// and tests/symsync_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int SL = 64;      // streams per workgroup: one wave, one lane each
constexpr int SB = 32;      // input samples per LDS block

__device__ __forceinline__ uint32_t sy_stride(uint32_t L) { const uint32_t w = L - 1 + SB; return w | 1u; }   // odd: no conflicts

// sum_j bank[j M + b] w[j], j = 0 (oldest) .. L - 1 (newest), starting from the first product
__device__ __forceinline__ float sy_dot(const float *bank, const float *w, uint32_t L, uint32_t M, int b)
{
    float acc = bank[b] * w[0];
#pragma unroll 8
    for (uint32_t j = 1; j < L; j++) acc = acc + bank[j * M + b] * w[j];   // unrolled: the LDS reads issue ahead of the add chain
    return acc;
}

// LDS: mf[L M] | dmf[L M] | xs[SL][stride(L)]  (xs row: the last L - 1 samples, then the block)
__global__ __launch_bounds__(SL) void k_symsync(const float *__restrict__ X, float *__restrict__ Y, uint32_t *__restrict__ NY,
                                                const float *__restrict__ gmf, const float *__restrict__ gdmf, float *__restrict__ hist,
                                                SymsyncState *__restrict__ st, uint32_t *__restrict__ fault_any, SymsyncLaunch l)
{
    extern __shared__ float lds[];
    const uint32_t L = l.L, M = l.M, LM = L * M, XS = sy_stride(L), H = L - 1;
    float *smf = lds, *sdmf = lds + LM, *xs = lds + 2 * LM;
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * SL, nc = min((uint32_t)SL, l.C - c0), n = l.n, cap = l.cap;
    for (uint32_t i = lane; i < LM; i += SL) { smf[i] = gmf[i]; sdmf[i] = gdmf[i]; }
    for (uint32_t e = lane; e < SL * H; e += SL) {
        const uint32_t rw = e / H, i = e % H;
        xs[rw * XS + i] = rw < nc ? hist[(size_t)(c0 + rw) * H + i] : 0.f;
    }
    // element e = lane + SL q of a block (q < SB): stream row e / SB, step e % SB
    float qx[SB];
    auto load = [&](uint32_t blk) {
#pragma unroll
        for (int q = 0; q < SB; q++) {
            const uint32_t e = lane + SL * q, rw = e / SB, t = blk * SB + e % SB;
            qx[q] = (rw < nc && t < n) ? X[(size_t)(c0 + rw) * n + t] : 0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < SB; q++) {
            const uint32_t e = lane + SL * q;
            xs[(e / SB) * XS + H + e % SB] = qx[q];
        }
    };
    const bool act = lane < nc;
    SymsyncState s{};
    if (act) s = st[c0 + lane];
    const float fM = (float)M;
    uint32_t cnt = 0;
    bool run = act && !s.fault;
    float *yrow = Y + (size_t)(c0 + (act ? lane : 0)) * cap;
    float *row = xs + lane * XS;
    const uint32_t nb = (n + SB - 1) / SB;
    if (nb) { load(0); stage(); }
    __syncthreads();
    for (uint32_t blk = 0; blk < nb; blk++) {
        if (blk + 1 < nb) load(blk + 1);                               // in flight while the recurrence runs
        const uint32_t steps = min((uint32_t)SB, n - blk * SB);
        for (uint32_t j = 0; j < steps && run; j++) {
            const float *w = row + j;                                  // window: w[0] oldest .. w[L - 1] = this sample
            int b = s.b;
            // symsync_rrrf_step's `while (b < npfb)`, bounded by the call's remaining output capacity
            for (uint32_t it = cnt; it < cap && b < (int)M; it++) {
                if (b < 0) { run = false; break; }                     // a bank index below 0 (never with del > 0)
                const float mf = sy_dot(smf, w, L, M, b);
                yrow[cnt++] = mf / l.kf;
                if (s.decim == l.k_out) {
                    s.decim = 0;
                    const float dmf = sy_dot(sdmf, w, L, M, b);
                    float q = mf * dmf;                                // Re(conj(mf) dmf)
                    q = q > 1.f ? 1.f : (q < -1.f ? -1.f : q);
                    const float v2 = s.v1;                             // iirfiltsos_rrrf, direct form II
                    s.v1 = s.v0;
                    s.v0 = (q - l.a1 * s.v1) - l.a2 * v2;
                    s.q_hat = (l.b0 * s.v0 + l.b1 * s.v1) + l.b2 * v2;
                    s.rate = s.rate + l.rate_adj * s.q_hat;
                    s.del = s.rate + s.q_hat;
                    if (!(s.del > 0.f)) { run = false; break; }        // would step backwards or stall: faulted
                }
                s.decim++;
                s.tau = s.tau + s.del;
                s.bf = s.tau * fM;
                if (!(s.bf < 8388608.f)) { run = false; break; }      // beyond 2^23 roundf has no integer meaning left
                b = (int)roundf(s.bf);
            }
            if (!run) break;
            if (b < (int)M) { run = false; break; }                   // more than cap outputs in this call: faulted
            s.tau = s.tau - 1.f;
            s.bf = s.bf - fM;
            s.b = b - (int)M;
        }
        if (act && !run) s.fault = 1;
        __syncthreads();
        if (act) {                                                     // this lane's row: keep the last L - 1 samples in front
            for (uint32_t i = 0; i < H; i++) row[i] = row[i + steps];
        }
        __syncthreads();
        if (blk + 1 < nb) stage();
        __syncthreads();
    }
    if (act) {
        for (uint32_t i = 0; i < H; i++) hist[(size_t)(c0 + lane) * H + i] = row[i];
        if (!run) s.fault = 1;
        st[c0 + lane] = s;
        NY[c0 + lane] = cnt;
        if (s.fault) *fault_any = 1u;
    }
}

}  // namespace

int launch_symsync(const float *x, float *y, uint32_t *ny, const float *mf, const float *dmf, float *hist, SymsyncState *st,
                   uint32_t *fault_any, const SymsyncLaunch &l, hipStream_t s)
{
    if (!l.C) return 0;
    const size_t lds = sizeof(float) * (2 * (size_t)l.L * l.M + (size_t)SL * ((l.L - 1 + SB) | 1u));
    hipLaunchKernelGGL(k_symsync, dim3((l.C + SL - 1) / SL), dim3(SL), lds, s, x, y, ny, mf, dmf, hist, st, fault_any, l);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
