// symSyncC m k (Liquid.chs:177-242): liquid's symsync_crcf on C independent CF32 streams with real banks.
//   k_symsyncc : symsync_crcf_step per input sample, one lane per stream, 64 streams per wave       sequential in t
// The structure is k_symsync's (kernels_symsync.hip): input blocks of SB samples staged through LDS behind the last L - 1
// samples of every stream (L = h_sub_len = 2 k m), both banks tap-major in LDS, every stream's SymsyncState in HBM.  A window
// holds interleaved (re, im) pairs read 8 bytes at a time; the row stride is odd in pairs, so the 32 lanes of a half wave
// meet 32 different pairs of the 64 banks.  At a loop instant the matched filter and its derivative are summed in one pass over
// the window: four independent add chains on shared window reads.
// Arithmetic contract: plain f32, no contraction; re and im of every dot product are two independent sums, oldest sample
// first starting from the first product; q = mf.re dmf.re + mf.im dmf.im (two rounded products, one add); roundf for b and
// a correctly rounded / k.  The output is the same for every chunking of the stream, bit for bit, and
// tests/symsyncc_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int SL = 64;      // streams per workgroup: one wave, one lane each
constexpr int SB = 32;      // input samples per LDS block

__host__ __device__ __forceinline__ uint32_t syc_stride(uint32_t L) { const uint32_t w = L - 1 + SB; return w | 1u; }   // pairs; odd

// mf = sum_j bank[j M + b] w[j], j = 0 (oldest) .. L - 1 (newest), re and im apart, each starting from its first product
__device__ __forceinline__ float2 syc_dot(const float *bank, const float2 *w, uint32_t L, uint32_t M, int b)
{
    const float h0 = bank[b];
    const float2 x0 = w[0];
    float re = h0 * x0.x, im = h0 * x0.y;
#pragma unroll 8
    for (uint32_t j = 1; j < L; j++) {
        const float h = bank[j * M + b];
        const float2 x = w[j];
        re = re + h * x.x;
        im = im + h * x.y;
    }
    return make_float2(re, im);
}

// the same sums for both banks in one pass over the window
__device__ __forceinline__ void syc_dot2(const float *mfb, const float *dmfb, const float2 *w, uint32_t L, uint32_t M, int b,
                                         float2 &mf, float2 &dmf)
{
    const float h0 = mfb[b], g0 = dmfb[b];
    const float2 x0 = w[0];
    float re = h0 * x0.x, im = h0 * x0.y, dre = g0 * x0.x, dim = g0 * x0.y;
#pragma unroll 8
    for (uint32_t j = 1; j < L; j++) {
        const float h = mfb[j * M + b], g = dmfb[j * M + b];
        const float2 x = w[j];
        re = re + h * x.x;
        im = im + h * x.y;
        dre = dre + g * x.x;
        dim = dim + g * x.y;
    }
    mf = make_float2(re, im);
    dmf = make_float2(dre, dim);
}

// LDS: mf[L M] | dmf[L M] | xs[SL][stride(L)] pairs  (xs row: the last L - 1 samples, then the block)
__global__ __launch_bounds__(SL) void k_symsyncc(const float2 *__restrict__ X, float2 *__restrict__ Y, uint32_t *__restrict__ NY,
                                                 const float *__restrict__ gmf, const float *__restrict__ gdmf,
                                                 float2 *__restrict__ hist, SymsyncState *__restrict__ st,
                                                 uint32_t *__restrict__ fault_any, SymsyncLaunch l)
{
    extern __shared__ float2 ldsc[];
    const uint32_t L = l.L, M = l.M, LM = L * M, XS = syc_stride(L), H = L - 1;
    float *smf = reinterpret_cast<float *>(ldsc), *sdmf = smf + LM;
    float2 *xs = ldsc + LM;                                            // 2 LM floats = LM pairs: 8-byte aligned
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * SL, nc = min((uint32_t)SL, l.C - c0), n = l.n, cap = l.cap;
    for (uint32_t i = lane; i < LM; i += SL) { smf[i] = gmf[i]; sdmf[i] = gdmf[i]; }
    for (uint32_t e = lane; e < SL * H; e += SL) {
        const uint32_t rw = e / H, i = e % H;
        xs[rw * XS + i] = rw < nc ? hist[(size_t)(c0 + rw) * H + i] : make_float2(0.f, 0.f);
    }
    // element e = lane + SL q of a block (q < SB): stream row e / SB, step e % SB
    float2 qx[SB];
    auto load = [&](uint32_t blk) {
#pragma unroll
        for (int q = 0; q < SB; q++) {
            const uint32_t e = lane + SL * q, rw = e / SB, t = blk * SB + e % SB;
            qx[q] = (rw < nc && t < n) ? X[(size_t)(c0 + rw) * n + t] : make_float2(0.f, 0.f);
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
    float2 *yrow = Y + (size_t)(c0 + (act ? lane : 0)) * cap;
    float2 *row = xs + lane * XS;
    const uint32_t nb = (n + SB - 1) / SB;
    if (nb) { load(0); stage(); }
    __syncthreads();
    for (uint32_t blk = 0; blk < nb; blk++) {
        if (blk + 1 < nb) load(blk + 1);                               // in flight while the recurrence runs
        const uint32_t steps = min((uint32_t)SB, n - blk * SB);
        for (uint32_t j = 0; j < steps && run; j++) {
            const float2 *w = row + j;                                 // window: w[0] oldest .. w[L - 1] = this sample
            int b = s.b;
            // symsync_crcf_step's `while (b < npfb)`, bounded by the call's remaining output capacity
            for (uint32_t it = cnt; it < cap && b < (int)M; it++) {
                if (b < 0) { run = false; break; }                     // a bank index below 0 (never with del > 0)
                const bool loop = s.decim == l.k_out;                  // a loop instant: MF and dMF in one pass
                float2 mf, dmf = make_float2(0.f, 0.f);
                if (loop) syc_dot2(smf, sdmf, w, L, M, b, mf, dmf);
                else mf = syc_dot(smf, w, L, M, b);
                yrow[cnt++] = make_float2(mf.x / l.kf, mf.y / l.kf);
                if (loop) {
                    s.decim = 0;
                    const float qr = mf.x * dmf.x, qi = mf.y * dmf.y;
                    float q = qr + qi;                                 // Re(conj(mf) dmf)
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

size_t symsyncc_lds_bytes(uint32_t L, uint32_t M) { return sizeof(float) * 2 * (size_t)L * M + sizeof(float2) * (size_t)SL * syc_stride(L); }

int launch_symsyncc(const float2 *x, float2 *y, uint32_t *ny, const float *mf, const float *dmf, float2 *hist, SymsyncState *st,
                    uint32_t *fault_any, const SymsyncLaunch &l, hipStream_t s)
{
    if (!l.C) return 0;
    const size_t lds = symsyncc_lds_bytes(l.L, l.M);
    if (lds > SYMSYNCC_MAX_LDS) { set_error("symsync: complex rows need %zu bytes of LDS > %zu", lds, SYMSYNCC_MAX_LDS); return -1; }
    hipLaunchKernelGGL(k_symsyncc, dim3((l.C + SL - 1) / SL), dim3(SL), lds, s, x, y, ny, mf, dmf, hist, st, fault_any, l);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
